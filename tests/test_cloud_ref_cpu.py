"""CPU: the point-cloud back end's restatement (tests/cloud_ref.py) against the lidar front end's restatement (the cloud of a metres map,
projected and rasterised again, is that map bit for bit), against the dataloader's inverse-depth encoding, and on hand-made maps:
the order, the frame_offsets and every validity clause.  test_gpu_cloud.py ties the kernels to the restatement."""
import numpy as np
import pytest

from tests import cloud_ref as ref
from tests import lidar_ref

MAX_DEPTH = 100.0
ENCODING_BOUND = 4 * 2.0 ** -24 * MAX_DEPTH


def intrinsics(size):
    """nuScenes' front camera scaled to an image of `size`, fx != fy."""
    k = size[1] / 1600.0
    return np.array([[1266.4 * k, 0.0, 816.3 * k], [0.0, 1270.9 * k, 491.5 * k], [0.0, 0.0, 1.0]])


def sparse_metres(rs, B, h, w, fill=0.3):
    d = rs.uniform(2.5, 100.0, size=(B, h, w)).astype(np.float32)
    d[rs.uniform(size=d.shape) > fill] = 0.0
    return d


# s >= 2 only: at s = 1 the first row and column have the full-resolution coordinate (0 + 0.5) * 1 - 0.5 = 0, which the projection's
# strict 0 < px refuses, so those pixels do not come back.
@pytest.mark.parametrize("size,s,cut", [((40, 64), 2, 3), ((45, 66), 3, 2), ((900, 1600), 2, 34)])
def test_round_trip_through_the_lidar_restatement(size, s, cut):
    rs = np.random.RandomState(11)
    B = 2
    h, w = size[0] // s - cut, size[1] // s
    depth = sparse_metres(rs, B, h, w)
    K = intrinsics(size)
    cloud = ref.point_cloud(depth, K, s, cut, stride=1, encoding="metres")
    n = int(cloud["frame_offsets"][-1])
    assert n == (depth > 0).sum() >= 100 and len(cloud["xyz"]) == n
    eye = np.eye(4)[None, :3]
    proj = lidar_ref.project(cloud["xyz"].astype(np.float64), np.zeros(n, dtype=np.int32), cloud["frame_offsets"], eye, eye, np.zeros((1, 4)),
                             K, image_size=size, min_distance=0.0, min_z=0.0)
    assert proj["valid"].all()
    _, back, _ = lidar_ref.ground_truth(proj, cloud["frame_offsets"], K, size, s, cut)
    assert back.dtype == depth.dtype and np.array_equal(back, depth)


def test_inverse_encoding_of_the_dataloader_decodes_within_three_roundings():
    rs = np.random.RandomState(12)
    h, w = 17, 32
    d = rs.uniform(0.0, 120.0, size=(2, h, w)).astype(np.float32)
    d[0, :4] = 0.0
    d[0, 4, :4] = (MAX_DEPTH, 99.99999, 1e-3, 2.5)
    g = np.clip(d, 0, np.float32(MAX_DEPTH))                                   # dataloader.py:240-245, in float32
    pos = g > 0
    g[pos] = (np.float32(MAX_DEPTH) - g[pos]) * (np.float32(1) / np.float32(MAX_DEPTH))
    assert g.dtype == np.float32
    points, valid = ref.unproject(g, intrinsics((40, 64)), 2, 3, MAX_DEPTH, "inverse", skip_empty=True)
    assert not valid[d == 0].any() and not valid[d >= MAX_DEPTH].any()       # no ground truth, and what the clip sends to 0
    inside = (d > 0) & (d < MAX_DEPTH) & (g > 0)
    assert valid[inside].all() and inside.sum() > 500
    err = np.abs(points[..., 2].astype(np.float64) - d.astype(np.float64))[inside]
    print(f"decode error: max {err.max():.3e}, bound {ENCODING_BOUND:.3e}")
    assert err.max() <= ENCODING_BOUND
    # without skip_empty a zero is max_depth metres: a prediction's far plane
    points, valid = ref.unproject(g, intrinsics((40, 64)), 2, 3, MAX_DEPTH, "inverse")
    assert valid[d == 0].all() and (points[..., 2][d == 0] == np.float32(MAX_DEPTH)).all()


def hand_map():
    """Two 3 x 4 frames in metres; image 8 x 8, s = 2, y_cutoff = 1."""
    nan, inf = np.nan, np.inf
    return np.array([[[5.0, 0.0, 7.0, nan], [-1.0, 9.0, inf, 11.0], [12.0, 13.0, -inf, 15.0]],
                     [[0.0, 0.0, 0.0, 0.0], [21.0, 22.0, 23.0, 24.0], [0.0, 0.0, 0.0, 30.0]]], dtype=np.float32)


HAND = dict(K=np.array([[4.0, 0.0, 3.5], [0.0, 8.0, 4.5], [0.0, 0.0, 1.0]]), s=2, y_cutoff=1, encoding="metres")


def pixels(cloud):
    off = cloud["frame_offsets"]
    return [[int(p) for p in cloud["pixel"][off[b]:off[b + 1]]] for b in range(len(off) - 1)]


def test_order_offsets_and_arithmetic_on_hand_made_maps():
    d = hand_map()
    c = ref.point_cloud(d, **HAND)
    assert pixels(c) == [[0, 2, 5, 7, 8, 9, 11], [4, 5, 6, 7, 11]]           # r * w + c, ascending inside a frame
    assert list(c["frame_offsets"]) == [0, 7, 12] and c["frame_offsets"].dtype == np.int32
    assert c["xyz"].dtype == np.float32 and c["xyz"].shape == (12, 3)
    # pixel (r, c) = (1, 1) of frame 0, 9 m: xf = 1.5 * 2 - 0.5 = 2.5, yf = (1 + 1 + 0.5) * 2 - 0.5 = 4.5
    assert list(c["xyz"][2]) == [(2.5 - 3.5) / 4.0 * 9.0, 0.0, 9.0]
    # the last pixel of frame 1, 30 m: xf = 6.5, yf = 6.5; Y uses fy
    assert list(c["xyz"][11]) == [(6.5 - 3.5) / 4.0 * 30.0, (6.5 - 4.5) / 8.0 * 30.0, 30.0]
    T = np.array([[0.0, 0.0, 1.0, 0.5], [-1.0, 0.0, 0.0, 0.25], [0.0, -1.0, 0.0, 2.0]])      # camera axes to x forward, z up
    t = ref.point_cloud(d, T=T, **HAND)
    assert list(t["xyz"][11]) == [30.5, -22.5 + 0.25, -7.5 + 2.0]
    per_frame = ref.point_cloud(d, T=np.stack([np.eye(4)[:3], T]), **HAND)
    assert np.array_equal(per_frame["xyz"][:7], c["xyz"][:7]) and np.array_equal(per_frame["xyz"][7:], t["xyz"][7:])
    s2 = ref.point_cloud(d, stride=2, **HAND)                                 # rows 0, 2 and columns 0, 2
    assert pixels(s2) == [[0, 2, 8], []] and list(s2["frame_offsets"]) == [0, 3, 3]
    s3 = ref.point_cloud(d, stride=3, **HAND)                                 # row 0 and columns 0, 3
    assert pixels(s3) == [[0], []]
    organised, valid = ref.unproject(d, **HAND)
    assert valid.sum() == 12 and not organised[valid == 0].any()
    assert np.array_equal(organised[valid != 0], c["xyz"])


def test_every_validity_clause_on_hand_made_maps():
    d = hand_map()
    assert pixels(ref.point_cloud(d, min_range=9.0, max_range=23.0, **HAND)) == [[5, 7, 8, 9, 11], [4, 5, 6]]       # both ends inclusive
    mask = np.ones((2, 3, 4), dtype=np.uint8)
    mask[0, 0] = 0
    mask[1, 1, 1] = 0
    mask[0, 2, 3] = 255
    assert pixels(ref.point_cloud(d, mask=mask, **HAND)) == [[5, 7, 8, 9, 11], [4, 6, 7, 11]]
    labels = np.arange(24, dtype=np.uint8).reshape(2, 3, 4) % 5
    labels[1, 2, 3] = 255
    kept = ref.point_cloud(d, labels=labels, keep={0, 3, 255}, **HAND)
    assert pixels(kept) == [[0, 5, 8], [6, 11]] and list(kept["label"]) == [0, 0, 3, 3, 255]
    table = np.zeros(256, dtype=np.uint8)
    table[[0, 3, 255]] = 7
    assert pixels(ref.point_cloud(d, labels=labels, keep=table, **HAND)) == [[0, 5, 8], [6, 11]]
    image = np.arange(72, dtype=np.uint8).reshape(2, 3, 4, 3)
    assert [list(v) for v in ref.point_cloud(d, image=image, **HAND)["rgb"][:2]] == [[0, 1, 2], [6, 7, 8]]
    # inverse encoding: p = 0 is max_depth metres unless skip_empty; p = 1 is 0 m and p > 1 is behind the camera; NaN and inf never pass
    p = np.array([[[0.0, 1.0, 0.5, 1.5], [-0.5, np.nan, np.inf, -np.inf], [0.25, 0.0, 0.999, 2.0]]], dtype=np.float32)
    kw = dict(HAND, encoding="inverse", max_depth=80.0)
    far = ref.point_cloud(p, **kw)
    assert pixels(far) == [[0, 2, 4, 8, 9, 10]]
    assert [float(z) for z in far["xyz"][:, 2]] == [80.0, 40.0, 120.0, 60.0, 80.0, float(np.float32(80.0 * (1.0 - float(np.float32(0.999)))))]
    assert pixels(ref.point_cloud(p, skip_empty=True, **kw)) == [[2, 4, 8, 10]]
    assert pixels(ref.point_cloud(p, max_range=80.0, **kw)) == [[0, 2, 8, 9, 10]]
    # metres: skip_empty changes nothing, 0 and negatives are never points
    assert pixels(ref.point_cloud(d, skip_empty=True, **HAND)) == pixels(ref.point_cloud(d, **HAND))
    nothing = ref.point_cloud(np.zeros((3, 3, 4), dtype=np.float32), **HAND)
    assert list(nothing["frame_offsets"]) == [0, 0, 0, 0] and nothing["xyz"].shape == (0, 3)
