"""Seeded inputs of the lidar front end's tests, shared by test_lidar_ref_cpu.py (which checks their conditions on the restatement) and
test_gpu_lidar.py (which runs the kernels on them)."""
import os

import numpy as np

from tests import lidar_ref as ref


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def load_fixture(golden_dir):
    """tests/golden/lidar_gt.npz with flow_im made dense again (it is stored at rasterised pixels only) and a frame axis on the maps."""
    f = dict(np.load(os.path.join(golden_dir, "lidar_gt.npz")))
    size, s, cut = tuple(int(v) for v in f["image_size"]), int(f["downsample_scale"]), int(f["y_cutoff"])
    h, w = size[0] // s - cut, size[1] // s
    flow_im = np.zeros((1, h, w, 2), dtype=np.float32)
    flow_im[0, f["flow_rows"].astype(int), f["flow_cols"].astype(int)] = f["flow_values"]
    proj = {k: f[k] for k in ref.PROJ_KEYS + ("low_h", "in_box")}
    stages = {"raster": {}, "box": dict(seg=f["seg"][None], corners=f["corners"], corner_offsets=offsets_of([len(f["corners"])])), }
    stages["flow"] = dict(stages["box"], flow_im=flow_im, thres=float(f["thres"]))
    return dict(f=f, proj=proj, off=offsets_of([len(f["x1"])]), K=f["K"], size=size, s=s, cut=cut, shape=(h, w), stages=stages)


def intrinsics(h, w, B=None):
    """A pinhole matrix for an h x w image (fy != fx: the reference divides v by fx); B given: one per frame, each a little different."""
    def one(j):
        return np.array([[0.8 * w + j, 0.0, 0.51 * w - j], [0.0, 0.83 * w, 0.55 * h + 0.5 * j], [0.0, 0.0, 1.0]])
    return one(0.0) if B is None else np.stack([one(1.0 + 0.37 * b) for b in range(B)])


def raster_points(n, h, w, seed, n_depths=10):
    """n projected points for an h x w image: many per pixel, depths from a small set so that exact ties are common, some a double's
    ulp apart, coordinates past every border and on exact halves, and points the rasteriser has to skip."""
    rs = np.random.RandomState(seed)
    depths = rs.uniform(2, 80, size=n_depths)
    depths = np.concatenate([depths, np.nextafter(depths[:4], 0.0), np.nextafter(depths[:4], 100.0)])
    p = {"x1": rs.uniform(-4, w + 4, n), "y1": rs.uniform(-4, h + 4, n), "depth1": rs.choice(depths, n)}
    spot = rs.uniform(size=n) < 0.4                                                  # a hot spot of about 12 x 8 pixels at scale 2
    p["x1"][spot], p["y1"][spot] = rs.uniform(w / 2 - 12, w / 2 + 12, int(spot.sum())), rs.uniform(h / 2 - 8, h / 2 + 8, int(spot.sum()))
    for k in ("x1", "y1"):
        q = rs.uniform(size=n) < 0.1
        p[k][q] = 2.0 * rs.randint(0, min(h, w) // 2 - 1, int(q.sum())) + 1.5          # scaled value k + .5 at scale 2, .0 at scale 1 ...
        q = rs.uniform(size=n) < 0.1
        p[k][q] = 1.0 * rs.randint(0, min(h, w) - 1, int(q.sum())) + 0.5               # ... and the other way round
    p["x2"], p["y2"] = p["x1"] + rs.normal(0, 5, n), p["y1"] + rs.normal(0, 2, n)
    bad = rs.uniform(size=n) < 0.05                                                  # what the reference raises on or reads as empty
    for i in np.nonzero(bad)[0]:
        k = ("x1", "y1", "depth1", "x2", "y2", "depth1", "depth1")[i % 7]
        p[k][i] = (np.nan, np.inf, -np.inf, 0.0, -1.0)[(i // 7) % 5] if k == "depth1" else (np.nan, np.inf, -np.inf)[(i // 7) % 3]
    p["low_h"] = (rs.uniform(size=n) < 0.5).astype(np.uint8)
    p["in_box"] = (rs.uniform(size=n) < 0.25).astype(np.uint8)
    p["valid"] = (rs.uniform(size=n) < 0.9).astype(np.uint8)
    return p


def filters_for(rs, B, h_img, w_img, s, cut, box_counts, depths):
    """seg, corners, corner_offsets, flow_im for B frames: box_counts[b] boxes in frame b around the middle of the image, some corners
    out of view, one box in ten with none in view, one in ten with its farthest corner out of view; d_max values among the points' depths
    so that depth == d_max happens; a blocky seg; an image flow of the size of the lidar's."""
    h, w = h_img // s - cut, w_img // s
    boxes = []
    for b in range(B):
        for j in range(box_counts[b]):
            x0, y0 = rs.uniform(0.1 * w_img, 0.6 * w_img), rs.uniform(0.1 * h_img, 0.6 * h_img)
            x1, y1 = x0 + rs.uniform(4, 0.4 * w_img), y0 + rs.uniform(4, 0.4 * h_img)
            if j == 0:                                                              # the first box of a frame lies over the hot spot
                x0, y0, x1, y1 = 0.5 * w_img - 14, 0.5 * h_img - 9, 0.5 * w_img + 11, 0.5 * h_img + 7
            xs = np.array([x0, x1, x0, x1, x0 + 1, x1 - 1, x0 + 1, x1 - 1]) + rs.uniform(-1, 1, 8)
            ys = np.array([y0, y0, y1, y1, y0 + 1, y0 + 1, y1 - 1, y1 - 1]) + rs.uniform(-1, 1, 8)
            if j % 2:                                                               # bounds on exact halves / whole pixels
                xs[0], ys[0], xs[3], ys[3] = 2.0 * int(x0 / 2) + 1.5, 2.0 * int(y0 / 2) + 0.5, 2.0 * int(x1 / 2) + 1.5, 2.0 * int(y1 / 2) + 1.5
            ds = rs.uniform(2, 30, 8)
            ds[rs.randint(8)] = rs.choice(depths)                                   # often the largest: a point at exactly d_max
            view = (rs.uniform(size=8) < 0.8).astype(np.float64)
            kind = rs.randint(10) if j else 9
            if kind == 0:
                view[:] = 0.0
            elif kind == 1:
                view[int(np.argmax(ds))] = 0.0
            boxes.append(np.stack([xs, ys, ds, view], axis=1))
    corners = np.array(boxes, dtype=np.float64).reshape(-1, 8, 4)
    r, c = np.mgrid[0:h, 0:w]
    seg = np.stack([((r // 5 + c // 7 + b) % 3 != 0) for b in range(B)]).astype(np.uint8)
    flow_im = rs.normal(0, 2.0 / s, size=(B, h, w, 2)).astype(np.float32)
    return dict(seg=seg, corners=corners, corner_offsets=offsets_of(box_counts), flow_im=flow_im, thres=6.0 / s)


RAGGED = {
    "ragged": dict(size=(128, 192), s=2, cut=4, counts=(0, 1, 600, 37), boxes=(2, 0, 5, 1), per_frame_K=False),
    "integer_division": dict(size=(101, 150), s=2, cut=0, counts=(300, 80), boxes=(1, 3), per_frame_K=False),
    "scale1": dict(size=(48, 80), s=1, cut=3, counts=(250, 0, 90), boxes=(4, 1, 0), per_frame_K=False),
    "scale3_per_frame_K": dict(size=(100, 151), s=3, cut=5, counts=(200, 3, 150), boxes=(0, 1, 6), per_frame_K=True),
}


def ragged_case(name):
    c = RAGGED[name]
    h, w = c["size"]
    B, n = len(c["counts"]), sum(c["counts"])
    proj = raster_points(n, h, w, seed=len(name))
    off = offsets_of(c["counts"])
    for b, m in enumerate(c["counts"]):                     # the first point of a frame of one or a few is a good one
        if 0 < m <= 3:
            for k, v in zip(ref.PROJ_KEYS + ref.FLAG_KEYS, (0.6 * w, 0.7 * h, 7.0, 0.6 * w + 3.3, 0.7 * h - 1.1, 1, 0, 1)):
                proj[k][off[b]] = v
    K = intrinsics(h, w, B if c["per_frame_K"] else None)
    rs = np.random.RandomState(100 + len(name))
    filt = filters_for(rs, B, h, w, c["s"], c["cut"], c["boxes"], np.unique(proj["depth1"][np.isfinite(proj["depth1"])]))
    return dict(c, proj=proj, off=off, K=K, filters=filt, B=B)


def contention_case():
    """200,000 points on a 64 x 96 map, depths from 16 values: every pixel is fought over by about thirty points and most pixels see
    several points at their smallest depth."""
    n, size, s, cut = 200000, (128, 192), 2, 0
    proj = raster_points(n, size[0], size[1], seed=77, n_depths=8)
    rs = np.random.RandomState(78)
    depths = np.unique(proj["depth1"][np.isfinite(proj["depth1"]) & (proj["depth1"] > 0)])
    assert len(depths) == 16
    filt = filters_for(rs, 1, size[0], size[1], s, cut, (3,), depths)
    return dict(size=size, s=s, cut=cut, proj=proj, off=offsets_of([n]), K=intrinsics(*size), filters=filt, B=1)


# ---- projection -------------------------------------------------------------------------------------------------------------
def rigid4(rs, angle=0.05, shift=1.0):
    """A random small rotation (Rodrigues) and translation as a 4 x 4 matrix."""
    a = rs.normal(size=3)
    a /= np.linalg.norm(a)
    t = rs.uniform(-angle, angle)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx
    M[:3, 3] = rs.uniform(-shift, shift, 3)
    return M


# the sensor looks along +x with y to the left and z up, the cameras along +z with x to the right and y down
AXES = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 1.2], [1.0, 0.0, 0.0, -0.5], [0.0, 0.0, 0.0, 1.0]])


def box_pose(centre, yaw):
    M = np.eye(4)
    M[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
    M[:3, 3] = centre
    return M


def projection_case():
    """About 2,000 points of 3 sweeps with 0, 1 and 5 box entries in 2 frames (per-frame K) and 30 trailing points that belong to no
    frame.  Box 3 is in sweeps 1 and 2, every other box in sweep 2 only.  Entries 2 and 3 are nested (the outer one first), entries 4
    and 5 too (the inner one first): their shared points go to the first.  A fifth of the points are drawn inside or just around
    the boxes."""
    rs = np.random.RandomState(41)
    S, counts = 3, (500, 700, 800)
    cam1 = np.stack([(rigid4(rs) @ AXES)[:3] for _ in range(S)])
    cam2 = np.stack([(rigid4(rs) @ AXES)[:3] for _ in range(S)])
    car_z = np.stack([(rigid4(rs, 0.02, 0.1) @ np.array([[1.0, 0, 0, 0.9], [0, 1, 0, 0], [0, 0, 1, 1.84], [0, 0, 0, 1]]))[2] for _ in range(S)])
    # (sweep, box id, centre, yaw, (l, w, h))
    spec = [(1, 3, (18.0, 2.0, -0.6), 0.3, (4.6, 1.9, 1.7)),
            (2, 5, (30.0, -6.0, -0.4), -0.5, (9.0, 2.6, 3.1)), (2, 3, (14.0, 4.0, -0.7), 0.2, (4.6, 1.9, 1.7)),
            (2, 0, (14.1, 4.1, -0.8), 0.25, (2.0, 0.9, 0.8)), (2, 6, (40.0, 3.0, -0.2), 1.2, (0.8, 0.7, 1.8)),
            (2, 1, (40.2, 3.1, -0.1), 1.1, (5.0, 2.2, 2.0))]
    poses = [box_pose(c, yaw) for (_, _, c, yaw, _) in spec]
    entries = np.array([np.concatenate([np.linalg.inv(P)[:3].reshape(12), 0.5 * np.array(sz)]) for P, (_, _, _, _, sz) in zip(poses, spec)])
    box_id = np.array([k for (_, k, *_r) in spec], dtype=np.int32)
    sweep_boxes = np.array([0, 0, 1, 6], dtype=np.int32)
    n_boxes = 7
    cam1_box = np.stack([(rigid4(rs, 0.05, 1.0) @ AXES @ box_pose((20.0 + 3 * k, 1.0 - k, -0.5), 0.1 * k))[:3] for k in range(n_boxes)])
    cam2_box = np.stack([(rigid4(rs, 0.05, 1.0) @ AXES @ box_pose((20.5 + 3 * k, 1.1 - k, -0.5), 0.1 * k + 0.02))[:3] for k in range(n_boxes)])
    vehicle = np.array([1, 0, 1, 1, 0, 1, 0], dtype=np.uint8)
    pts, sw = [], []
    for s, n in enumerate(counts + (30,)):
        p = np.stack([rs.uniform(0.3, 100, n), rs.uniform(-60, 60, n), rs.uniform(-4, 7, n)], axis=1)
        near = rs.uniform(size=n) < 0.15
        p[near, 0], p[near, 1] = rs.uniform(-4, 4, int(near.sum())), rs.uniform(-4, 4, int(near.sum()))
        ground = rs.uniform(size=n) < 0.3
        p[ground, 2] = rs.uniform(-2.2, 0.6, int(ground.sum()))
        mine = [e for e in range(len(spec)) if spec[e][0] == s]
        for i in np.nonzero(rs.uniform(size=n) < (0.25 if mine else 0.0))[0]:
            e = mine[rs.randint(len(mine))]
            q = rs.uniform(-1.3, 1.3, 3) * entries[e, 12:]
            p[i] = (poses[e] @ np.append(q, 1.0))[:3]
        pts.append(p)
        sw.append(np.full(n, s if s < S else rs.randint(S), dtype=np.int32))
    pts, sw = np.concatenate(pts), np.concatenate(sw)
    K = np.stack([np.array([[1266.4 + 3 * b, 0, 816.3 - b], [0, 1270.9 + b, 491.5 + 2 * b], [0, 0, 1.0]]) for b in range(2)])
    off = offsets_of((counts[0] + counts[1], counts[2]))
    c = dict(pts=pts, sw=sw, off=off, cam1=cam1, cam2=cam2, car_z=car_z, K=K, sweep_boxes=sweep_boxes, entries=entries, box_id=box_id,
             cam1_box=cam1_box, cam2_box=cam2_box, vehicle=vehicle, size=(900, 1600))
    # a point almost in a camera's plane Z = 0 has coordinates of any size, and their rounding errors with them: such points move 3 m on
    for _ in range(3):
        want = project_ref(c)
        big = np.abs(np.stack([want[k] for k in ref.PROJ_KEYS])).max(axis=0) > 1e5
        pts[big, 0] += 3.0
    return c


def project_ref(c, **kw):
    return ref.project(c["pts"], c["sw"], c["off"], c["cam1"], c["cam2"], c["car_z"], c["K"], c.get("sweep_boxes"), c.get("entries"),
                       c.get("box_id"), c.get("cam1_box"), c.get("cam2_box"), c.get("vehicle"), c["size"], **kw)


def boundary_case():
    """Identity rotations, axis permutations and dyadic numbers only, so every product and sum is exact on both sides.
    -> (case, expected) with expected = [(what, valid, low_h, in_box, box_entry)] per point."""
    cam = np.array([[0.0, -1.0, 0.0, 3.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])      # X = 3 - y, Y = -z, Z = x
    K = np.array([[1024.0, 0.0, 800.0], [0.0, 1024.0, 448.0], [0.0, 0.0, 1.0]])
    entry = np.concatenate([np.array([[1.0, 0, 0, -16.0], [0, 1.0, 0, -3.0], [0, 0, 1.0, 0.0]]).reshape(12), [2.0, 1.0, 0.75]])
    rows = [("inside the box", (16.5, 3.25, 0.25), 1, 0, 1, 0)]
    for axis, half in enumerate((2.0, 1.0, 0.75)):                                            # on each of the six faces: outside
        for sign in (-1.0, 1.0):
            p = [16.5, 3.25, 0.25]
            p[axis] = (16.0, 3.0, 0.0)[axis] + sign * half
            rows.append((f"on face {axis} {sign:+.0f}", tuple(p), 1, int(0.3 <= p[2] <= 2.0), 0, -1))
    rows += [("z_car exactly 0.3", (8.0, 3.0, 0.3), 1, 1, 0, -1), ("z_car just below 0.3", (8.0, 3.0, np.nextafter(0.3, 0.0)), 1, 0, 0, -1),
             ("z_car exactly 2.0", (64.0, 3.0, 2.0), 1, 1, 0, -1), ("z_car just above 2.0", (64.0, 3.0, np.nextafter(2.0, 3.0)), 1, 0, 0, -1),
             ("Z exactly min_z", (2.0, 3.0, -0.25), 1, 0, 0, -1), ("Z just below min_z", (np.nextafter(2.0, 0.0), 3.0, -0.25), 0, 0, 0, -1),
             ("px exactly 0", (4.0, 6.125, -0.25), 0, 0, 0, -1), ("px a quarter pixel", (4.0, 6.125 - 2.0 ** -10, -0.25), 1, 0, 0, -1),
             ("px exactly im_w", (4.0, -0.125, -0.25), 0, 0, 0, -1), ("px a quarter pixel inside", (4.0, -0.125 + 2.0 ** -10, -0.25), 1, 0, 0, -1),
             ("|x| = |y| = min_distance", (2.5, 2.5, -0.25), 1, 0, 0, -1),
             ("inside the min_distance square", (np.nextafter(2.5, 0.0), np.nextafter(2.5, 0.0), -0.25), 0, 0, 0, -1)]
    n = len(rows)
    case = dict(pts=np.array([r[1] for r in rows]), sw=np.zeros(n, dtype=np.int32), off=offsets_of([n]), cam1=cam[None], cam2=cam[None],
                car_z=np.array([[0.0, 0.0, 1.0, 0.0]]), K=K, sweep_boxes=np.array([0, 1], dtype=np.int32), entries=entry[None],
                box_id=np.zeros(1, dtype=np.int32), cam1_box=(cam @ np.array([[1.0, 0, 0, 16.0], [0, 1.0, 0, 3.0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]))[None],
                vehicle=np.ones(1, dtype=np.uint8), size=(900, 1600))
    case["cam2_box"] = case["cam1_box"]
    return case, [(r[0],) + r[2:] for r in rows]
