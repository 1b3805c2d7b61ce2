"""GPU: the radar front end (camradepth_amd.radar: project_radar, rasterize_radar, radar_inputs, RadarWorkspace) against the fixture the
reference's own rasteriser produced (tests/golden/radar_raster.npz) and against the NumPy restatement in tests/radar_ref.py.

The rasteriser is additions, divisions, a clip, a round-half-even and two roundings to fp32 -- all correctly rounded on both sides and
never contracted -- so it is compared bit for bit.  The projection has multiply-adds a compiler may contract: 1e-8 absolute, in pixels
and metres (the largest intermediate, fx * X, is about 1e5 with an ulp of 1.5e-11, over a handful of operations; a wrong formula shows
at 1e-3 or more)."""
import os

import numpy as np
import pytest
import torch

from tests import radar_ref as ref

pytestmark = pytest.mark.gpu

PROJECT_BOUND = 1e-8


@pytest.fixture(scope="module")
def radar():
    from camradepth_amd import radar as module
    return module


def cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def dev_proj(proj):
    d = {k: cuda(proj[k], np.float64) for k in ref.PROJ_KEYS}
    if proj.get("valid") is not None:
        d["valid"] = cuda(proj["valid"], np.uint8)
    return d


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def intrinsics(h, w, B=None):
    """A pinhole matrix for an h x w image (fy != fx: the reference divides v by fx); B given: one per frame, each a little different."""
    def one(j):
        return np.array([[0.8 * w + j, 0.0, 0.51 * w - j], [0.0, 0.83 * w, 0.55 * h + 0.5 * j], [0.0, 0.0, 1.0]])
    return one(0.0) if B is None else np.stack([one(1.0 + 0.37 * b) for b in range(B)])


def raster_points(n, h, w, seed):
    """n projected points for an h x w image: many per pixel, depths from a small set so that exact ties are common, some a double's
    ulp apart, coordinates past every border and on exact halves, and points the rasteriser has to skip."""
    rs = np.random.RandomState(seed)
    depths = rs.uniform(2, 80, size=10)
    depths = np.concatenate([depths, np.nextafter(depths[:4], 0.0), np.nextafter(depths[:4], 100.0)])
    p = {"x1": rs.uniform(-4, w + 4, n), "y1": rs.uniform(-4, h + 4, n), "depth1": rs.choice(depths, n), "v_comp": rs.uniform(0, 1.2, n)}
    spot = rs.uniform(size=n) < 0.4                                                  # a hot spot of about 12 x 8 pixels at scale 2
    p["x1"][spot], p["y1"][spot] = rs.uniform(w / 2 - 12, w / 2 + 12, int(spot.sum())), rs.uniform(h / 2 - 8, h / 2 + 8, int(spot.sum()))
    for k in ("x1", "y1"):
        q = rs.uniform(size=n) < 0.1
        p[k][q] = 2.0 * rs.randint(0, min(h, w) // 2 - 1, int(q.sum())) + 1.5          # scaled value k + .5 at scale 2, .0 at scale 1 ...
        q = rs.uniform(size=n) < 0.1
        p[k][q] = 1.0 * rs.randint(0, min(h, w) - 1, int(q.sum())) + 0.5               # ... and the other way round
    p["x2"], p["y2"] = p["x1"] + rs.normal(0, 5, n), p["y1"] + rs.normal(0, 2, n)
    p["v_comp"][rs.uniform(size=n) < 0.1] = 0.5
    p["v_comp"][rs.uniform(size=n) < 0.1] = np.nextafter(0.5, 1.0)
    bad = rs.uniform(size=n) < 0.05                                                  # what the reference raises on or reads as empty
    for i in np.nonzero(bad)[0]:
        k = ("x1", "y1", "depth1", "x2", "y2", "v_comp", "depth1", "depth1")[i % 8]
        p[k][i] = (np.nan, np.inf, -np.inf, 0.0, -1.0)[(i // 8) % 5] if k == "depth1" else (np.nan, np.inf, -np.inf)[(i // 8) % 3]
    p["valid"] = (rs.uniform(size=n) < 0.9).astype(np.uint8)
    good = np.nonzero(spot & ~bad & (p["valid"] == 1))[0]                            # on the pixel of a good point and nearer than any,
    j = good[good + 1 < n][0]                                                        # one that only a non-finite v_comp keeps out
    for k in ("x1", "y1", "x2", "y2"):
        p[k][j + 1] = p[k][j]
    p["depth1"][j + 1], p["v_comp"][j + 1], p["valid"][j + 1] = 0.5 * depths.min(), np.nan, 1
    return p


def run_raster(radar, proj, off, K, size, s, cut, **kw):
    out = radar.rasterize_radar(dev_proj(proj), cuda(off), cuda(K, np.float64), size, s, cut, **kw)
    torch.cuda.synchronize()
    return out["radar"], out["rad_vel"]


def assert_equal(got, want, what):
    want = torch.from_numpy(want) if isinstance(want, np.ndarray) else want
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} values differ; first at {i}: {got[i].item()!r} against {want[i].item()!r}")


def test_fixture_of_the_reference_rasteriser(radar, golden_dir):
    f = dict(np.load(os.path.join(golden_dir, "radar_raster.npz")))
    size, s, cut = tuple(int(v) for v in f["image_size"]), int(f["downsample_scale"]), int(f["y_cutoff"])
    assert (size, s, cut) == ((900, 1600), 2, 34)
    proj = {k: f[k] for k in ref.PROJ_KEYS}
    got_radar, got_vel = run_raster(radar, proj, offsets_of([len(f["x1"])]), f["K"], size, s, cut)
    want_radar, want_vel = np.zeros((1, 416, 800, 3), dtype=np.float32), np.zeros((1, 416, 800), dtype=np.float32)
    r, c = f["entries"][:, 0].astype(int), f["entries"][:, 1].astype(int)
    want_radar[0, r, c] = f["entries"][:, 2:5].astype(np.float32)
    want_vel[0, r, c] = f["entries"][:, 5].astype(np.float32)
    assert_equal(got_radar, want_radar, "radar")
    assert_equal(got_vel, want_vel, "rad_vel")


def v_comp_only_point(proj, off, size, s, cut, candidates):
    """The first point that the rasteriser skips for its v_comp alone (every other value is finite, depth1 > 0, valid, below the
    cutoff) and that is nearer than every candidate of its pixel, of which there is one at least; or None."""
    h_new, w_new = size[0] // s, size[1] // s
    with np.errstate(invalid="ignore"):
        frame = np.searchsorted(off, np.arange(len(proj["x1"])), side="right")
        pixel = (frame * h_new + np.rint(ref.scaled(proj["y1"], s, h_new - 1))) * w_new + np.rint(ref.scaled(proj["x1"], s, w_new - 1))
        rest = np.stack([np.asarray(proj[k]) for k in ref.PROJ_KEYS if k != "v_comp"])
        alone = ~np.isfinite(proj["v_comp"]) & np.isfinite(rest).all(axis=0) & (proj["depth1"] > 0) & (proj["valid"] == 1) & \
            (np.rint(ref.scaled(proj["y1"], s, h_new - 1)) >= cut)
    nearest = {}
    for j in np.nonzero(candidates)[0]:
        nearest[pixel[j]] = min(proj["depth1"][j], nearest.get(pixel[j], np.inf))
    return next((int(i) for i in np.nonzero(alone)[0] if proj["depth1"][i] < nearest.get(pixel[i], -np.inf)), None)


CASES = {
    "ragged": dict(size=(128, 192), s=2, cut=4, counts=(0, 1, 600, 37), per_frame_K=False),
    "integer_division": dict(size=(101, 150), s=2, cut=0, counts=(300, 80), per_frame_K=False),
    "scale1": dict(size=(48, 80), s=1, cut=3, counts=(250, 0, 90), per_frame_K=False),
    "scale3_per_frame_K": dict(size=(100, 151), s=3, cut=5, counts=(200, 3, 150), per_frame_K=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_batches_against_the_restatement(radar, name):
    c = CASES[name]
    h, w = c["size"]
    B, n = len(c["counts"]), sum(c["counts"])
    proj = raster_points(n, h, w, seed=len(name))
    off = offsets_of(c["counts"])
    K = intrinsics(h, w, B if c["per_frame_K"] else None)
    for b, m in enumerate(c["counts"]):                     # the first point of a frame of one or a few is a good one
        if 0 < m <= 3:
            for k, v in zip(ref.PROJ_KEYS + ("valid",), (0.6 * w, 0.7 * h, 7.0, 0.6 * w + 3.3, 0.7 * h - 1.1, 0.9, 1)):
                proj[k][off[b]] = v
    want_radar, want_vel = ref.rasterize(proj, off, K, c["size"], c["s"], c["cut"])
    assert want_radar.shape == (B, h // c["s"] - c["cut"], w // c["s"], 3)
    won = [int((want_radar[b, ..., 0] != 0).sum()) for b in range(B)]
    arrs = np.stack([np.asarray(proj[k]) for k in ref.PROJ_KEYS])
    with np.errstate(invalid="ignore"):
        candidates = (proj["valid"] == 1) & np.isfinite(arrs).all(axis=0) & (proj["depth1"] > 0) & \
                     (np.rint(ref.scaled(proj["y1"], c["s"], h // c["s"] - 1)) >= c["cut"])
    assert all((k == 0) == (m == 0) for k, m in zip(won, c["counts"])) and sum(won) <= candidates.sum() - 10      # pixels are fought over
    # a point that only its v_comp keeps out, on a pixel that is fought over: without it the maps are the same, with a finite v_comp not
    i = v_comp_only_point(proj, off, c["size"], c["s"], c["cut"], candidates)
    assert i is not None
    without = ref.rasterize({k: np.delete(np.asarray(v), i) for k, v in proj.items()}, off - (off > i), K, c["size"], c["s"], c["cut"])
    finite = ref.rasterize(dict(proj, v_comp=np.where(np.arange(n) == i, 0.9, proj["v_comp"])), off, K, c["size"], c["s"], c["cut"])
    assert np.array_equal(without[0], want_radar) and np.array_equal(without[1], want_vel)
    assert not (np.array_equal(finite[0], want_radar) and np.array_equal(finite[1], want_vel))
    got_radar, got_vel = run_raster(radar, proj, off, K, c["size"], c["s"], c["cut"])
    assert_equal(got_radar, want_radar, "radar")
    assert_equal(got_vel, want_vel, "rad_vel")
    # frames do not see each other's points: the frames in another order give the same maps in that order
    order = list(range(B))[::-1] if B == 2 else [2, 0, 3, 1][:B] if B == 4 else [1, 2, 0]
    idx = np.concatenate([np.arange(off[b], off[b + 1]) for b in order]).astype(int)
    perm = {k: np.asarray(v)[idx] for k, v in proj.items()}
    Kp = K[order] if K.ndim == 3 else K
    got_radar_p, got_vel_p = run_raster(radar, perm, offsets_of([c["counts"][b] for b in order]), Kp, c["size"], c["s"], c["cut"])
    assert_equal(got_radar_p, want_radar[order], "radar, frames permuted")
    assert_equal(got_vel_p, want_vel[order], "rad_vel, frames permuted")
    # without a mask every point counts
    nomask = {k: v for k, v in proj.items() if k != "valid"}
    want = ref.rasterize(nomask, off, K, c["size"], c["s"], c["cut"])
    got = run_raster(radar, nomask, off, K, c["size"], c["s"], c["cut"])
    assert_equal(got[0], want[0], "radar, no mask")
    assert_equal(got[1], want[1], "rad_vel, no mask")


def rigid(rs, angle=0.05, shift=1.0):
    """A random small rotation (Rodrigues) and translation as a 4 x 4 matrix."""
    a = rs.normal(size=3)
    a /= np.linalg.norm(a)
    t = rs.uniform(-angle, angle)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx
    M[:3, 3] = rs.uniform(-shift, shift, 3)
    return M


def sweeps(rs, S):
    """cam1_from_sensor, cam2_from_sensor [S,3,4] and lags [S,2] of both signs.  The sensor looks along +x with y to the left and z up,
    the cameras along +z with x to the right and y down."""
    axes = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 1.2], [1.0, 0.0, 0.0, -0.5], [0.0, 0.0, 0.0, 1.0]])
    cam1 = np.stack([(rigid(rs) @ axes)[:3] for _ in range(S)])
    cam2 = np.stack([(rigid(rs) @ axes)[:3] for _ in range(S)])
    return cam1, cam2, rs.uniform(-0.45, 0.45, size=(S, 2))


def sensor_points(rs, n, S_lo, S_hi):
    """n detections of the sweeps S_lo .. S_hi - 1: most in front of the sensor over a field wider and taller than the camera's, some
    around the close-range box, some too near for min_z, some behind."""
    pts = np.stack([rs.uniform(0.3, 100, n), rs.uniform(-60, 60, n), rs.uniform(-4, 7, n), rs.normal(0, 3, n), rs.normal(0, 3, n)], axis=1)
    near = rs.uniform(size=n) < 0.15
    pts[near, 0], pts[near, 1] = rs.uniform(-2, 2, int(near.sum())), rs.uniform(-2, 2, int(near.sum()))
    low = rs.uniform(size=n) < 0.1
    pts[low, 0], pts[low, 1] = rs.uniform(1.2, 4, int(low.sum())), rs.uniform(-1, 1, int(low.sum()))
    pts[rs.uniform(size=n) < 0.1, 3:] = 0.0
    return pts, rs.randint(S_lo, S_hi, n).astype(np.int32)


def make_sweep_case():
    """3 frames of 5 sweeps each at 900 x 1600 with per-frame intrinsics, 20 trailing points that belong to no frame, and its restatement."""
    rs = np.random.RandomState(5)
    counts, S = (260, 140, 200), 15
    cam1, cam2, lags = sweeps(rs, S)
    parts = [sensor_points(rs, n, 5 * b, 5 * b + 5) for b, n in enumerate(counts + (20,))]
    pts, sw = np.concatenate([p for p, _ in parts]), np.concatenate([s for _, s in parts])
    sw[-20:] = rs.randint(0, S, 20)
    K = np.stack([np.array([[1266.4 + 3 * b, 0, 816.3 - b], [0, 1270.9 + b, 491.5 + 2 * b], [0, 0, 1.0]]) for b in range(3)])
    off = offsets_of(counts)
    want = ref.project(pts, sw, off, cam1, cam2, lags, K, (900, 1600), 1.0, 2.0)
    return dict(pts=pts, sw=sw, off=off, cam1=cam1, cam2=cam2, lags=lags, K=K, want=want)


def test_projection_against_the_restatement(radar, sweep_case):
    c = sweep_case
    want, n_in = c["want"], int(c["off"][-1])
    m = want["margins"][:n_in]
    # both sides of every condition occur, and no compared quantity is within 1e-6 of its threshold on the restatement
    assert np.isfinite(m[:, :11]).all() and m.min() >= 1e-6, m.min()
    x, y = np.abs(c["pts"][:n_in, 0]), np.abs(c["pts"][:n_in, 1])
    assert ((x < 1) & (y < 1)).any() and ((x < 1) & (y >= 1)).any() and ((x >= 1) & (y < 1)).any()
    for Z, px, py in ((want["depth1"], want["x1"], want["y1"]),):
        Z, px, py = Z[:n_in], px[:n_in], py[:n_in]
        assert (Z < 2).any() and (Z < 0).any() and (px[Z >= 2] <= 0).any() and (px[Z >= 2] >= 1600).any()
        assert (py[Z >= 2] <= 0).any() and (py[Z >= 2] >= 900).any()
    assert (c["lags"] < 0).any() and (c["lags"] > 0).any()
    v = want["valid"]
    assert 0.1 < v[:n_in].mean() < 0.9 and not v[n_in:].any()
    got = radar.project_radar(cuda(c["pts"]), cuda(c["sw"]), cuda(c["off"]), cuda(c["cam1"]), cuda(c["cam2"]), cuda(c["lags"]), cuda(c["K"]),
                              (900, 1600), 1.0, 2.0)
    torch.cuda.synchronize()
    assert set(got) == set(ref.PROJ_KEYS) | {"valid"}
    assert_equal(got["valid"], want["valid"], "valid")
    for k in ref.PROJ_KEYS:
        assert got[k].dtype == torch.float64 and got[k].shape == (len(c["pts"]),)
        err = np.abs(got[k].cpu().numpy() - want[k])
        print(f"project_radar {k}: max |error| {err.max():.3e}")
        assert err.max() <= PROJECT_BOUND, (k, err.max(), int(err.argmax()))
    # one K for all frames; min_distance and min_z other than the defaults
    want1 = ref.project(c["pts"], c["sw"], c["off"], c["cam1"], c["cam2"], c["lags"], c["K"][1], (900, 1600), 2.5, 10.0)
    got1 = radar.project_radar(cuda(c["pts"]), cuda(c["sw"]), cuda(c["off"]), cuda(c["cam1"]), cuda(c["cam2"]), cuda(c["lags"]),
                               cuda(c["K"][1]), (900, 1600), 2.5, 10.0)
    assert want1["margins"][:n_in].min() >= 1e-6 and (want1["valid"] != want["valid"]).any()
    assert_equal(got1["valid"], want1["valid"], "valid, one K")
    assert np.abs(got1["x2"].cpu().numpy() - want1["x2"]).max() <= PROJECT_BOUND


def test_projection_of_nan_and_unknown_sweeps_is_invalid(radar):
    rs = np.random.RandomState(9)
    cam1, cam2, lags = sweeps(rs, 2)
    pts = np.tile(np.array([[30.0, 1.0, 0.5, 0.3, -0.2]]), (9, 1))
    for i in range(5):
        pts[i, i] = np.nan
    sw = np.array([0, 0, 0, 0, 0, 1, 2, -1, 0], dtype=np.int32)             # rows 6, 7: a sweep outside the tables
    K = np.array([[1266.4, 0, 816.3], [0, 1270.9, 491.5], [0, 0, 1.0]])
    want = ref.project(pts, sw, [0, 9], cam1, cam2, lags, K)
    assert list(want["valid"]) == [0, 0, 0, 0, 0, 1, 0, 0, 1]
    got = radar.project_radar(cuda(pts), cuda(sw), cuda(offsets_of([9])), cuda(cam1), cuda(cam2), cuda(lags), cuda(K))
    assert_equal(got["valid"], want["valid"], "valid")
    for k in ref.PROJ_KEYS:
        assert np.allclose(got[k].cpu().numpy(), want[k], rtol=0, atol=PROJECT_BOUND, equal_nan=True), k


@pytest.fixture(scope="module")
def sweep_case():
    return make_sweep_case()


def make_small_case():
    """4 frames at 128 x 192 from sensor points, for the end-to-end, determinism and capture tests: (inputs, restatement's projection)."""
    rs = np.random.RandomState(21)
    counts, S, size = (400, 0, 250, 150), 8, (128, 192)
    cam1, cam2, lags = sweeps(rs, S)
    pts, sw = sensor_points(rs, sum(counts), 0, S)
    K = np.array([[150.0, 0, 96.3], [0, 153.0, 61.7], [0, 0, 1.0]])
    off = offsets_of(counts)
    proj = ref.project(pts, sw, off, cam1, cam2, lags, K, size, 1.0, 2.0)
    return dict(pts=pts, sw=sw, off=off, cam1=cam1, cam2=cam2, lags=lags, K=K, size=size, s=2, cut=4, proj=proj)


@pytest.fixture(scope="module")
def small_case():
    return make_small_case()


def front_end(radar, c, **kw):
    return radar.radar_inputs(cuda(c["pts"]), cuda(c["sw"]), cuda(c["off"]), cuda(c["cam1"]), cuda(c["cam2"]), cuda(c["lags"]), cuda(c["K"]),
                              c["size"], 1.0, 2.0, c["s"], c["cut"], **kw)


def test_end_to_end_into_assemble_batch(radar, small_case):
    from camradepth_amd.batch import assemble_batch
    c = small_case
    proj, s, (h, w) = c["proj"], c["s"], c["size"]
    h_new, w_new = h // s, w // s
    ok = proj["valid"] == 1
    assert ok.sum() >= 60
    # on the restatement: no scaled coordinate within 1e-6 of a rounding boundary, no two points of a pixel at one depth
    for k, hi in (("x1", w_new - 1), ("y1", h_new - 1)):
        a = ref.scaled(proj[k][ok], s, hi)
        assert np.abs(np.abs(a - np.floor(a)) - 0.5).min() >= 1e-6
    pix = {}
    for i in np.nonzero(ok)[0]:
        key = (np.searchsorted(c["off"], i, side="right"), int(round(ref.scaled(proj["y1"][i], s, h_new - 1))),
               int(round(ref.scaled(proj["x1"][i], s, w_new - 1))))
        pix.setdefault(key, []).append(proj["depth1"][i])
    assert all(len(set(v)) == len(v) for v in pix.values()) and any(len(v) > 1 for v in pix.values())
    want_radar, want_vel = ref.rasterize(proj, c["off"], c["K"], c["size"], s, c["cut"])
    B, H, W = want_vel.shape
    rs = np.random.RandomState(3)
    img = cuda(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8))
    gt = cuda(rs.uniform(0, 90, size=(B, H, W)).astype(np.float32))
    maps = front_end(radar, c)
    got = assemble_batch(img, maps["radar"], maps["rad_vel"], gt)["image"].cpu().numpy()
    want = assemble_batch(img, cuda(want_radar), cuda(want_vel), gt)["image"].cpu().numpy()
    assert got.shape == (B, 7, H, W)
    assert np.array_equal(got[:, :3], want[:, :3])
    assert np.array_equal(got[:, 3], want[:, 3]) and np.array_equal(got[:, 6], want[:, 6])
    assert np.array_equal(maps["radar"][..., 0].cpu().numpy() != 0, want_radar[..., 0] != 0) and (want_radar[..., 0] != 0).sum() >= 50
    # u, v: a 1e-8 wobble of the projection can flip the fp32 rounding of xm (one ulp of w_new, divided by fx / s); then the cast of the value
    f = c["K"][0, 0] / s
    for ch in (4, 5):
        bound = float(np.spacing(np.float32(w_new))) / f + np.spacing(np.abs(want[:, ch]))
        err = np.abs(got[:, ch].astype(np.float64) - want[:, ch].astype(np.float64))
        print(f"channel {ch}: max |error| {err.max():.3e}, bound at least {float(np.spacing(np.float32(w_new))) / f:.3e}")
        assert (err <= bound).all(), (ch, err.max())


def test_two_runs_give_identical_bits(radar, small_case):
    a, b = front_end(radar, small_case), front_end(radar, small_case)
    torch.cuda.synchronize()
    for k in ("radar", "rad_vel"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert a["radar"].data_ptr() != b["radar"].data_ptr() and (a["radar"][..., 0] != 0).sum() >= 50


def test_capture_in_a_graph_and_replay_with_other_points(radar, small_case):
    """With a workspace and out= the front end is kernel launches only (the key images are reset by a fill kernel, not a memset node):
    captured once on one stream, replayed for two sets of points, the second with fewer points than the buffers hold."""
    c = small_case
    n, B = len(c["pts"]), len(c["off"]) - 1
    rs = np.random.RandomState(33)
    other = dict(c)
    m = n - 40                                              # the second set has fewer points: the tail of the buffers belongs to no frame
    pts2, sw2 = sensor_points(rs, m, 0, len(c["lags"]))
    other.update(pts=pts2, sw=sw2, off=offsets_of((170, 300, 0, m - 470)))
    other["cam1"], other["cam2"], other["lags"] = sweeps(rs, len(c["lags"]))
    eager = [front_end(radar, c), front_end(radar, other)]
    assert not torch.equal(eager[0]["radar"], eager[1]["radar"])
    keys = ("pts", "sw", "off", "cam1", "cam2", "lags", "K")
    bufs = {k: cuda(c[k]) for k in keys}
    ws = radar.RadarWorkspace(B, c["size"], c["s"], max_points=n)
    h, w = radar.map_shape(c["size"], c["s"], c["cut"])
    out = {"radar": torch.empty(B, h, w, 3, device="cuda"), "rad_vel": torch.empty(B, h, w, device="cuda")}

    def call():
        return radar.radar_inputs(bufs["pts"], bufs["sw"], bufs["off"], bufs["cam1"], bufs["cam2"], bufs["lags"], bufs["K"], c["size"], 1.0,
                                  2.0, c["s"], c["cut"], workspace=ws, out=out)

    res = call()                                            # eager once: the code objects are loaded before the capture
    assert res["radar"].data_ptr() == out["radar"].data_ptr() and res["rad_vel"].data_ptr() == out["rad_vel"].data_ptr()
    assert_equal(out["radar"], eager[0]["radar"], "radar, workspace and out=")
    torch.cuda.synchronize()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count          # with a workspace and out= a call allocates nothing
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for which in (1, 0):
        src = (c, other)[which]
        for k in keys:
            new = cuda(src[k])
            bufs[k].fill_(float("nan") if bufs[k].dtype == torch.float64 else 0)
            bufs[k][:len(new)].copy_(new)
        out["radar"].fill_(-1.0), out["rad_vel"].fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert_equal(out["radar"], eager[which]["radar"], f"radar, replay of set {which}")
        assert_equal(out["rad_vel"], eager[which]["rad_vel"], f"rad_vel, replay of set {which}")


def test_host_tensors_wrong_dtypes_and_shapes_are_refused(radar, small_case):
    from camradepth_amd import lib as L
    c = small_case
    args = [cuda(c[k]) for k in ("pts", "sw", "off", "cam1", "cam2", "lags", "K")]

    def refused(i, bad, fn=radar.project_radar):
        a = list(args)
        a[i] = bad
        with pytest.raises(L.CrdError):
            fn(*a, c["size"])

    for i in range(7):
        refused(i, args[i].cpu())                                            # not on the GPU
        refused(i, args[i].cpu(), radar.radar_inputs)
    refused(0, args[0].float()), refused(1, args[1].long()), refused(2, args[2].long()), refused(3, args[3].float())
    refused(5, args[5].float()), refused(6, args[6].float())                 # wrong dtypes
    refused(0, args[0][:, :4].contiguous()), refused(1, args[1][:-1]), refused(4, args[4][:-1]), refused(5, args[5][:, :1].contiguous())
    refused(6, args[6].expand(3, 3, 3).contiguous())                         # K for 3 frames, 4 given
    refused(0, args[0].t().contiguous().t())                                 # not contiguous
    proj = radar.project_radar(*args, c["size"])
    off, K = args[2], args[6]
    for k in proj:
        with pytest.raises(L.CrdError):
            radar.rasterize_radar(dict(proj, **{k: proj[k].cpu()}), off, K, c["size"], c["s"], c["cut"])
        with pytest.raises(L.CrdError):
            radar.rasterize_radar(dict(proj, **{k: proj[k].float()}), off, K, c["size"], c["s"], c["cut"])
        with pytest.raises(L.CrdError):
            radar.rasterize_radar(dict(proj, **{k: proj[k][:-1]}), off, K, c["size"], c["s"], c["cut"])
    with pytest.raises(L.CrdError):
        radar.rasterize_radar({k: v for k, v in proj.items() if k != "x2"}, off, K, c["size"], c["s"], c["cut"])
    with pytest.raises(L.CrdError):
        radar.rasterize_radar(proj, off, K, c["size"], 0, c["cut"])
    with pytest.raises(L.CrdError):
        radar.rasterize_radar(proj, off, K, c["size"], c["s"], 64)
    with pytest.raises(L.CrdError):                                          # a workspace for fewer frames
        radar.rasterize_radar(proj, off, K, c["size"], c["s"], c["cut"], workspace=radar.RadarWorkspace(1, c["size"], c["s"]))
    with pytest.raises(L.CrdError):
        radar.rasterize_radar(proj, off, K, c["size"], c["s"], c["cut"], out={"radar": torch.empty(4, 60, 96, 3, device="cuda"),
                                                                               "rad_vel": torch.empty(4, 60, 95, device="cuda")})
    with pytest.raises(L.CrdError):
        radar.RadarWorkspace(4, c["size"], c["s"], max_points=10).proj_out(11)
