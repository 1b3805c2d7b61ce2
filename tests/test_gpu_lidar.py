"""GPU: the lidar ground-truth front end (camradepth_amd.lidar: project_lidar, lidar_ground_truth, lidar_gt, LidarWorkspace) against
the fixture the reference's own ground-truth stage produced (tests/golden/lidar_gt.npz) and against the NumPy restatement in
tests/lidar_ref.py.

The ground-truth stage is additions, divisions, clips, a round-half-even, one square root and roundings to fp32 -- all correctly
rounded on both sides and never contracted -- so it is compared bit for bit.  The projection is compared within 1e-8 absolute, in
pixels and metres, the bound tests/test_gpu_radar.py derives for the same arithmetic (the box-frame transform adds one 3 x 4 product of
the same size; test_lidar_ref_cpu.py checks that no coordinate of the case exceeds 1e6 and that every compared quantity is 1e-6 away
from its threshold, so the flags are compared exactly)."""
import numpy as np
import pytest
import torch

from tests import lidar_cases as cases
from tests import lidar_ref as ref

pytestmark = pytest.mark.gpu

PROJECT_BOUND = 1e-8


@pytest.fixture(scope="module")
def lidar():
    from camradepth_amd import lidar as module
    return module


def cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def dev_proj(proj):
    d = {k: cuda(proj[k], np.float64) for k in ref.PROJ_KEYS}
    d.update({k: cuda(proj[k], np.uint8) for k in ("low_h", "in_box")})
    if proj.get("valid") is not None:
        d["valid"] = cuda(proj["valid"], np.uint8)
    return d


def dev_filters(f):
    return {k: (v if isinstance(v, float) else cuda(v)) for k, v in f.items()}


def run_gt(lidar, proj, off, K, size, s, cut, filters, **kw):
    out = lidar.lidar_ground_truth(dev_proj(proj), cuda(off), cuda(K, np.float64), size, s, cut, **dev_filters(filters), **kw)
    torch.cuda.synchronize()
    return out


def assert_equal(got, want, what):
    want = torch.from_numpy(want) if isinstance(want, np.ndarray) else want
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} values differ; first at {i}: {got[i].item()!r} against {want[i].item()!r}")


def assert_maps(got, want, what):
    gt, depth, msk = want
    assert_equal(got["gt"], gt, what + ": gt")
    assert_equal(got["depth"], depth, what + ": depth")
    assert_equal(got["msk_lh"], msk, what + ": msk_lh")
    assert got["depth"].is_contiguous()


@pytest.mark.parametrize("stage", ["raster", "box", "flow"])
def test_fixture_of_the_reference_after_every_stage(lidar, golden_dir, stage):
    c = cases.load_fixture(golden_dir)
    got = run_gt(lidar, c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"], c["stages"][stage])
    h, w = c["shape"]
    e = c["f"]["entries_" + stage]
    gt, msk = np.zeros((1, h, w, 3), dtype=np.float32), np.zeros((1, h, w), dtype=np.uint8)
    r, col = e[:, 0].astype(int), e[:, 1].astype(int)
    gt[0, r, col] = e[:, 2:5].astype(np.float32)
    msk[0, r, col] = e[:, 5].astype(np.uint8)
    assert_maps(got, (gt, np.ascontiguousarray(gt[..., 0]), msk), stage)


@pytest.mark.parametrize("name", list(cases.RAGGED))
def test_ragged_batches_against_the_restatement(lidar, name):
    c = cases.ragged_case(name)
    box_only = {k: c["filters"][k] for k in ("seg", "corners", "corner_offsets")}
    nomask = {k: v for k, v in c["proj"].items() if k != "valid"}
    for what, proj, filt in (("both filters", c["proj"], c["filters"]), ("no filter", c["proj"], {}), ("box filter", c["proj"], box_only),
                             ("flow filter", c["proj"], {k: c["filters"][k] for k in ("flow_im", "thres")}),
                             ("no mask", nomask, c["filters"])):
        want = ref.ground_truth(proj, c["off"], c["K"], c["size"], c["s"], c["cut"], **filt)
        assert_maps(run_gt(lidar, proj, c["off"], c["K"], c["size"], c["s"], c["cut"], filt), want, f"{name}, {what}")


@pytest.fixture(scope="module")
def projection_case():
    c = cases.projection_case()
    return c, cases.project_ref(c)


def project(lidar, c, **kw):
    box = {k: cuda(c[v]) for k, v in (("sweep_boxes", "sweep_boxes"), ("box_entries", "entries"), ("box_id", "box_id"),
                                      ("cam1_from_box", "cam1_box"), ("cam2_from_box", "cam2_box"), ("vehicle", "vehicle")) if v in c}
    out = lidar.project_lidar(cuda(c["pts"]), cuda(c["sw"]), cuda(c["off"]), cuda(c["cam1"]), cuda(c["cam2"]), cuda(c["car_z"]), cuda(c["K"]),
                              image_size=c["size"], **box, **kw)
    torch.cuda.synchronize()
    return out


def assert_projection(got, want, n, what):
    assert set(got) == set(ref.PROJ_KEYS) | set(ref.FLAG_KEYS) | {"box_entry"}
    for k in ref.FLAG_KEYS:
        assert_equal(got[k], want[k], f"{what}: {k}")
    assert_equal(got["box_entry"], want["box_entry"], f"{what}: box_entry")
    for k in ref.PROJ_KEYS:
        assert got[k].dtype == torch.float64 and got[k].shape == (n,)
        err = np.abs(got[k].cpu().numpy() - want[k])
        print(f"project_lidar {what} {k}: max |error| {err.max():.3e}")
        assert err.max() <= PROJECT_BOUND, (what, k, err.max(), int(err.argmax()))


def test_projection_against_the_restatement(lidar, projection_case):
    c, want = projection_case
    n_in = int(c["off"][-1])
    assert want["margin"][:n_in].min() >= 1e-6                       # test_lidar_ref_cpu.py shows how the case meets it
    assert_projection(project(lidar, c), want, len(c["pts"]), "defaults")
    kw = dict(min_distance=1.0, min_z=10.0, h_min=-0.5, h_max=1.0)
    other = cases.project_ref(c, **kw)
    assert other["margin"][:n_in].min() >= 1e-6
    assert_projection(project(lidar, c, **kw), other, len(c["pts"]), "other thresholds")
    # one K for all frames, no box tables: every point goes through its sweep's matrices
    plain = {k: v for k, v in c.items() if k not in ("sweep_boxes", "entries", "box_id", "cam1_box", "cam2_box", "vehicle")}
    plain["K"] = c["K"][1]
    want_plain = cases.project_ref(plain)
    assert want_plain["margin"][:n_in].min() >= 1e-6 and not want_plain["in_box"].any()
    assert_projection(project(lidar, plain), want_plain, len(c["pts"]), "no boxes")


def test_exact_boundaries(lidar):
    c, expected = cases.boundary_case()
    got = project(lidar, c)
    want = cases.project_ref(c)
    for j, (what, valid, low, in_box, entry) in enumerate(expected):
        flags = tuple(int(got[k][j]) for k in ("valid", "low_h", "in_box", "box_entry"))
        assert flags == (valid, low, in_box, entry), (what, flags)
    for k in ref.PROJ_KEYS:                                          # exact arithmetic on both sides
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


def test_nan_unknown_sweeps_and_unknown_boxes_are_invalid(lidar):
    c, _ = cases.boundary_case()
    c["pts"] = np.tile(np.array([[16.5, 3.25, 0.25]]), (8, 1))
    for i in range(3):
        c["pts"][i, i] = np.nan
    c["sw"] = np.array([0, 0, 0, 0, 1, -1, 0, 0], dtype=np.int32)     # rows 4, 5: a sweep outside the tables
    c["off"] = cases.offsets_of([7])                                 # row 7: outside every frame
    want = cases.project_ref(c)
    assert list(want["valid"]) == [0, 0, 0, 1, 0, 0, 1, 0] and list(want["box_entry"]) == [-1, -1, -1, 0, -1, -1, 0, -1]
    got = project(lidar, c)
    for k in ref.FLAG_KEYS + ("box_entry",):
        assert_equal(got[k], want[k], k)
    for k in ref.PROJ_KEYS:
        assert np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), k
    c["box_id"] = np.array([1], dtype=np.int32)                       # the entry names a box the tables do not hold
    got = project(lidar, c)
    assert int(got["valid"].sum()) == 0                                # rows 3 and 6 lie in that box: invalid, zeros
    assert_equal(got["box_entry"], np.full(8, -1, dtype=np.int32), "box_entry, unknown box")
    assert not got["x1"][3:].any() and not got["depth1"][3:].any()


@pytest.fixture(scope="module")
def small_case():
    """4 frames at 128 x 192 from sensor points with boxes, for the end-to-end, determinism and capture tests."""
    c = cases.projection_case()
    rs = np.random.RandomState(21)
    c["size"] = (128, 192)
    c["K"] = np.array([[150.0, 0, 96.3], [0, 153.0, 61.7], [0, 0, 1.0]])
    c["off"] = cases.offsets_of((500, 0, 700, 800))
    c["s"], c["cut"] = 2, 4
    c["filters"] = cases.filters_for(rs, 4, 128, 192, 2, 4, (2, 1, 0, 3), np.array([10.0, 20.0]))
    return c


def front_end(lidar, c, **kw):
    box = {k: cuda(c[v]) for k, v in (("sweep_boxes", "sweep_boxes"), ("box_entries", "entries"), ("box_id", "box_id"),
                                      ("cam1_from_box", "cam1_box"), ("cam2_from_box", "cam2_box"), ("vehicle", "vehicle"))}
    return lidar.lidar_gt(cuda(c["pts"]), cuda(c["sw"]), cuda(c["off"]), cuda(c["cam1"]), cuda(c["cam2"]), cuda(c["car_z"]), cuda(c["K"]),
                          image_size=c["size"], downsample_scale=c["s"], y_cutoff=c["cut"], **box, **dev_filters(c["filters"]), **kw)


def test_hand_off_into_assemble_batch(lidar, small_case):
    from camradepth_amd.batch import assemble_batch
    c = small_case
    proj = project(lidar, c)                                         # the device's own projection: the maps are then compared bit for bit
    host = {k: v.cpu().numpy() for k, v in proj.items()}
    want_gt, want_depth, want_msk = ref.ground_truth(host, c["off"], c["K"], c["size"], c["s"], c["cut"], **c["filters"])
    maps = front_end(lidar, c)
    assert_maps(maps, (want_gt, want_depth, want_msk), "lidar_gt")
    B, H, W = want_depth.shape
    assert (want_depth != 0).sum() >= 50 and want_msk.any()
    rs = np.random.RandomState(3)
    img = cuda(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8))
    radar, vel = cuda(rs.uniform(0, 60, size=(B, H, W, 3)).astype(np.float32)), cuda(rs.uniform(size=(B, H, W)).astype(np.float32))
    got = assemble_batch(img, radar, vel, maps["depth"])
    want = assemble_batch(img, radar, vel, cuda(want_depth))
    assert_equal(got["gt_full"], want["gt_full"], "gt_full")
    assert (got["gt_full"] != 0).sum() >= 50


def test_order_independence_and_two_runs(lidar):
    c = cases.ragged_case("ragged")
    proj, off = c["proj"], c["off"]
    rs = np.random.RandomState(8)
    perm = np.arange(len(proj["x1"]))
    with np.errstate(invalid="ignore"):
        for b in range(c["B"]):                                      # within a frame: any order that keeps equal depths in their order
            lo, hi = off[b], off[b + 1]
            p = lo + rs.permutation(hi - lo)
            d = proj["depth1"][p]
            for v in np.unique(d[np.isfinite(d)]):
                slots = np.nonzero(d == v)[0]
                p[slots] = np.sort(p[slots])
            perm[lo:hi] = p
    assert (perm != np.arange(len(perm))).sum() >= 300
    shuffled = {k: np.asarray(v)[perm] for k, v in proj.items()}
    args = (off, c["K"], c["size"], c["s"], c["cut"], c["filters"])
    a, b, s = run_gt(lidar, proj, *args), run_gt(lidar, proj, *args), run_gt(lidar, shuffled, *args)
    for k in ("gt", "depth", "msk_lh"):
        bits = (lambda t: t.view(torch.int32)) if k != "msk_lh" else (lambda t: t)
        assert torch.equal(bits(a[k]), bits(b[k])), k
        assert torch.equal(bits(a[k]), bits(s[k])), k + ", points in another order"
    assert a["gt"].data_ptr() != b["gt"].data_ptr() and (a["depth"] != 0).sum() >= 50


def test_workspace_capture_and_replay_with_fewer_points(lidar, small_case):
    """With a workspace and out= the front end is kernel launches only: captured once on one stream, replayed with the same points and
    with a frame_offsets that ends 60 points earlier; both give the eager result."""
    c = small_case
    n, B = len(c["pts"]), len(c["off"]) - 1
    short = dict(c, off=cases.offsets_of((400, 300, 0, n - 30 - 60 - 700)))
    assert short["off"][-1] == c["off"][-1] - 60
    eager = [front_end(lidar, c), front_end(lidar, short)]
    assert not torch.equal(eager[0]["gt"], eager[1]["gt"])
    keys = ("pts", "sw", "off", "cam1", "cam2", "car_z", "K", "sweep_boxes", "entries", "box_id", "cam1_box", "cam2_box", "vehicle")
    bufs = {k: cuda(c[k]) for k in keys}
    filt = dev_filters(c["filters"])
    ws = lidar.LidarWorkspace(B, c["size"], c["s"], max_points=n, max_boxes=len(c["filters"]["corners"]))
    h, w = lidar.map_shape(c["size"], c["s"], c["cut"])
    out = {"gt": torch.empty(B, h, w, 3, device="cuda"), "depth": torch.empty(B, h, w, device="cuda"),
           "msk_lh": torch.empty(B, h, w, dtype=torch.uint8, device="cuda")}

    def call():
        return lidar.lidar_gt(bufs["pts"], bufs["sw"], bufs["off"], bufs["cam1"], bufs["cam2"], bufs["car_z"], bufs["K"], bufs["sweep_boxes"],
                              bufs["entries"], bufs["box_id"], bufs["cam1_box"], bufs["cam2_box"], bufs["vehicle"], c["size"],
                              downsample_scale=c["s"], y_cutoff=c["cut"], workspace=ws, out=out, **filt)

    res = call()                                            # eager once: the code objects are loaded before the capture
    assert all(res[k].data_ptr() == out[k].data_ptr() for k in out)
    assert_equal(out["gt"], eager[0]["gt"], "gt, workspace and out=")
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for which in (1, 0):
        bufs["off"].copy_(cuda((c, short)[which]["off"]))
        for k in out:
            out[k].fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for k in out:
            assert_equal(out[k], eager[which][k], f"{k}, replay {which}")


def test_wrong_inputs_are_refused(lidar, small_case):
    from camradepth_amd import lib as L
    c = small_case
    names = ("pts", "sw", "off", "cam1", "cam2", "car_z", "K")
    args = [cuda(c[k]) for k in names]
    box = {k: cuda(c[v]) for k, v in (("sweep_boxes", "sweep_boxes"), ("box_entries", "entries"), ("box_id", "box_id"),
                                      ("cam1_from_box", "cam1_box"), ("cam2_from_box", "cam2_box"), ("vehicle", "vehicle"))}

    def refused(i, bad, fn=lidar.project_lidar, **kw):
        a = list(args)
        if i is not None:
            a[i] = bad
        with pytest.raises(L.CrdError):
            fn(*a, image_size=c["size"], **dict(box, **kw))

    for i in range(7):
        refused(i, args[i].cpu())                                            # not on the GPU
        refused(i, args[i].cpu(), lidar.lidar_gt)
    refused(0, args[0].float()), refused(1, args[1].long()), refused(2, args[2].long()), refused(3, args[3].float())
    refused(5, args[5].float()), refused(6, args[6].float())                 # wrong dtypes
    refused(0, args[0][:, :2].contiguous()), refused(1, args[1][:-1]), refused(4, args[4][:-1]), refused(5, args[5][:, :3].contiguous())
    refused(6, args[6].expand(3, 3, 3).contiguous())                         # K for 3 frames, 4 given
    refused(0, args[0].t().contiguous().t())                                 # not contiguous
    for k, bad in (("sweep_boxes", box["sweep_boxes"][:-1]), ("box_entries", box["box_entries"][:, :12].contiguous()),
                   ("box_id", box["box_id"].long()), ("cam2_from_box", box["cam2_from_box"][:-1]), ("vehicle", box["vehicle"].int()),
                   ("vehicle", None), ("box_id", box["box_id"].cpu())):
        refused(None, None, **{k: bad})
    proj = lidar.project_lidar(*args, image_size=c["size"], **box)
    off, K = args[2], args[6]
    filt = dev_filters(c["filters"])
    gt = lambda p, **kw: lidar.lidar_ground_truth(p, off, K, c["size"], c["s"], c["cut"], **kw)          # noqa: E731
    for k in proj:
        if k == "box_entry":
            continue
        for bad in (proj[k].cpu(), proj[k].float(), proj[k][:-1]):
            with pytest.raises(L.CrdError):
                gt(dict(proj, **{k: bad}))
    for kw in (dict(seg=filt["seg"]), dict(seg=filt["seg"], corners=filt["corners"]), dict(corners=filt["corners"]),
               dict(filt, seg=filt["seg"].float()), dict(filt, seg=filt["seg"][:, :-1].contiguous()), dict(filt, corners=filt["corners"][:, :7].contiguous()),
               dict(filt, corner_offsets=filt["corner_offsets"][:-1]), dict(filt, flow_im=filt["flow_im"].double()),
               dict(filt, flow_im=filt["flow_im"][..., :1].contiguous()), dict(filt, flow_im=filt["flow_im"].cpu())):
        with pytest.raises(L.CrdError):
            gt(proj, **kw)
    with pytest.raises(L.CrdError):
        gt({k: v for k, v in proj.items() if k != "low_h"})
    with pytest.raises(L.CrdError):
        lidar.lidar_ground_truth(proj, off, K, c["size"], 0, c["cut"])
    with pytest.raises(L.CrdError):
        lidar.lidar_ground_truth(proj, off, K, c["size"], c["s"], 64)
    with pytest.raises(L.CrdError):                                          # a workspace for fewer frames
        gt(proj, workspace=lidar.LidarWorkspace(1, c["size"], c["s"]))
    with pytest.raises(L.CrdError):                                          # a workspace without room for the boxes' rectangles
        tight = lidar.LidarWorkspace(4, c["size"], c["s"])
        tight.keys = tight.keys[:lidar.workspace_bytes(4 * 60 * 96)]
        gt(proj, workspace=tight, **filt)
    with pytest.raises(L.CrdError):
        gt(proj, out={"gt": torch.empty(4, 60, 96, 3, device="cuda"), "depth": torch.empty(4, 60, 95, device="cuda"),
                      "msk_lh": torch.empty(4, 60, 96, dtype=torch.uint8, device="cuda")})
    with pytest.raises(L.CrdError):
        lidar.LidarWorkspace(4, c["size"], c["s"], max_points=10).proj_out(11)


def test_project_corners_feeds_the_box_filter(lidar):
    """The corner table through project_lidar's code path: eight corners per box, in view or not as proj2im decides."""
    rs = np.random.RandomState(5)
    cam = np.stack([(cases.AXES @ cases.box_pose((12.0 + 9 * k, 6.0 - 4 * k, -0.3), 0.3 * k))[:3] for k in range(4)])
    size = np.array([[1.9, 4.6, 1.7], [2.6, 9.0, 3.1], [0.7, 0.8, 1.8], [2.0, 4.4, 1.6]])              # w, l, h
    K = np.array([[1266.4, 0, 816.3], [0, 1270.9, 491.5], [0, 0, 1.0]])
    off = cases.offsets_of((3, 1))
    got = lidar.project_corners(cuda(cam), cuda(size), cuda(off), cuda(K)).cpu().numpy()
    assert got.shape == (4, 8, 4)
    j = 0
    for k in range(4):
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    X = cam[k] @ np.array([sx * size[k, 1] / 2, sy * size[k, 0] / 2, sz * size[k, 2] / 2, 1.0])
                    px, py = (K[0, 0] * X[0] + K[0, 2] * X[2]) / X[2], (K[1, 1] * X[1] + K[1, 2] * X[2]) / X[2]
                    assert np.allclose(got[k, j % 8, :3], (px, py, X[2]), rtol=0, atol=1e-8), (k, j)
                    assert got[k, j % 8, 3] == float(X[2] >= 2 and 0 < px < 1600 and 0 < py < 900)
                    j += 1
    assert 0 < got[..., 3].sum() < 32


def test_contention(lidar):
    """200,000 points on a 64 x 96 map with depths from 16 values: the smallest shape at which the contended atomics and the tie pass do
    real work."""
    c = cases.contention_case()
    want = ref.ground_truth(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"], **c["filters"])
    plain = ref.ground_truth(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"])
    assert (plain[1] != 0).mean() > 0.99 and 50 <= (want[1] != 0).sum() < (plain[1] != 0).sum()
    assert_maps(run_gt(lidar, c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"], {}), plain, "contention, no filter")
    assert_maps(run_gt(lidar, c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"], c["filters"]), want, "contention")
