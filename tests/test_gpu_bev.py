"""GPU: camradepth_amd.bev -- point clouds to bird's-eye-view grids -- against tests/bev_ref.py, the NumPy restatement of
include/camradepth_hip.h (itself checked against a per-point loop in tests/test_bev_ref_cpu.py).  Everything is compared bit for bit:
torch.equal, floats as their int32 views (an empty cell is a NaN)."""
import numpy as np
import pytest
import torch

from tests import bev_cases, bev_ref

pytestmark = pytest.mark.gpu

CASES = bev_cases.all_cases()
_WANT = {}
SENTINEL = 7


def cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def want_of(name):
    """The restatement's grids of case `name`, computed once."""
    if name not in _WANT:
        _WANT[name] = bev_ref.bev_grid(**whole_frames(CASES[name]))
    return _WANT[name]


def whole_frames(case):
    """An organised case cut to B whole frames: the Python interface takes [B,h,w,3], which has no rows beyond the last frame."""
    if case.get("frame_offsets") is not None:
        return case
    n = case["B"] * case["rows_per_frame"]
    return dict(case, xyz=case["xyz"][:n], valid=case["valid"][:n], label=case["label"][:n])


def assert_grids(got, want, what):
    """got: tensors, want: arrays or tensors."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in sorted(got):
        a, b = got[k], want[k]
        b = b if torch.is_tensor(b) else cuda(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == torch.float32:
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} cells, first at {(a != b).nonzero()[:3].tolist()}"


def options(case):
    return dict(x_range=(case["x_min"], case["x_min"] + case["nx"] * case["cell"]), y_range=(case["y_min"], case["y_min"] + case["ny"] * case["cell"]),
                cell=case["cell"], z_range=(case["z_lo"], case["z_hi"]), min_points=case["min_points"], flip=(case["flip_x"], case["flip_y"]),
                grid_from_points=cuda(case["T"]))


def run(case, **kw):
    """bev.bev_grid on a case of tests/bev_cases.py, through the input form the case has."""
    from camradepth_amd import bev
    case = whole_frames(case)
    if case.get("frame_offsets") is not None:
        return bev.bev_grid(cuda(case["xyz"]), cuda(case["frame_offsets"]), valid=cuda(case["valid"]), labels=cuda(case["label"]),
                            **options(case), **kw)
    B, rows = case["B"], case["rows_per_frame"]
    organised = {"points": cuda(case["xyz"]).view(B, 1, rows, 3), "valid": cuda(case["valid"]).view(B, 1, rows)}
    return bev.bev_grid(organised, labels=cuda(case["label"]).view(B, 1, rows), **options(case), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    got = run(CASES[name])
    assert got["count"].shape == (CASES[name]["B"], CASES[name]["nx"], CASES[name]["ny"])
    assert_grids(got, want_of(name), name)


def test_rows_beyond_the_last_frame_of_an_organised_cloud():
    """rows_per_frame with more rows than B frames hold: the C entry ignores the rest (the Python interface cannot say this)."""
    from camradepth_amd import bev
    from camradepth_amd import lib as L
    name = "B 3, 5 x 7, organised"
    case = CASES[name]
    n, B, nx, ny = len(case["xyz"]), case["B"], case["nx"], case["ny"]
    assert n > B * case["rows_per_frame"]
    xyz, valid, label = cuda(case["xyz"]), cuda(case["valid"]), cuda(case["label"])
    ws = bev.BevWorkspace(B, nx, ny)
    out = ws.outputs(label=True)
    L.check(L.load().crd_bev_grid(L.ptr(xyz), L.ptr(valid), L.ptr(label), None, case["rows_per_frame"], B, n, None, 0, L.f64_bits(case["x_min"]),
                                  L.f64_bits(case["y_min"]), L.f64_bits(case["cell"]), nx, ny, L.f64_bits(case["z_lo"]), L.f64_bits(case["z_hi"]),
                                  case["min_points"], int(case["flip_x"]), int(case["flip_y"]), L.ptr(ws.keys), ws.keys.numel(),
                                  L.ptr(out["count"]), L.ptr(out["z_max"]), L.ptr(out["z_min"]), L.ptr(out["top_index"]), L.ptr(out["top_label"]),
                                  L.ptr(out["occupancy"]), L.stream()), "crd_bev_grid")
    assert_grids(out, bev_ref.bev_grid(**case), name)
    assert_grids(out, want_of(name), name + ", cut to whole frames")


@pytest.mark.parametrize("cells", [2, 1], ids=["2 x 2", "one cell"])
def test_contention(cells):
    """4,096 rows into four cells or one: every add arrives, and among the many rows at the largest height the lowest index wins."""
    rs = np.random.RandomState(60 + cells)
    n = 4096
    xyz = np.stack([rs.uniform(0.0, 1.0, n), rs.uniform(0.0, 1.0, n), np.round(rs.uniform(-3, 3, n) * 2) / 2], axis=1).astype(np.float32)
    cell = 1.0 / cells
    case = dict(xyz=xyz, B=1, x_min=0.0, y_min=0.0, cell=cell, nx=cells, ny=cells, frame_offsets=np.array([0, n], dtype=np.int32), valid=None,
                label=None, T=None, z_lo=-bev_cases.INF, z_hi=bev_cases.INF, min_points=1, flip_x=False, flip_y=False)
    got = run(case)
    assert_grids(got, bev_ref.bev_grid(**case), f"{cells} x {cells}")
    assert int(got["count"].sum()) == n and (got["z_max"] == 3.0).all() and (got["z_min"] == -3.0).all()
    ix, iy = np.floor(xyz[:, 0].astype(np.float64) / cell).astype(int), np.floor(xyz[:, 1].astype(np.float64) / cell).astype(int)
    for i in range(cells):
        for j in range(cells):
            here = (ix == i) & (iy == j)
            assert int(got["count"][0, i, j]) == here.sum() and (here & (xyz[:, 2] == 3.0)).sum() > 20
            assert int(got["top_index"][0, i, j]) == np.nonzero(here & (xyz[:, 2] == 3.0))[0][0]


def test_two_runs_stale_state_and_no_rows():
    """Two calls give the same bits; a call into a used workspace and used outputs shows nothing of the call before (the clear pass);
    a cloud without rows gives the empty grid."""
    from camradepth_amd import bev
    first, second = "B 3, 16 x 12, transform per frame", "B 3, 16 x 12, transform None"
    a, b = run(CASES[first]), run(CASES[first])
    torch.cuda.synchronize()
    assert a["count"].data_ptr() != b["count"].data_ptr()
    assert_grids(a, b, "second run")
    ws = bev.BevWorkspace(3, 16, 12)
    out = ws.outputs(label=True)
    assert set(ws.out) == {"count", "z_max", "z_min", "top_index", "occupancy"} and ws.keys.numel() == bev_ref.workspace_bytes(3, 16, 12)
    for name in (first, second, first):
        res = run(CASES[name], workspace=ws, out=out)
        assert all(res[k].data_ptr() == out[k].data_ptr() for k in out)
        assert_grids(out, want_of(name), f"{name} into a used workspace")
    case = dict(CASES[second], xyz=np.zeros((0, 3), np.float32), valid=None, label=None, frame_offsets=np.zeros(4, np.int32))
    empty = run(case, workspace=ws, out=ws.out)
    assert_grids(empty, bev_ref.bev_grid(**case), "no rows")
    assert int(empty["count"].sum()) == 0 and (empty["z_max"].view(torch.int32) == 0x7fc00000).all() and (empty["top_index"] == -1).all()
    assert (empty["z_min"].view(torch.int32) == 0x7fc00000).all() and int(empty["occupancy"].sum()) == 0


def synthetic_depth(rs, B, h, w):
    """Normalised inverse depth of a road scene: the ground plane 1.6 m under the camera in the lower half, walls at 8 .. 40 m above."""
    rows = np.arange(h, dtype=np.float64)[None, :, None] + np.zeros((B, h, w))
    ground = 1.6 * 30.0 / np.maximum(rows - h / 2 + 0.5, 0.5)                  # fy = 30 at map resolution
    wall = 8.0 + 32.0 * rs.uniform(size=(B, 1, w // 8)).repeat(8, axis=2) + np.zeros((B, h, w))
    metres = np.minimum(np.where(rows >= h / 2, ground, 1e9), wall)
    p = (1.0 - metres / 100.0).astype(np.float32)
    p[rs.uniform(size=p.shape) < 0.02] = np.nan
    return p


def test_through_the_real_producers():
    """point_cloud with labels -> bev_grid equals the restatement on the same cloud; unproject_depth -> bev_grid equals the compact path
    wherever both are defined (the rows are numbered differently, so not top_index)."""
    from camradepth_amd import bev, cloud
    rs = np.random.RandomState(70)
    B, h, w = 2, 32, 64
    size, s, cut = (64, 128), 2, 0
    depth = cuda(synthetic_depth(rs, B, h, w))
    labels = cuda(rs.randint(0, 19, size=(B, h, w)).astype(np.uint8))
    K = cuda(np.array([[60.0, 0, 63.5], [0, 60.0, 31.5], [0, 0, 1.0]]))
    T = bev.CAM_TO_BEV.cuda()
    kw = dict(x_range=(0, 40), y_range=(-20, 20), cell=0.5, z_range=(-3.0, 3.0), min_points=2)
    compact = cloud.point_cloud(depth, K, size, s, cut, labels=labels, keep=range(256))
    got = bev.bev_grid(compact, grid_from_points=T, **kw)
    n = int(compact["frame_offsets"][-1])
    assert n > 3000 and set(got) == {"count", "z_max", "z_min", "top_index", "occupancy", "top_label"}
    want = bev_ref.bev_grid(compact["xyz"].cpu().numpy(), B, 0.0, -20.0, 0.5, 80, 80, frame_offsets=compact["frame_offsets"].cpu().numpy(),
                            label=compact["label"].cpu().numpy(), T=bev.CAM_TO_BEV.numpy(), z_lo=-3.0, z_hi=3.0, min_points=2)
    assert_grids(got, want, "compact cloud")
    assert 100 < int((got["count"] > 0).sum()) and int(got["count"].max()) >= 8 and 0 < int(got["occupancy"].sum()) < int((got["count"] > 0).sum())
    assert int(got["count"].sum()) < n                                         # some points lie above the band or outside the grid
    organised = cloud.unproject_depth(depth, K, size, s, cut, labels=labels, keep=range(256))
    same = bev.bev_grid(organised, grid_from_points=T, labels=labels, **kw)
    for k in ("count", "z_max", "z_min", "occupancy", "top_label"):            # both number their rows in (b, r, c) order: the same point wins
        assert_grids({k: same[k]}, {k: got[k]}, "organised cloud")
    some = got["count"] > 0
    assert torch.equal(organised["points"].view(-1, 3)[same["top_index"][some].long()], compact["xyz"][got["top_index"][some].long()])


def test_capture_on_a_side_stream():
    """bev_grid with a workspace, captured once; new rows and new offsets in the same buffers, replayed: the eager result."""
    from camradepth_amd import bev
    names = ("B 3, 5 x 7, transform shared", "B 3, 5 x 7, transform None", "B 3, 5 x 7, transform per frame")
    cases = {}
    for name in names:                                                         # one grid and one transform layout for all three
        cases[name] = dict(CASES[name], T=CASES[names[2]]["T"], x_min=-3.0, y_min=-3.0, cell=6.0 / 7, flip_x=True, flip_y=False)
    want = {k: bev_ref.bev_grid(**v) for k, v in cases.items()}
    first = cases[names[0]]
    n = len(first["xyz"])
    xyz, off, valid, label = cuda(first["xyz"]), cuda(first["frame_offsets"]), cuda(first["valid"]), cuda(first["label"])
    opts = options(first)
    ws = bev.BevWorkspace(3, 5, 7)
    out = ws.outputs(label=True)

    def call():
        return bev.bev_grid(xyz, off, valid=valid, labels=label, workspace=ws, out=out, **opts)

    call()                                                                     # eager once: the code objects are loaded before the capture
    torch.cuda.synchronize()
    assert_grids(out, want[names[0]], "eager")
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream, four launches in a row
        call()
    for name in (names[1], names[2], names[0]):
        c = cases[name]
        assert len(c["xyz"]) == n
        xyz.copy_(cuda(c["xyz"])), off.copy_(cuda(c["frame_offsets"])), valid.copy_(cuda(c["valid"])), label.copy_(cuda(c["label"]))
        for k in out:
            out[k].fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_grids(out, want[name], f"replay: {name}")


def test_picture_is_colorize_of_the_height_map():
    from camradepth_amd import bev, viz
    grid = run(CASES["B 3, 16 x 12, transform None"])
    got = bev.picture(grid, (-4.0, 5.0))
    assert got.dtype == torch.uint8 and got.shape == (3, 16, 12, 3)
    assert torch.equal(got, viz.colorize(grid["z_max"], "jet", vmin=-4.0, vmax=5.0))
    empty = grid["count"] == 0
    assert 0 < int(empty.sum()) < empty.numel()
    assert (got[empty] == 0).all() and (got[~empty].sum(dim=1) > 0).all()       # bad_colour is black; jet has no black row
    canvas = torch.full((3, 16, 12, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    assert bev.picture(grid, (-4.0, 5.0), cmap="rainbow", out=canvas).data_ptr() == canvas.data_ptr()
    assert torch.equal(canvas, viz.colorize(grid["z_max"], "rainbow", vmin=-4.0, vmax=5.0)) and not torch.equal(canvas, got)


def test_live_pipeline_with_a_grid():
    """LivePipeline(cloud=, bev=): run()['bev'] has the bits of bev_grid on the cloud of the stages called one by one, for two sensor
    sets in a row (the second replay, another number of points, a pose); everything else equals a pipeline built without bev=."""
    from camradepth_amd import bev, viz
    from camradepth_amd import lib as L
    from camradepth_amd.inference import InferenceGraph
    from camradepth_amd.live import LivePipeline
    from tests.test_gpu_live import (B, CLOUD, CUT, H, N_SWEEPS, S, SETS, SIZE, W, assert_same, flat, sensor_set, small_model, stagewise)
    model = small_model()
    # every point within max_depth lies inside 128 m of the origin of any of the poses
    grid_opts = dict(x_range=(-128, 128), y_range=(-64, 128), cell=2.0, min_points=2, flip=(False, True))
    with pytest.raises(L.CrdError, match="cloud"):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, bev=grid_opts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={},
                        bev=dict(grid_opts, picture=True, picture_z_range=(-128.0, 128.0)))
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={})
    ig, vz = InferenceGraph(model, B, H, W), viz.Visualizer(B, H, W)
    views, counts = [], []
    for seed, n_points, pose in SETS:
        c = sensor_set(seed, n_points, pose)
        res = live.run(**c)
        assert set(res) == {"image", "x", "radar", "rad_vel", "pred", "cloud", "bev", "pictures"}
        assert set(res["bev"]) == {"count", "z_max", "z_min", "top_index", "occupancy", "picture"}
        views.append({k: v.data_ptr() for k, v in res["bev"].items()})
        got_bev = {k: v.clone() for k, v in res["bev"].items()}
        got = {k: v.clone() for k, v in flat(res).items()}
        torch.cuda.synchronize()
        assert_same(got, {k: v.clone() for k, v in flat(plain.run(**c)).items()}, f"set {seed}: with and without bev=")
        stages = stagewise(model, ig, vz, c)
        want = bev.bev_grid(stages["cloud"], **grid_opts)
        want["picture"] = bev.picture(want, (-128.0, 128.0))
        assert_grids(got_bev, want, f"set {seed}")
        assert want["count"].shape == (B, 128, 96) and int(want["count"].sum()) > 100 and int(want["occupancy"].sum()) > 0
        counts.append(want["count"].clone())
    assert views[0] == views[1] and not torch.equal(counts[0], counts[1])
    copies = live.run(clone=True, **c)["bev"]
    assert all(copies[k].data_ptr() != p for k, p in views[0].items())
    assert_grids(copies, got_bev, "clone=True")
