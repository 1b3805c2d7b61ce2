"""GPU: camradepth_amd.occupancy -- point clouds fused into a rolling occupancy map -- against tests/occupancy_ref.py, the NumPy
restatement of include/camradepth_hip.h (itself checked against plain loops and a world-cell dictionary in
tests/test_occupancy_ref_cpu.py).  Everything is compared bit for bit with torch.equal: the outputs of every call of a sequence, the
bins and the hit counts in the workspace, and the map's own state."""
import numpy as np
import pytest
import torch

from tests import occupancy_cases, occupancy_ref

pytestmark = pytest.mark.gpu

CASES = occupancy_cases.all_cases()
OUT = ("log_odds", "state", "evidence", "value", "origin")
_WANT = {}
SENTINEL = 7


def cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def want_of(name):
    """The restatement's results of every call of case `name` and its state at the end, computed once and left unchanged."""
    if name not in _WANT:
        case = CASES[name]
        state = occupancy_ref.new_state(case["params"])
        _WANT[name] = ([occupancy_ref.update(case["params"], state, B=case["B"], **f) for f in case["frames"]], state)
    return _WANT[name]


def new_map(params):
    from camradepth_amd import occupancy
    return occupancy.OccupancyMap(**params)


def feed(omap, case, frame, **kw):
    """occupancy.update with one frame of a case, through the input form the case has."""
    from camradepth_amd import occupancy
    B = case["B"]
    pose = dict(map_from_points=cuda(frame["T"]), sensor=cuda(frame["sensor"]), centre=cuda(frame["centre"]))
    xyz, valid = cuda(frame["xyz"]), cuda(frame.get("valid"))
    if case["form"] == "organised":
        rows = frame["rows_per_frame"]
        return occupancy.update(omap, {"points": xyz.view(B, 1, rows, 3), "valid": valid.view(B, 1, rows)}, **pose, **kw)
    if case["form"] == "bare":
        return occupancy.update(omap, xyz, cuda(frame["frame_offsets"]), valid=valid, **pose, **kw)
    return occupancy.update(omap, {"xyz": xyz, "frame_offsets": cuda(frame["frame_offsets"])}, valid=valid, **pose, **kw)


def assert_outputs(got, want, what):
    assert set(got) == set(OUT), (what, sorted(got))
    for k in OUT:
        a, b = got[k], cuda(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == torch.float32:
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def tables(ws, B, p):
    """hit_min, seen_max and hits as the last call left them in the workspace (the header's layout)."""
    def up(n):
        return (n + 15) & ~15
    keys, cells = 8 * B * p["n_bins"], 4 * p["M"] * p["nx"] * p["ny"]
    raw = ws.keys
    at = 2 * up(keys) + up(24 * B)
    return {"hit_min": raw[:keys].view(torch.int64).view(B, -1), "seen_max": raw[up(keys):up(keys) + keys].view(torch.int64).view(B, -1),
            "hits": raw[at:at + cells].view(torch.int32).view(p["M"], p["nx"], p["ny"])}


def assert_state(omap, state, what):
    for k, t in (("map", omap.log_odds), ("prev_origin", omap.prev_origin), ("cur_origin", omap.cur_origin), ("initialised", omap.initialised),
                 ("status", omap.status_word)):
        assert torch.equal(t, cuda(state[k])), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """Every call of the sequence: the outputs, and the bins and hit counts behind them; then the torus, the origins and the status."""
    from camradepth_amd import occupancy
    case = CASES[name]
    want, state = want_of(name)
    omap = new_map(case["params"])
    ws = occupancy.OccupancyWorkspace(omap, case["B"])
    assert ws.keys.numel() == occupancy_ref.workspace_bytes(case["B"], omap.n_bins, omap.M, omap.nx, omap.ny)
    for step, frame in enumerate(case["frames"]):
        got = feed(omap, case, frame, workspace=ws, out=ws.out)
        assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in OUT)
        assert_outputs(got, want[step], f"{name}, call {step}")
        for k, t in tables(ws, case["B"], case["params"]).items():
            assert torch.equal(t, cuda(want[step][k].view(np.int64) if k != "hits" else want[step][k])), (name, step, k)
    assert_state(omap, state, name)
    assert omap.status() == state["status"].tolist()


def test_a_pose_that_is_not_finite():
    """Three maps; a NaN centre for map 1 in the third call: the others update, map 1 is left as it was with evidence 0, and status
    bit 1 is set; an infinite sensor for frame 2 in the fourth: it contributes nothing, status bit 2."""
    from camradepth_amd import occupancy
    case = CASES["bad poses"]
    want, state = want_of("bad poses")
    omap = new_map(case["params"])
    seen = []
    for step, frame in enumerate(case["frames"]):
        got = feed(omap, case, frame)
        assert_outputs(got, want[step], f"call {step}")
        seen.append({k: v.clone() for k, v in got.items()})
        assert omap.status() == [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 2], [0, 1, 2]][step]
    assert torch.equal(seen[2]["log_odds"][1], seen[1]["log_odds"][1]) and torch.equal(seen[2]["origin"][1], seen[1]["origin"][1])
    assert int(seen[2]["evidence"][1].sum()) == 0 and int(seen[2]["evidence"][0].sum()) > 0 and int(seen[2]["evidence"][2].sum()) > 0
    assert not torch.equal(seen[2]["log_odds"][0], seen[1]["log_odds"][0])
    assert int(seen[3]["evidence"][2].sum()) == 0 and int(seen[3]["evidence"][1].sum()) > 0
    assert (occupancy.SKIPPED, occupancy.SENSOR_NOT_FINITE) == (1, 2)
    assert_state(omap, state, "bad poses")


def test_two_runs_stale_state_and_wrong_maps():
    """Two runs from reset() give the same bits; garbage in the workspace, the outputs and the torus of a reset map does not show; a
    call without workspace= and out= gives the same; M maps that fit no B are refused."""
    from camradepth_amd import occupancy
    from camradepth_amd import lib as L
    name = "5 x 7, 720 bins, one rig, compact"
    case = CASES[name]
    want, _ = want_of(name)
    omap = new_map(case["params"])
    ws = occupancy.OccupancyWorkspace(omap, case["B"])
    runs = []
    for run in range(3):
        omap.reset()
        if run == 2:
            ws.keys.fill_(0xA5)
            omap.log_odds.fill_(-12345)
            omap.prev_origin.fill_(3)
            for t in ws.out.values():
                t.fill_(SENTINEL)
        kw = dict(workspace=ws, out=ws.out) if run else {}
        runs.append([{k: v.clone() for k, v in feed(omap, case, frame, **kw).items()} for frame in case["frames"]])
    for run in runs:
        for step, got in enumerate(run):
            assert_outputs(got, want[step], f"{name}, call {step}")
    two = new_map(dict(case["params"], M=2))
    with pytest.raises(L.CrdError, match="2 maps for 3 frames"):
        feed(two, case, case["frames"][0])
    with pytest.raises(L.CrdError, match="workspace"):
        feed(new_map(dict(case["params"], nx=9)), case, case["frames"][0], workspace=ws)


def test_through_the_real_producers():
    """point_cloud -> update equals the restatement on the same cloud; unproject_depth -> update gives the same map."""
    from camradepth_amd import bev, cloud, occupancy
    from tests.test_gpu_bev import synthetic_depth
    rs = np.random.RandomState(70)
    B, h, w = 2, 32, 64
    size, s, cut = (64, 128), 2, 0
    depth = cuda(synthetic_depth(rs, B, h, w))
    K = cuda(np.array([[60.0, 0, 63.5], [0, 60.0, 31.5], [0, 0, 1.0]]))
    up = np.concatenate([bev.CAM_TO_BEV.numpy()[:, :3], [[0.25], [-0.5], [1.6]]], axis=1)              # the camera 1.6 m over the road
    p = occupancy_cases.params(M=2, nx=64, ny=48, n_bins=64, max_range=30.0, z_floor=-0.3, z_lo=0.3, z_hi=3.0)
    compact = cloud.point_cloud(depth, K, size, s, cut)
    n = int(compact["frame_offsets"][-1])
    assert n > 3000
    sensor = cuda(np.zeros(3))
    state = occupancy_ref.new_state(p)
    omap = new_map(p)
    for step in range(2):
        T = up.copy()
        T[0, 3] += 0.75 * step
        want = occupancy_ref.update(p, state, compact["xyz"].cpu().numpy(), B, frame_offsets=compact["frame_offsets"].cpu().numpy(), T=T,
                                    sensor=np.zeros(3))
        got = occupancy.update(omap, compact, map_from_points=cuda(T), sensor=sensor)
        assert_outputs(got, want, f"compact cloud, call {step}")
    assert (np.bincount(want["evidence"].ravel(), minlength=3) > 0).all()                     # unknown, free and occupied all occur
    organised = cloud.unproject_depth(depth, K, size, s, cut)
    other = new_map(p)
    for step in range(2):
        T = up.copy()
        T[0, 3] += 0.75 * step
        same = occupancy.update(other, organised, map_from_points=cuda(T))
    assert_outputs(same, want, "organised cloud")


def test_capture_on_a_side_stream():
    """update with a workspace, captured once; new rows, offsets and poses in the same buffers, replayed over a drive: the calls made
    one by one.  The map's state lives in its own tensors, so the replays fuse as the calls do."""
    from camradepth_amd import occupancy
    rs = np.random.RandomState(90)
    B = 3
    p = occupancy_cases.params(M=3, nx=16, ny=12, n_bins=64, max_range=8.0)
    n_rows = 900
    clouds = [np.concatenate([occupancy_cases.fan(rs, 300, 150, wall=2.5, reach=4.0) for _ in range(B)])[:n_rows] for _ in range(2)]
    assert all(len(c) == n_rows for c in clouds)
    steps = []
    for i, (x, y, heading) in enumerate(occupancy_cases.DRIVE):
        T = np.stack([occupancy_cases.pose(x + 0.3 * b, y, heading + b) for b in range(B)])
        steps.append(dict(xyz=clouds[i % 2], frame_offsets=np.array([0, 280 + i, 600 - i, n_rows - 4], np.int32), T=T,
                          centre=np.array([[1.0, 0.25 * i, 0.0]] * B)))
    state = occupancy_ref.new_state(p)
    want = [occupancy_ref.update(p, state, B=B, **f) for f in steps]
    omap = new_map(p)
    ws = occupancy.OccupancyWorkspace(omap, B)
    xyz, off, T, centre = (cuda(steps[0][k]) for k in ("xyz", "frame_offsets", "T", "centre"))

    def call():
        return occupancy.update(omap, xyz, off, map_from_points=T, centre=centre, workspace=ws, out=ws.out)

    def load(f):
        xyz.copy_(cuda(f["xyz"])), off.copy_(cuda(f["frame_offsets"])), T.copy_(cuda(f["T"])), centre.copy_(cuda(f["centre"]))

    for i, f in enumerate(steps):                                              # eager, one by one: also loads the code objects
        load(f)
        assert_outputs(call(), want[i], f"eager call {i}")
    load(steps[0])
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    omap.reset()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream, three launches in a row
        call()
    omap.reset()                                                               # the capture runs nothing, the call before it did
    for i, f in enumerate(steps):
        load(f)
        for t in ws.out.values():
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_outputs(ws.out, want[i], f"replay {i}")
    assert_state(omap, state, "after the replays")


def test_picture_is_colorize_of_the_log_odds():
    from camradepth_amd import occupancy, viz
    name = "40 x 36, 8 bins, one rig, bare xyz"
    case = CASES[name]
    omap = new_map(case["params"])
    for frame in case["frames"][:3]:
        res = feed(omap, case, frame)
    got = occupancy.picture(res, omap)
    assert got.dtype == torch.uint8 and got.shape == (1, 40, 36, 3)
    assert torch.equal(got, viz.colorize(res["value"], "jet", vmin=-10.0, vmax=10.0)) and torch.equal(got, occupancy.picture(res, 10))
    assert torch.equal(res["value"], res["log_odds"].float()) and len(got.view(-1, 3).unique(dim=0)) >= 3
    canvas = torch.full((1, 40, 36, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    assert occupancy.picture(res, omap, cmap="rainbow", out=canvas).data_ptr() == canvas.data_ptr()
    assert torch.equal(canvas, viz.colorize(res["value"], "rainbow", vmin=-10.0, vmax=10.0)) and not torch.equal(canvas, got)


def test_live_pipeline_with_a_map():
    """LivePipeline(cloud=, occupancy=) over three frames of a drive: run()['occupancy'] has the bits of occupancy.update on the
    clouds of the stages called one by one, fused from an EMPTY map -- the pipeline's warm-up pass before the capture updates the map
    for real and has to be undone; everything else equals a pipeline built without occupancy=."""
    from camradepth_amd import bev, occupancy, viz
    from camradepth_amd import lib as L
    from camradepth_amd.inference import InferenceGraph
    from camradepth_amd.live import LivePipeline
    from tests.test_gpu_live import B, CLOUD, CUT, H, N_SWEEPS, S, SIZE, W, assert_same, flat, sensor_set, small_model, stagewise
    model = small_model()
    opts = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=120.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
                occupied_at=4, free_at=2)
    with pytest.raises(L.CrdError, match="cloud"):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, occupancy=opts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={},
                        occupancy=dict(opts, centre=(20.0, 0.0, 0.0), picture=True))
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={})
    assert live.occupancy_map.M == B and live.occupancy_map.status() == [0, 0]
    with pytest.raises(L.CrdError, match="map_from_out"):
        plain.run(map_from_out=torch.eye(3, 4, dtype=torch.float64, device="cuda"), **sensor_set(11, (350, 250)))
    ig, vz = InferenceGraph(model, B, H, W), viz.Visualizer(B, H, W)
    fresh = occupancy.OccupancyMap(B, device="cuda", **opts)
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)                             # x forward, y left, z up
    out_from_cam = out_from_cam.cuda()
    centre, views, evidence = cuda(np.array([20.0, 0.0, 0.0])), [], []
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = None if i == 0 else cuda(occupancy_cases.pose(3.0 * i, -2.5 * i, 0.2 * i))
        res = live.run(map_from_out=pose, **c)
        assert set(res) == {"image", "x", "radar", "rad_vel", "pred", "cloud", "occupancy", "pictures"}
        assert set(res["occupancy"]) == set(OUT) | {"picture"}
        views.append({k: v.data_ptr() for k, v in res["occupancy"].items()})
        got_map = {k: v.clone() for k, v in res["occupancy"].items()}
        got = {k: v.clone() for k, v in flat(res).items()}
        torch.cuda.synchronize()
        assert_same(got, {k: v.clone() for k, v in flat(plain.run(**c)).items()}, f"frame {i}: with and without occupancy=")
        stages = stagewise(model, ig, vz, c)
        want = occupancy.update(fresh, stages["cloud"], map_from_points=pose, sensor=out_from_cam[:, 3].contiguous(), centre=centre)
        want["picture"] = occupancy.picture(want, fresh)
        assert_same(got_map, want, f"frame {i}")
        evidence.append(want["evidence"].clone())
    alone = lambda r: torch.where(r["evidence"] == 2, 3, torch.where(r["evidence"] == 1, -1, 0)).int()      # noqa: E731: one frame into an empty map
    assert views[0] == views[1] == views[2] and int((evidence[0] > 0).sum()) > 0 and live.occupancy_map.status() == [0, 0]
    assert not torch.equal(want["log_odds"].int(), alone(want))                                      # fused over the frames
    copies = live.run(clone=True, map_from_out=pose, **c)["occupancy"]
    assert all(copies[k].data_ptr() != p for k, p in views[0].items())
    live.occupancy_map.reset()
    again = live.run(map_from_out=pose, **c)["occupancy"]
    assert torch.equal(again["log_odds"].int(), alone(again))
