"""GPU: camradepth_amd.match -- the pose of a cloud corrected against the occupancy map -- against tests/match_ref.py, the NumPy
restatement of include/camradepth_hip.h (itself held to a plain loop, to planted offsets and to invariants in
tests/test_match_ref_cpu.py).  The map of a case is the restatement's, copied up; every output, the full score table included, is
compared bit for bit with torch.equal, fp64 through an int64 view."""
import numpy as np
import pytest
import torch

from tests import match_cases, match_ref

pytestmark = pytest.mark.gpu

CASES = match_cases.all_cases()
_WANT = {}
SENTINEL = 7
KEYS = match_ref.OUT + ("scores",)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def want_of(name, i):
    """The restatement's outputs of match i of case `name`, computed once and left unchanged."""
    if (name, i) not in _WANT:
        _WANT[name, i] = match_cases.match_of(CASES[name], match_cases.state_of(name, CASES[name]), i)
    return _WANT[name, i]


def same(a, b, what):
    b = cuda(b) if isinstance(b, np.ndarray) else b
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    assert torch.equal(a, b), f"{what} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def map_of(name):
    """An OccupancyMap that holds the restatement's map of the case."""
    from camradepth_amd import occupancy
    c = CASES[name]
    p, state = c["params"], match_cases.state_of(name, c)
    omap = occupancy.OccupancyMap(**p)
    omap.log_odds.copy_(cuda(state["map"]))
    omap.prev_origin.copy_(cuda(state["prev_origin"]))
    omap.cur_origin.copy_(cuda(state["cur_origin"]))
    omap.initialised.copy_(cuda(state["initialised"]))
    return omap


def arguments(c, kw):
    """-> (cloud_or_xyz, keyword arguments) of match_scan and occupancy.update for the case's form of a cloud."""
    B, form = c["B"], c.get("form", "compact")
    T = kw.get("T")
    more = dict(map_from_points=cuda(T), sensor=cuda(kw.get("sensor")))
    if form == "organised":
        rows = kw["rows_per_frame"]
        return {"points": cuda(kw["xyz"]).view(B, 1, rows, 3), "valid": cuda(kw["valid"]).view(B, 1, rows)}, more
    if form == "bare":
        return cuda(kw["xyz"]), dict(more, frame_offsets=cuda(kw["frame_offsets"]), valid=cuda(kw.get("valid")))
    return {"xyz": cuda(kw["xyz"]), "frame_offsets": cuda(kw["frame_offsets"])}, dict(more, valid=cuda(kw.get("valid")))


def spec_of(match):
    from camradepth_amd import match as mt
    return mt.MatchSpec(**match["spec"])


def assert_match(got, want, what):
    assert set(got) == set(KEYS), (what, sorted(got))
    for k in KEYS:
        same(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """Every output of every match of the case, written into buffers full of a sentinel; the map is left as it was."""
    from camradepth_amd import match as mt
    c, omap = CASES[name], map_of(name)
    before = {k: getattr(omap, k).clone() for k in ("log_odds", "prev_origin", "cur_origin", "initialised", "status_word")}
    for i, match in enumerate(c["matches"]):
        spec = spec_of(match)
        ws = mt.MatchWorkspace(omap, spec, c["B"], scores=True)
        for t in ws.out.values():
            t.view(torch.uint8).fill_(SENTINEL)
        cloud, more = arguments(c, match["kw"])
        got = mt.match_scan(omap, spec, cloud, workspace=ws, scores=True, **more)
        assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in KEYS)
        assert_match(got, want_of(name, i), f"{name}, match {i}")
        planted = match.get("planted")
        if planted is not None and name not in ("a corridor", "an uninitialised map"):      # recovered on the device
            kept = (got["status"] & mt.KEEPS_PRIOR) != 0
            assert got["pick"][~kept].tolist() == [list(planted)] * int((~kept).sum()) and int((~kept).sum()) >= c["params"]["M"] - 1
    for k, v in before.items():
        same(getattr(omap, k), v, f"{name}: the map's {k} after the matches")


def test_without_workspace_and_without_the_table():
    from camradepth_amd import match as mt
    name = "three maps, compact"
    c, omap = CASES[name], map_of(name)
    match = c["matches"][0]
    cloud, more = arguments(c, match["kw"])
    got = mt.match_scan(omap, spec_of(match), cloud, **more)
    assert set(got) == set(match_ref.OUT)
    for k in match_ref.OUT:
        same(got[k], want_of(name, 0)[k], f"{name} without workspace=: {k}")


def test_the_corrected_pose_feeds_the_update():
    """update with out['pose'] marks the cells the map already holds: after a planted offset no new cell turns up occupied, while the
    update with the prior smears the wall."""
    from camradepth_amd import match as mt
    from camradepth_amd import occupancy
    name = "37 x 53, planted offsets"
    c = CASES[name]
    match = c["matches"][4]
    cloud, more = arguments(c, match["kw"])
    new_cells = []
    for corrected in (True, False):
        omap = map_of(name)
        had = omap.log_odds > 0                                              # the torus: a slot is a world cell, wherever the window goes
        pose = mt.match_scan(omap, spec_of(match), cloud, **more)["pose"] if corrected else more["map_from_points"]
        occupancy.update(omap, cloud, map_from_points=pose, sensor=more["sensor"], valid=more["valid"])
        new_cells.append(int(((omap.log_odds > 0) & ~had).sum()))
    assert new_cells[0] == 0 and new_cells[1] > 0


def test_capture_on_a_side_stream():
    """match_scan with its workspace, captured once; the cloud and the prior changed in place and the graph replayed: the eager
    calls.  A call allocates nothing."""
    from camradepth_amd import match as mt
    name = "37 x 53, planted offsets"
    c, omap = CASES[name], map_of(name)
    spec = spec_of(c["matches"][0])
    ws = mt.MatchWorkspace(omap, spec, 1, scores=True)
    cloud, more = arguments(c, c["matches"][1]["kw"])
    prior = more["map_from_points"]

    def call():
        return mt.match_scan(omap, spec, cloud, workspace=ws, scores=True, **more)

    call()                                                                     # eager: also loads the code object
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream
        got = call()
    for i in (3, 1, 1, 4):                                                     # match 1 twice in a row: a replay leaves nothing behind
        prior.copy_(cuda(c["matches"][i]["kw"]["T"]))
        for t in ws.out.values():
            t.view(torch.uint8).fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_match(got, want_of(name, i), f"replay of match {i}")


def test_live_pipeline_with_match():
    """LivePipeline(cloud=, occupancy=, match=) over three frames: run()['match'] has the bits of match_scan called alone on the run's
    own cloud against a map kept beside it, run()['occupancy'] those of the update with the corrected pose, and a pipeline without
    match= those of the update with the pose as it came."""
    from camradepth_amd import bev, occupancy
    from camradepth_amd import lib as L
    from camradepth_amd import match as mt
    from camradepth_amd.live import LivePipeline
    from tests.occupancy_cases import pose as pose_of
    from tests.test_gpu_live import B, CLOUD, CUT, N_SWEEPS, S, SIZE, sensor_set, small_model
    model = small_model()
    opts = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=120.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
                occupied_at=3, free_at=1, centre=(20.0, 0.0, 0.0))
    mopts = dict(n_xy=3, n_theta=2, d_theta=0.02, min_cells=0, min_score=-10 ** 9)
    with pytest.raises(L.CrdError, match="match= needs occupancy="):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, match=mopts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, match=mopts)
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts)
    assert live.match_spec.n_xy == 3 and plain.match_spec is None and not bool(live.occupancy_map.initialised.any())
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)
    out_from_cam = out_from_cam.cuda()
    map_opts = {k: opts[k] for k in occupancy.MAP_OPTIONS}
    beside, raw = (occupancy.OccupancyMap(B, 64, 48, 2.0, **map_opts) for _ in range(2))
    beside.cur_origin.copy_(live.occupancy_map.cur_origin)                    # reset() leaves the origins: n_cells of an empty map counts
    beside.prev_origin.copy_(live.occupancy_map.prev_origin)                  # inside the window it had
    spec = mt.MatchSpec(**mopts)
    sensor = out_from_cam[:, 3].expand(B, 3).contiguous()
    centre = torch.tensor(opts["centre"], dtype=torch.float64, device="cuda")
    views, applied = [], 0
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = cuda(np.stack([pose_of(3.0 * i, -2.5 * i, 0.2 * i)] * B))
        res = live.run(map_from_out=pose, **c)
        assert "match" in res and set(res["match"]) == set(match_ref.OUT)
        views.append({k: v.data_ptr() for k, v in res["match"].items()})
        got = {k: v.clone() for k, v in res["match"].items()}
        got_map = {k: v.clone() for k, v in res["occupancy"].items()}
        cloud = {k: v.clone() for k, v in res["cloud"].items() if torch.is_tensor(v)}
        torch.cuda.synchronize()
        want = mt.match_scan(beside, spec, cloud, map_from_points=pose, sensor=sensor)
        for k in want:
            same(got[k], want[k], f"frame {i}: match.{k}")
        status = got["status"].tolist()
        assert all(s & mt.UNINITIALISED for s in status) if i == 0 else not any(s & mt.KEEPS_PRIOR for s in status), (i, status)
        if i == 0:
            same(got["pose"], pose, "frame 0: the prior passes through")
        applied += int((got["pick"] != 0).any())
        want_map = occupancy.update(beside, cloud, map_from_points=want["pose"], sensor=sensor, centre=centre)
        for k in want_map:
            same(got_map[k], want_map[k], f"frame {i}: occupancy.{k} with match=")
        other = plain.run(map_from_out=pose, **c)
        assert "match" not in other
        want_raw = occupancy.update(raw, cloud, map_from_points=pose, sensor=sensor, centre=centre)
        for k in want_raw:
            same(other["occupancy"][k], want_raw[k], f"frame {i}: occupancy.{k} without match=")
    assert views[0] == views[1] == views[2]
