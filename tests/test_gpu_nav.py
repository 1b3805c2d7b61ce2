"""GPU: camradepth_amd.nav -- the cost-to-go of a costmap, its direction map and the planned paths -- against tests/nav_ref.py, the NumPy
restatement of include/camradepth_hip.h (itself held to heap Dijkstra and scipy's in tests/test_nav_ref_cpu.py).  Everything is compared
bit for bit with torch.equal, the paths' cell centres through an int64 view."""
import numpy as np
import pytest
import torch

from tests import nav_cases, nav_ref

pytestmark = pytest.mark.gpu

CASES = nav_cases.all_cases()
OUT = ("togo", "next", "info")
PATH_OUT = ("cells", "xy", "n_cells", "start_togo", "status")
SERPENTINE = "33 x 65, a serpentine of column walls"
_WANT = {}
SENTINEL = 7


def cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def want_of(name):
    """The restatement's field and paths of case `name`, computed once and left unchanged."""
    if name not in _WANT:
        c = CASES[name]
        f = nav_ref.nav_field(c["cost"], c["goals"], c["n_goals"], c["origin"], c["cell"], c["neutral"], c["blocked_at"], 64)
        _WANT[name] = (f, nav_ref.plan_paths(c["starts"], c["path_map"], c["origin"], c["cell"], f["togo"], f["next"], c["P"]))
    return _WANT[name]


def spec_of(c, **kw):
    from camradepth_amd import nav
    return nav.NavSpec(c["cell"], **dict(dict(neutral=c["neutral"], blocked_at=c["blocked_at"]), **kw))


def same(a, b, what):
    b = cuda(b) if isinstance(b, np.ndarray) else b
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    assert torch.equal(a, b), f"{what} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def assert_field(got, want, what):
    assert set(got) == set(OUT), (what, sorted(got))
    same(got["togo"], want["togo"], f"{what}: togo")
    same(got["next"], want["next"], f"{what}: next")
    same(got["info"][:, [0, 2, 3]], want["info"][:, [0, 2, 3]], f"{what}: info")
    rounds = got["info"][:, 1]
    assert bool((rounds >= 1).all()) and bool((rounds <= 64).all()), (what, rounds.tolist())


def assert_paths(got, want, what):
    assert set(got) == set(PATH_OUT), (what, sorted(got))
    for k in PATH_OUT:
        same(got[k], want[k], f"{what}: {k}")


def inputs(c):
    return cuda(c["cost"]), cuda(c["origin"]), cuda(c["goals"]), cuda(c["n_goals"]), cuda(c["starts"]), cuda(c["path_map"])


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """Field and paths written into buffers full of a sentinel; a second run and a call without workspace= and out= give the same bits."""
    from camradepth_amd import nav
    c = CASES[name]
    want, want_paths = want_of(name)
    spec = spec_of(c)
    cost, origin, goals, n_goals, starts, path_map = inputs(c)
    ws = nav.NavWorkspace(spec, *cost.shape)
    pout = nav.path_outputs(len(c["starts"]), c["P"])
    for t in list(ws.out.values()) + list(pout.values()):
        t.fill_(SENTINEL)
    got = nav.nav_field(spec, cost, origin, goals, n_goals, workspace=ws)
    assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in OUT)
    assert_field(got, want, name)
    paths = nav.plan_paths(spec, got, origin, starts, c["P"], path_map, out=pout)
    assert all(paths[k].data_ptr() == pout[k].data_ptr() for k in PATH_OUT)
    assert_paths(paths, want_paths, name)
    first = {k: v.clone() for k, v in list(got.items()) + list(paths.items())}
    again = nav.nav_field(spec, {"cost": cost}, {"origin": origin}, goals, n_goals, workspace=ws, out=ws.out)
    again_paths = nav.plan_paths(spec, again, (None, origin), starts, c["P"], path_map, out=pout)
    fresh = nav.nav_field(spec, cost, origin, goals, n_goals)
    fresh_paths = nav.plan_paths(spec, fresh, origin, starts, c["P"], path_map)
    for k in OUT + PATH_OUT:
        same(dict(again, **again_paths)[k], first[k], f"{name}, second run: {k}")
        same(dict(fresh, **fresh_paths)[k], first[k], f"{name}, without workspace= and out=: {k}")
        assert dict(fresh, **fresh_paths)[k].data_ptr() != first[k].data_ptr()


def test_outputs_left_out_and_arguments_refused():
    from camradepth_amd import lib as L
    from camradepth_amd import nav
    name = "two maps of 13 x 17, n_goals 2 and 1"
    c = CASES[name]
    want, want_paths = want_of(name)
    spec = spec_of(c)
    cost, origin, goals, n_goals, starts, path_map = inputs(c)
    out = {"togo": torch.full(cost.shape, SENTINEL, dtype=torch.int32, device="cuda"), "next": None,
           "info": torch.full((2, 4), SENTINEL, dtype=torch.int32, device="cuda")}
    got = nav.nav_field(spec, cost, origin, goals, n_goals, out=out)                         # NULL for the kernel: no third launch
    assert got["next"] is None
    same(got["togo"], want["togo"], "without next: togo")
    with pytest.raises(L.CrdError, match="'next'"):
        nav.plan_paths(spec, got, origin, starts, c["P"])
    full = nav.nav_field(spec, cost, origin, goals, n_goals)
    no_xy = nav.plan_paths(spec, full, origin, starts, c["P"], path_map, xy=False)
    assert set(no_xy) == set(PATH_OUT) - {"xy"}
    for k in no_xy:
        same(no_xy[k], want_paths[k], f"without xy: {k}")
    all_goals = nav.nav_field(spec, cost, origin, goals)                                     # n_goals None: both goals of map 1 as well
    ref = nav_ref.nav_field(c["cost"], c["goals"], None, c["origin"], c["cell"], c["neutral"], c["blocked_at"], 64)
    assert not np.array_equal(ref["togo"], want["togo"])
    assert_field(all_goals, ref, "n_goals None")
    on_map_0 = nav.plan_paths(spec, full, origin, starts, c["P"])                            # path_map None: map 0 for every path
    ref = nav_ref.plan_paths(c["starts"], None, c["origin"], c["cell"], want["togo"], want["next"], c["P"])
    assert_paths(on_map_0, ref, "path_map None")
    with pytest.raises(L.CrdError, match="togo"):
        nav.nav_field(spec, cost, origin, goals, out=dict(out, togo=None))
    with pytest.raises(L.CrdError, match="workspace"):
        nav.nav_field(spec, cost[:1], origin[:1], goals[:1], workspace=nav.NavWorkspace(spec, *cost.shape))
    with pytest.raises(L.CrdError, match="origin"):
        nav.nav_field(spec, cost, origin[:1], goals)
    with pytest.raises(L.CrdError, match="n_goals"):
        nav.nav_field(spec, cost, origin, goals, n_goals[:1])
    with pytest.raises(L.CrdError, match="path_map"):
        nav.plan_paths(spec, full, origin, starts, c["P"], path_map[:2])


def test_one_round_of_the_serpentine():
    from camradepth_amd import nav
    c = CASES[SERPENTINE]
    want, _ = want_of(SERPENTINE)
    cost, origin, goals, n_goals, _, _ = inputs(c)
    got = nav.nav_field(spec_of(c, max_rounds=1), cost, origin, goals, n_goals)
    assert got["info"][0].tolist() == [0, 1, 1, 0]
    fixed = cuda(want["togo"])
    assert bool((got["togo"] >= fixed).all()) and bool((got["togo"] > fixed).any())
    done = nav.nav_field(spec_of(c, max_rounds=c["rounds"]), cost, origin, goals, n_goals)  # the rounds the restatement's order needs
    assert_field(done, want, "max_rounds 9")
    assert done["info"][0, 1].item() == c["rounds"]


def test_a_planned_path_passes_check_paths():
    """The cell centres of plan_paths, as they are, through field.check_paths on the costmap they were planned on."""
    from camradepth_amd import field, nav
    from tests import field_cases
    state_np = field_cases.scatter(6, (1, 40, 36), 0.03)
    spec = field.FieldSpec(0.5, max_cells=4, inscribed=0.5, scale=1.0)
    state, origin = cuda(state_np), cuda(np.array([[-7, 3]], np.int64))
    f = field.distance_field(spec, state)
    cost = f["cost"].cpu().numpy()
    gi, gj = nav_cases.passable_near(cost[0], 253, 20, 18)
    nspec = nav.NavSpec(0.5)
    goals = cuda(np.array([[nav_cases.centre((-7, 3), 0.5, gi, gj)]], np.float64))
    res = nav.nav_field(nspec, f, {"state": state, "origin": origin}, goals)
    ii, jj = np.nonzero(res["togo"][0].cpu().numpy() != nav_ref.UNREACHED)
    assert ii.size > 100
    pick = np.linspace(0, ii.size - 1, 24).astype(np.int64)
    starts = cuda(np.array([nav_cases.centre((-7, 3), 0.5, ii[q], jj[q]) for q in pick], np.float64))
    P = 120
    paths = nav.plan_paths(nspec, res, (state, origin), starts, P)
    assert bool((paths["status"] == 0).all()) and int(paths["n_cells"].max()) > 10
    checked = field.check_paths(spec, f, (state, origin), paths["xy"], n_poses=paths["n_cells"], pose_cell=True)
    assert bool((checked["first_blocked"] == -1).all()) and bool((checked["n_outside"] == 0).all())
    counted = torch.arange(P, device="cuda")[None, :] < paths["n_cells"][:, None]
    assert torch.equal(torch.where(counted, checked["pose_cell"], -1), paths["cells"])       # the centres fall into the cells they name


def test_capture_of_both_entries_on_a_side_stream():
    """nav_field and plan_paths with their buffers, captured once; the goals, the starts and the costmap changed in place, replayed:
    the calls made one by one."""
    from camradepth_amd import nav
    name = "two maps of 13 x 17, n_goals 2 and 1"
    c = CASES[name]
    spec = spec_of(c)
    rs = np.random.RandomState(8)
    steps = []
    for s in range(3):
        cost_np = c["cost"] if s == 0 else nav_cases.scattered(40 + s, c["cost"].shape, 0.05, R=3, scale=2.0)
        goals_np = c["goals"] if s == 0 else c["goals"] + rs.uniform(-1.5, 1.5, c["goals"].shape)
        starts_np = c["starts"] if s == 0 else c["starts"] + rs.uniform(-1.0, 1.0, c["starts"].shape)
        f = nav_ref.nav_field(cost_np, goals_np, c["n_goals"], c["origin"], c["cell"], c["neutral"], c["blocked_at"], 64)
        steps.append((cost_np, goals_np, starts_np, f,
                      nav_ref.plan_paths(starts_np, c["path_map"], c["origin"], c["cell"], f["togo"], f["next"], c["P"])))
    cost, origin, goals, n_goals, starts, path_map = inputs(c)
    ws = nav.NavWorkspace(spec, *cost.shape)
    pout = nav.path_outputs(len(c["starts"]), c["P"])

    def call():
        f = nav.nav_field(spec, cost, origin, goals, n_goals, workspace=ws)
        return f, nav.plan_paths(spec, f, origin, starts, c["P"], path_map, out=pout)

    call()                                                                     # eager: also loads the code objects
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream, four launches in a row
        call()
    for s, (cost_np, goals_np, starts_np, f, p) in enumerate(steps):
        cost.copy_(cuda(cost_np)), goals.copy_(cuda(goals_np)), starts.copy_(cuda(starts_np))
        for t in list(ws.out.values()) + list(pout.values()):
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_field(ws.out, f, f"replay {s}")
        assert_paths(pout, p, f"replay {s}")
    assert not np.array_equal(steps[0][3]["togo"], steps[1][3]["togo"]) and not np.array_equal(steps[0][4]["cells"], steps[1][4]["cells"])


def test_live_pipeline_with_a_navigation_field():
    """LivePipeline(cloud=, occupancy=, field=, nav=) over three frames: run()['nav'] has the bits of the stages called alone on the run's
    own field output, and everything else equals a pipeline built without nav=."""
    from camradepth_amd import bev, field, nav
    from camradepth_amd import lib as L
    from camradepth_amd.live import LivePipeline
    from tests.occupancy_cases import pose as pose_of
    from tests.test_gpu_live import B, CLOUD, CUT, N_SWEEPS, S, SIZE, assert_same, flat, sensor_set, small_model
    model = small_model()
    opts = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=120.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
                occupied_at=3, free_at=1, centre=(20.0, 0.0, 0.0))
    fopts = dict(max_cells=5, sources=(2,), inscribed=2.0, scale=0.2)
    G, K, P = 2, 5, 90
    nopts = dict(goals=G, starts=(K, P), neutral=20, blocked_at=200, max_rounds=32)
    with pytest.raises(L.CrdError, match="nav= needs field="):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, nav=nopts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, field=fopts, nav=nopts)
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, field=fopts)
    M = live.occupancy_map.M
    assert live.nav_spec.cell == 2.0 and bool(torch.isnan(live.nav_goals).all()) and bool(torch.isnan(live.nav_starts).all())
    assert live.nav_goals.shape == (M, G, 2) and live.nav_starts.shape == (K, 2)
    with pytest.raises(L.CrdError, match="goals"):
        plain.run(goals=torch.zeros(M, G, 2, dtype=torch.float64, device="cuda"), **sensor_set(11, (350, 250)))
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)
    out_from_cam = out_from_cam.cuda()
    spec = nav.NavSpec(2.0, neutral=20, blocked_at=200, max_rounds=32)
    rs = np.random.RandomState(5)
    views, reached = [], 0
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = None if i == 0 else cuda(pose_of(3.0 * i, -2.5 * i, 0.2 * i))
        goals = None if i == 0 else cuda(np.stack([rs.uniform(-30.0, 70.0, (M, G)), rs.uniform(-40.0, 40.0, (M, G))], -1))
        starts = None if i == 0 else cuda(np.stack([rs.uniform(-50.0, 90.0, K), rs.uniform(-50.0, 50.0, K)], -1))
        res = live.run(map_from_out=pose, goals=goals, starts=starts, **c)
        assert "nav" in res and set(res["nav"]) == set(OUT) | {"paths"} and set(res["nav"]["paths"]) == set(PATH_OUT)
        views.append({k: v.data_ptr() for k, v in res["nav"].items() if k != "paths"})
        got_paths = {k: v.clone() for k, v in res["nav"]["paths"].items()}
        got_nav = {k: v.clone() for k, v in res["nav"].items() if k != "paths"}
        field_out = {k: v.clone() for k, v in res["field"].items()}
        occ_out = {k: v.clone() for k, v in res["occupancy"].items()}
        got = {k: v.clone() for k, v in flat(dict((k, v) for k, v in res.items() if k != "nav")).items()}
        torch.cuda.synchronize()
        other = plain.run(map_from_out=pose, **c)
        assert "nav" not in other
        assert_same(got, {k: v.clone() for k, v in flat(other).items()}, f"frame {i}: with and without nav=")
        for k in field_out:
            same(field_out[k], other["field"][k].clone(), f"frame {i}: the field with and without nav=: {k}")
        if i == 0:                                                              # the goals and starts a pipeline starts with: none
            assert got_nav["info"][:, [0, 2, 3]].tolist() == [[1, 0, G]] * M and bool((got_nav["togo"] == nav.UNREACHED).all())
            assert got_paths["status"].tolist() == [2] * K and got_paths["n_cells"].tolist() == [0] * K
            continue
        want = nav.nav_field(spec, field_out, occ_out, goals)
        for k in OUT:
            same(got_nav[k], want[k], f"frame {i}: nav {k}")
        alone = nav.plan_paths(spec, want, occ_out, starts, P)
        for k in PATH_OUT:
            same(got_paths[k], alone[k], f"frame {i}: paths {k}")
        reached += int((want["togo"] != nav.UNREACHED).sum())
    assert reached > 0 and views[0] == views[1] == views[2]
