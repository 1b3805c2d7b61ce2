"""GPU: camradepth_amd.rollout -- the local planner -- against tests/rollout_ref.py, the NumPy restatement of include/camradepth_hip.h
(itself held to a plain loop, to the closed form of its tables and to the behaviour of a planner in tests/test_rollout_ref_cpu.py).
Every output, the per-candidate tables and 'xy' included, is compared bit for bit with torch.equal, fp64 through an int64 view."""
import numpy as np
import pytest
import torch

from tests import rollout_cases, rollout_ref

pytestmark = pytest.mark.gpu

CASES = rollout_cases.all_cases()
SENTINEL = 7
KEYS = rollout_ref.OUT + rollout_ref.TABLES + ("xy",)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b, what):
    b = cuda(b) if isinstance(b, np.ndarray) else b
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    assert torch.equal(a, b), f"{what} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def spec_of(case):
    from camradepth_amd import rollout
    return rollout.RolloutSpec(**case["spec"])


def tracks_of(case):
    """An ObjectTracks that holds the case's track tables, or None."""
    from camradepth_amd import tracks
    if case["tracks"] is None:
        return None
    sc, T = case["scene"], case["tracks"].shape[1]
    t = tracks.ObjectTracks(tracks.TrackSpec(max_tracks=T), sc["M"], sc["nx"], sc["ny"], sc["cell"])
    t.tracks.copy_(cuda(case["tracks"]))
    t.pos.copy_(cuda(case["pos"]))
    t.vel.copy_(cuda(case["vel"]))
    return t


def arguments(case):
    """-> (pose, field_result, (state, origin), keyword arguments) of plan_rollouts."""
    sc = case["scene"]
    field_result = {"dist2": cuda(sc["dist2"]), "cost": cuda(sc["cost"])}
    nav_result = None if case["togo"] is None else {"togo": cuda(case["togo"])}
    return cuda(case["pose"]), field_result, (cuda(sc["state"]), cuda(sc["origin"])), dict(nav_result=nav_result, tracks=tracks_of(case),
                                                                                          twist=cuda(case["twist"]))


def assert_rollouts(got, want, what, keys=KEYS):
    assert set(got) == set(keys), (what, sorted(got))
    for k in keys:
        same(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """Every output of the case, written into buffers full of a sentinel; the inputs are left as they were."""
    from camradepth_amd import rollout
    case = CASES[name]
    spec = spec_of(case)
    ws = rollout.RolloutWorkspace(spec, case["scene"]["M"], tables=True, xy=True)
    assert ws.buf.numel() == rollout_ref.workspace_bytes(case["scene"]["M"], spec.K)
    for t in ws.out.values():
        t.view(torch.uint8).fill_(SENTINEL)
    pose, field_result, state_origin, kw = arguments(case)
    before = [t.clone() for t in (pose, field_result["cost"], state_origin[1])]
    got = rollout.plan_rollouts(spec, pose, field_result, state_origin, workspace=ws, tables=True, xy=True, **kw)
    assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in KEYS)
    assert_rollouts(got, rollout_cases.want_of(name), name)
    for t, b in zip((pose, field_result["cost"], state_origin[1]), before):
        same(t, b, f"{name}: an input after the call")
    if kw["tracks"] is not None:
        same(kw["tracks"].pos, case["pos"], f"{name}: the tracks' pos after the call")


def test_without_workspace_and_without_the_tables():
    from camradepth_amd import rollout
    name = "64 x 65, 3 maps, K 45, P 64, T 64, nav, twist"
    case = CASES[name]
    pose, field_result, state_origin, kw = arguments(case)
    got = rollout.plan_rollouts(spec_of(case), pose, field_result, state_origin, **kw)
    assert_rollouts(got, rollout_cases.want_of(name), f"{name} without workspace=", rollout_ref.OUT)
    got = rollout.plan_rollouts(spec_of(case), pose, field_result, {"state": state_origin[0], "origin": state_origin[1]}, xy=True, **kw)
    assert_rollouts(got, rollout_cases.want_of(name), f"{name} with xy alone", rollout_ref.OUT + ("xy",))


def test_check_paths_takes_xy_as_it_is():
    """field.check_paths on a map's 'xy': the static half.  Without tracks its first_blocked and max_cost are the planner's."""
    from camradepth_amd import field, rollout
    name = "K 15, P 65, no tracks, leaves the window, outside blocks"
    case = CASES[name]
    sc = case["scene"]
    pose, field_result, state_origin, kw = arguments(case)
    got = rollout.plan_rollouts(spec_of(case), pose, field_result, state_origin, tables=True, xy=True, **kw)
    fspec = field.FieldSpec(sc["cell"], max_cells=rollout_cases.R)
    paths = field.check_paths(fspec, field_result, state_origin, got["xy"][0])
    same(paths["first_blocked"], got["first_blocked"][0], "first_blocked by check_paths")
    same(paths["max_cost"].to(torch.int32), got["max_cost"][0], "max_cost by check_paths")
    assert bool((paths["first_blocked"] >= 0).any()) and bool((paths["first_blocked"] < 0).any()) and bool((paths["n_outside"] > 0).any())


def test_capture_on_a_side_stream():
    """plan_rollouts with its workspace, captured once; the pose, the twist and the tracks changed in place and the graph replayed: the
    restatement's bits for the changed inputs.  A call allocates nothing."""
    from camradepth_amd import rollout
    name = "64 x 65, 3 maps, K 45, P 64, T 64, nav, twist"
    case = CASES[name]
    spec = spec_of(case)
    ws = rollout.RolloutWorkspace(spec, 3, tables=True, xy=True)
    pose, field_result, state_origin, kw = arguments(case)

    def call():
        return rollout.plan_rollouts(spec, pose, field_result, state_origin, workspace=ws, tables=True, xy=True, **kw)

    call()                                                                     # eager: also loads the code object
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream
        got = call()
    rng = np.random.default_rng(3)
    steps = []
    for step in range(3):
        moved = dict(case)
        if step:                                                               # step 0: the case itself
            moved["pose"] = rollout_cases.vehicle(case["scene"], 40 + step, where=(0.35, 0.45))
            moved["twist"] = case["twist"] + rng.uniform(-0.2, 0.2, case["twist"].shape)
            moved["vel"] = -case["vel"]
        steps.append(rollout_ref.plan_rollouts(moved["spec"], **rollout_cases.arguments(moved)))
        pose.copy_(cuda(moved["pose"]))
        kw["twist"].copy_(cuda(moved["twist"]))
        kw["tracks"].vel.copy_(cuda(moved["vel"]))
        for t in ws.out.values():
            t.view(torch.uint8).fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_rollouts(got, steps[-1], f"replay {step}")
    assert_rollouts(call(), steps[-1], "the eager call after the replays")
    assert not np.array_equal(steps[0]["scores"], steps[1]["scores"]) and not np.array_equal(steps[1]["first_track"], steps[2]["first_track"])


def test_live_pipeline_with_rollouts():
    """LivePipeline(..., field=, nav=, objects=, tracks=, rollout=) over three frames: run()['rollout'] has the bits of plan_rollouts called
    alone on the run's own field, cost-to-go, tracks and pose, and everything else, the keys included, equals a pipeline built without
    rollout=."""
    from camradepth_amd import bev, rollout
    from camradepth_amd import lib as L
    from camradepth_amd.live import LivePipeline
    from tests.occupancy_cases import pose as pose_of
    from tests.test_gpu_live import B, CLOUD, CUT, N_SWEEPS, S, SIZE, assert_same, flat, sensor_set, small_model
    model = small_model()
    opts = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=120.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
                occupied_at=3, free_at=1, centre=(20.0, 0.0, 0.0))
    fopts = dict(max_cells=5, sources=(2,), inscribed=2.0, scale=0.2)
    nopts = dict(goals=1, neutral=20, blocked_at=200, max_rounds=32)
    oopts = dict(sources=(1, 2), connectivity=8, min_cells=2, max_objects=64)
    topts = dict(max_tracks=32, gate=6.0, confirm_hits=2, max_misses=1)
    ropts = dict(v=(2.0, 10.0, 3), w=(0.4, 5), dt=0.25, n_poses=40, keep_out=3.0, min_status=1, accel=(20.0, 4.0), outside_blocks=False,
                 weights=dict(togo=1, max_cost=2, sum_cost=1, slow=3, turn=4), tables=True, xy=True)
    stages = dict(cloud=CLOUD, occupancy=opts, field=fopts, nav=nopts, objects=oopts, tracks=topts)
    with pytest.raises(L.CrdError, match="rollout= needs field="):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, rollout=ropts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, rollout=ropts, **stages)
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, **stages)
    M = live.occupancy_map.M
    assert live.rollout_spec.cell == 2.0 and live.rollout_spec.K == 15 and plain.rollout_spec is None and live.rollout_twist.tolist() == [[0.0, 0.0]] * M
    with pytest.raises(L.CrdError, match="twist"):
        plain.run(twist=torch.zeros(M, 2, dtype=torch.float64, device="cuda"), **sensor_set(11, (350, 250)))
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)
    out_from_cam = out_from_cam.cuda()
    spec = rollout.RolloutSpec(cell=2.0, **{k: v for k, v in ropts.items() if k not in ("tables", "xy")})
    names = rollout_ref.OUT + rollout_ref.TABLES + ("xy",)
    views, picked = [], 0
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = cuda(np.stack([pose_of(3.0 * i, -2.5 * i, 0.2 * i)] * B))
        goals = cuda(np.tile(np.array([[[60.0 + i, 5.0]]]), (M, 1, 1)))
        twist = None if i == 0 else cuda(np.tile(np.array([[5.0 + i, 0.1 * i]]), (M, 1)))
        res = live.run(map_from_out=pose, goals=goals, twist=twist, **c)
        assert "rollout" in res and set(res["rollout"]) == set(names)
        views.append({k: v.data_ptr() for k, v in res["rollout"].items()})
        got = {k: v.clone() for k, v in res["rollout"].items()}
        rest = {k: v.clone() for k, v in flat(dict((k, v) for k, v in res.items() if k != "rollout")).items()}
        field_out = {k: v.clone() for k, v in res["field"].items()}
        occ_out = {k: v.clone() for k, v in res["occupancy"].items()}
        nav_out = {k: v.clone() for k, v in res["nav"].items()}
        torch.cuda.synchronize()
        want = rollout.plan_rollouts(spec, pose[:M].contiguous(), field_out, occ_out, nav_result=nav_out, tracks=live.object_tracks,
                                     twist=live.rollout_twist, tables=True, xy=True)
        for k in names:
            same(got[k], want[k], f"frame {i}: rollout {k}")
        picked += int((got["best"] >= 0).sum())
        other = plain.run(map_from_out=pose, goals=goals, **c)
        assert set(other) == set(res) - {"rollout"}
        assert_same(rest, {k: v.clone() for k, v in flat(other).items()}, f"frame {i}: with and without rollout=")
        for stage, mine in (("field", field_out), ("occupancy", occ_out), ("nav", nav_out), ("tracks", res["tracks"]), ("objects", res["objects"])):
            for k, v in mine.items():
                same(v, other[stage][k], f"frame {i}: {stage}.{k} with and without rollout=")
    assert picked > 0 and views[0] == views[1] == views[2]
    # the frames as the cameras of one rig, one map for all: the vehicle's pose is frame 0's
    del live, plain
    rig = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=dict(opts, M=1), field=fopts,
                       rollout=dict(ropts, accel=None))
    assert rig.occupancy_map.M == 1 and B > 1 and rig.rollout_twist is None
    spec = rollout.RolloutSpec(cell=2.0, **{k: v for k, v in dict(ropts, accel=None).items() if k not in ("tables", "xy")})
    pose = cuda(np.stack([pose_of(3.0, -2.5, 0.2)] + [pose_of(-4.0 - b, 6.0, -0.5) for b in range(1, B)]))
    res = rig.run(map_from_out=pose, **dict(sensor_set(12, (200, 320)), out_from_cam=out_from_cam))
    got = {k: v.clone() for k, v in res["rollout"].items()}
    torch.cuda.synchronize()
    assert got["best"].shape == (1,) and got["xy"].shape == (1, 15, 40, 2)
    want = rollout.plan_rollouts(spec, pose[:1].contiguous(), res["field"], res["occupancy"], tables=True, xy=True)
    for k in names:
        same(got[k], want[k], f"one map for {B} frames: rollout {k}")
    other = rollout.plan_rollouts(spec, pose[1:2].contiguous(), res["field"], res["occupancy"], tables=True, xy=True)
    assert not torch.equal(other["xy"], got["xy"])
