"""GPU: camradepth_amd.field -- the distance field of a state map and the path check -- against tests/field_ref.py, the NumPy
restatement of include/camradepth_hip.h (itself checked against brute-force loops and scipy's EDT in tests/test_field_ref_cpu.py).
Everything is compared bit for bit with torch.equal: the four outputs, launch 1's table in the workspace, and the per-path results."""
import numpy as np
import pytest
import torch

from tests import field_cases, field_ref

pytestmark = pytest.mark.gpu

CASES = dict(field_cases.all_cases(), **field_cases.tile_cases())
PATHS = field_cases.path_cases()
OUT = ("dist2", "nearest", "clearance", "cost")
PATH_OUT = ("first_blocked", "max_cost", "min_dist2", "n_outside", "n_unknown")
_WANT = {}
SENTINEL = 7


def cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def want_of(name):
    """The restatement's field of case `name`, computed once and left unchanged."""
    if name not in _WANT:
        c = CASES[name]
        clear, cost = field_ref.tables(c["cell"], c["R"], **c["table"])
        _WANT[name] = field_ref.distance_field(c["state"], c["sources"], c["R"], c["unknown_cost"], clear, cost)
    return _WANT[name]


def spec_of(c, **kw):
    from camradepth_amd import field
    states = tuple(s for s in range(8) if (c["sources"] >> s) & 1)
    return field.FieldSpec(c["cell"], **dict(dict(max_cells=c["R"], sources=states, unknown_cost=c["unknown_cost"], **c["table"]), **kw))


def same(a, b, what):
    b = cuda(b) if isinstance(b, np.ndarray) else b
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), f"{what} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def assert_field(got, want, what, keys=OUT):
    assert set(got) == set(OUT), (what, sorted(got))
    for k in keys:
        same(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """The four outputs and row_near behind them, written into a workspace full of garbage; a second run and a call without
    workspace= and out= give the same bits."""
    from camradepth_amd import field
    c = CASES[name]
    want = want_of(name)
    spec = spec_of(c)
    state = cuda(c["state"])
    ws = field.FieldWorkspace(spec, *state.shape)
    assert ws.buf.numel() == field_ref.workspace_bytes(*state.shape)
    ws.buf.fill_(0xA5)
    for t in ws.out.values():
        t.fill_(SENTINEL)
    got = field.distance_field(spec, state, workspace=ws, out=ws.out)
    assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in OUT)
    assert_field(got, want, name)
    same(ws.row_near, want["row_near"], f"{name}: row_near")
    first = {k: v.clone() for k, v in got.items()}
    again = field.distance_field(spec, {"state": state}, workspace=ws, out=ws.out)
    fresh = field.distance_field(spec, state)
    for k in OUT:
        same(again[k], first[k], f"{name}, second run: {k}")
        same(fresh[k], first[k], f"{name}, without workspace= and out=: {k}")
        assert fresh[k].data_ptr() != ws.out[k].data_ptr()


def test_outputs_left_out_unknown_cost_two_states_and_a_table_of_the_caller():
    from camradepth_amd import field
    from camradepth_amd import lib as L
    name = "two maps of 13 x 17"
    c = CASES[name]
    want = want_of(name)
    state = cuda(c["state"])
    spec = spec_of(c)
    ws = field.FieldWorkspace(spec, *state.shape)
    for left_out in (("clearance",), ("cost",), ("clearance", "cost")):                  # NULL for the kernel
        out = {k: None if k in left_out else torch.full(state.shape, SENTINEL, dtype=field.OUTPUTS[k], device="cuda") for k in OUT}
        got = field.distance_field(spec, state, workspace=ws, out=out)
        assert all(got[k] is None for k in left_out)
        assert_field(got, want, f"without {left_out}", keys=[k for k in OUT if k not in left_out])
    with pytest.raises(L.CrdError, match="dist2"):
        field.distance_field(spec, state, out=dict(out, dist2=None))
    with pytest.raises(L.CrdError, match="workspace"):
        field.distance_field(spec, state[:1], workspace=ws)
    clear, cost = field_ref.tables(c["cell"], c["R"], **c["table"])
    assert (c["state"] == 0).any() and (want["cost"][c["state"] == 0] < 90).any() and (want["cost"] > 90).any()
    for unknown_cost in (1, 90, 255):
        ref = field_ref.distance_field(c["state"], c["sources"], c["R"], unknown_cost, clear, cost)
        assert not np.array_equal(ref["cost"], want["cost"])
        assert_field(field.distance_field(spec_of(c, unknown_cost=unknown_cost), state), ref, f"unknown_cost {unknown_cost}")
    for states in ((1, 2), (0, 2), (0, 1, 2, 3, 7)):                                      # FREE and OCCUPIED, UNKNOWN and OCCUPIED, ...
        mask = sum(1 << s for s in states)
        ref = field_ref.distance_field(c["state"], mask, c["R"], 0, clear, cost)
        assert not np.array_equal(ref["dist2"], want["dist2"])
        assert_field(field.distance_field(spec_of(c, sources=states, unknown_cost=0), state), ref, f"sources {states}")
    own = (np.arange(c["R"] ** 2 + 2) * 37 % 251).astype(np.uint8)
    ref = field_ref.distance_field(c["state"], c["sources"], c["R"], c["unknown_cost"], clear, own)
    assert_field(field.distance_field(spec_of(c, cost_table=own), state), ref, "the caller's cost_table")
    assert_field(field.distance_field(spec_of(c, cost_table=cuda(own)), state), ref, "the caller's cost_table, from the device")


def path_setup():
    from camradepth_amd import field
    state = field_cases.path_map_state()
    spec = field.FieldSpec(field_cases.PATH_CELL, max_cells=field_cases.PATH_R)
    clear, cost = field_ref.tables(field_cases.PATH_CELL, field_cases.PATH_R)
    ref = field_ref.distance_field(state, 1 << field_cases.OCCUPIED, field_cases.PATH_R, 0, clear, cost)
    return spec, state, ref


def want_paths(c, state, ref, blocked_at, outside_blocks):
    return field_ref.check_paths(c["xy"], c["n_poses"], c["path_map"], field_cases.PATH_ORIGIN, field_cases.PATH_CELL, state, ref["dist2"], ref["cost"],
                                 field_cases.PATH_R, blocked_at, outside_blocks)


def test_paths_bit_equality_with_the_restatement():
    from camradepth_amd import field
    from camradepth_amd import lib as L
    spec, state, ref = path_setup()
    state_d, origin = cuda(state), cuda(field_cases.PATH_ORIGIN)
    f = field.distance_field(spec, state_d)
    assert_field(f, ref, "the map of the paths")
    for name, c in PATHS.items():
        xy, n_poses, path_map = cuda(c["xy"]), cuda(c["n_poses"]), cuda(c["path_map"])
        K, P = c["xy"].shape[:2]
        for outside_blocks, blocked_at, with_cells in ((True, 253, True), (False, 253, False), (True, 40, False), (False, 1, True)):
            want = want_paths(c, state, ref, blocked_at, outside_blocks)
            out = field.path_outputs(K, P, pose_cell=with_cells)
            for t in out.values():
                t.fill_(SENTINEL)
            got = field.check_paths(spec, f, {"state": state_d, "origin": origin}, xy, n_poses, path_map, blocked_at=blocked_at,
                                    outside_blocks=outside_blocks, pose_cell=with_cells, out=out)
            assert set(got) == set(PATH_OUT) | ({"pose_cell"} if with_cells else set())
            for k in got:
                assert got[k].data_ptr() == out[k].data_ptr()
                same(got[k], want[k], f"{name}, outside_blocks {outside_blocks}, blocked_at {blocked_at}: {k}")
        fresh = field.check_paths(spec, f, (state_d, origin), xy, n_poses, path_map, blocked_at=1, outside_blocks=False, pose_cell=True)
        for k in fresh:
            same(fresh[k], got[k], f"{name}, without out=: {k}")
    with pytest.raises(L.CrdError, match="blocked_at"):
        field.check_paths(spec, f, (state_d, origin), xy, blocked_at=0)
    with pytest.raises(L.CrdError, match="n_poses"):
        field.check_paths(spec, f, (state_d, origin), xy, n_poses=n_poses[:2])
    with pytest.raises(L.CrdError, match="origin"):
        field.check_paths(spec, f, (state_d, origin[:1]), xy)


def test_capture_of_both_entries_on_a_side_stream():
    """distance_field and check_paths with their workspaces, captured once; the state and the trajectories changed in place, replayed:
    the calls made one by one."""
    from camradepth_amd import field
    spec, state0, _ = path_setup()
    clear, cost = field_ref.tables(field_cases.PATH_CELL, field_cases.PATH_R)
    c = PATHS["5 paths of 130"]
    K, P = c["xy"].shape[:2]
    rs = np.random.RandomState(44)
    steps = []
    for i in range(3):
        state = field_cases.scatter(50 + i, state0.shape, 0.05) if i else state0
        xy = c["xy"] if i == 0 else c["xy"] + rs.uniform(-1.0, 1.0, size=c["xy"].shape)
        ref = field_ref.distance_field(state, 1 << field_cases.OCCUPIED, field_cases.PATH_R, 0, clear, cost)
        steps.append((state, xy, ref, want_paths(dict(c, xy=xy), state, ref, 253, True)))
    state, xy, origin = cuda(steps[0][0]), cuda(steps[0][1]), cuda(field_cases.PATH_ORIGIN)
    n_poses, path_map = cuda(c["n_poses"]), cuda(c["path_map"])
    ws = field.FieldWorkspace(spec, *state.shape)
    pout = field.path_outputs(K, P, pose_cell=True)

    def call():
        f = field.distance_field(spec, state, workspace=ws, out=ws.out)
        return f, field.check_paths(spec, f, (state, origin), xy, n_poses, path_map, pose_cell=True, out=pout)

    call()                                                                     # eager: also loads the code objects
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream, three launches in a row
        call()
    for i, (s, p, ref, want) in enumerate(steps):
        state.copy_(cuda(s)), xy.copy_(cuda(p))
        for t in list(ws.out.values()) + list(pout.values()) + [ws.buf]:
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_field(ws.out, ref, f"replay {i}")
        same(ws.row_near, ref["row_near"], f"replay {i}: row_near")
        for k in pout:
            same(pout[k], want[k], f"replay {i}: {k}")
    assert not np.array_equal(steps[0][2]["dist2"], steps[1][2]["dist2"]) and not np.array_equal(steps[0][3]["pose_cell"], steps[1][3]["pose_cell"])


def test_picture_is_colorize_of_the_clearance():
    from camradepth_amd import field, viz
    name = "33 x 65"
    c = CASES[name]
    spec = spec_of(c)
    res = field.distance_field(spec, cuda(c["state"]))
    got = field.picture(res, spec)
    assert got.dtype == torch.uint8 and got.shape == (1, 33, 65, 3)
    assert torch.equal(got, viz.colorize(res["clearance"], "jet", vmin=0.0, vmax=4.0))
    far = res["dist2"] == spec.far
    assert bool(far.any()) and bool((~far).any()) and bool((got[far] == 0).all()) and torch.isinf(res["clearance"][far]).all()
    canvas = torch.full((1, 33, 65, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    assert field.picture(res, spec, cmap="rainbow", out=canvas).data_ptr() == canvas.data_ptr()
    assert torch.equal(canvas, viz.colorize(res["clearance"], "rainbow", vmin=0.0, vmax=4.0)) and not torch.equal(canvas, got)


def test_live_pipeline_with_a_field():
    """LivePipeline(cloud=, occupancy=, field=) over three frames: run()['field'] has the bits of the stage called alone on the run's
    own occupancy output, and everything else equals a pipeline built without field=."""
    from camradepth_amd import field
    from camradepth_amd import lib as L
    from camradepth_amd.live import LivePipeline
    from tests.occupancy_cases import pose as pose_of
    from tests.test_gpu_live import B, CLOUD, CUT, N_SWEEPS, S, SIZE, assert_same, flat, sensor_set, small_model
    from camradepth_amd import bev
    model = small_model()
    opts = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=120.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
                occupied_at=3, free_at=1, centre=(20.0, 0.0, 0.0))
    fopts = dict(max_cells=5, sources=(1, 2), unknown_cost=30, inscribed=2.0, scale=0.2)
    K, P = 3, 70
    with pytest.raises(L.CrdError, match="occupancy"):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, field=fopts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={}, occupancy=opts,
                        field=dict(fopts, picture=True, paths=(K, P), blocked_at=100))
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={}, occupancy=opts)
    assert live.field_spec.cell == 2.0 and bool(torch.isnan(live.paths_xy).all())
    with pytest.raises(L.CrdError, match="paths"):
        plain.run(paths=torch.zeros(K, P, 2, dtype=torch.float64, device="cuda"), **sensor_set(11, (350, 250)))
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)
    out_from_cam = out_from_cam.cuda()
    spec = field.FieldSpec(2.0, **fopts)
    rs = np.random.RandomState(5)
    views = []
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = None if i == 0 else cuda(pose_of(3.0 * i, -2.5 * i, 0.2 * i))
        xy = None if i == 0 else cuda(np.stack([rs.uniform(-60.0, 100.0, (K, P)), rs.uniform(-60.0, 60.0, (K, P))], -1))
        res = live.run(map_from_out=pose, paths=xy, **c)
        assert set(res) == {"image", "x", "radar", "rad_vel", "pred", "cloud", "occupancy", "field", "pictures"}
        assert set(res["field"]) == set(OUT) | {"picture", "paths"} and set(res["field"]["paths"]) == set(PATH_OUT)
        views.append({k: v.data_ptr() for k, v in res["field"].items() if k != "paths"})
        got_field = {k: (v if k != "paths" else dict(v)) for k, v in res["field"].items()}
        got_paths = {k: v.clone() for k, v in got_field.pop("paths").items()}
        got_field = {k: v.clone() for k, v in got_field.items()}
        occ_out = {k: v.clone() for k, v in res["occupancy"].items()}
        got = {k: v.clone() for k, v in flat(res).items()}
        torch.cuda.synchronize()
        other = plain.run(map_from_out=pose, **c)
        assert "field" not in other
        assert_same(got, {k: v.clone() for k, v in flat(other).items()}, f"frame {i}: with and without field=")
        assert_same(occ_out, {k: v.clone() for k, v in other["occupancy"].items()}, f"frame {i}: the map with and without field=")
        want = field.distance_field(spec, occ_out)
        want["picture"] = field.picture(want, spec)
        for k in want:
            same(got_field[k], want[k], f"frame {i}: field {k}")
        if i == 0:                                                              # the trajectories a pipeline starts with: every pose outside
            assert got_paths["n_outside"].tolist() == [P] * K and got_paths["first_blocked"].tolist() == [0] * K
        else:
            alone = field.check_paths(spec, want, occ_out, xy, blocked_at=100)
            for k in alone:
                same(got_paths[k], alone[k], f"frame {i}: paths {k}")
            assert int(alone["n_outside"].sum()) < K * P
        assert bool((want["dist2"] != spec.far).any()) and bool((want["dist2"] == spec.far).any())
    assert views[0] == views[1] == views[2]
