"""GPU: camradepth_amd.terrain -- point clouds fused into a rolling ground-height map with a traversability state -- against
tests/terrain_ref.py, the NumPy restatement of include/camradepth_hip.h (itself checked against plain loops and a world-cell
dictionary in tests/test_terrain_ref_cpu.py).  Everything is compared bit for bit with torch.equal (fp32 through its bits, because of
NaN): the ten outputs of every call of a sequence, lo, hi and n in the workspace, and the map's own state."""
import numpy as np
import pytest
import torch

from tests import field_ref, occupancy_cases, terrain_cases, terrain_ref

pytestmark = pytest.mark.gpu

CASES = terrain_cases.all_cases()
OUT = terrain_ref.OUT
_WANT = {}
SENTINEL = 7


def cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def want_of(name):
    """The restatement's results of every call of case `name` and its state at the end, computed once and left unchanged."""
    if name not in _WANT:
        case = CASES[name]
        state = terrain_ref.new_state(case["params"])
        _WANT[name] = ([terrain_ref.update(case["params"], state, B=case["B"], **f) for f in case["frames"]], state)
    return _WANT[name]


def new_map(params):
    from camradepth_amd import terrain
    return terrain.TerrainMap(**params)


def feed(tmap, case, frame, **kw):
    """terrain.update with one frame of a case, through the input form the case has."""
    from camradepth_amd import terrain
    B = case["B"]
    pose = dict(map_from_points=cuda(frame["T"]), sensor=cuda(frame["sensor"]), centre=cuda(frame["centre"]))
    xyz, valid = cuda(frame["xyz"]), cuda(frame.get("valid"))
    if case["form"] == "organised":
        rows = frame["rows_per_frame"]
        return terrain.update(tmap, {"points": xyz.view(B, 1, rows, 3), "valid": valid.view(B, 1, rows)}, **pose, **kw)
    if case["form"] == "bare":
        return terrain.update(tmap, xyz, cuda(frame["frame_offsets"]), valid=valid, **pose, **kw)
    return terrain.update(tmap, {"xyz": xyz, "frame_offsets": cuda(frame["frame_offsets"])}, valid=valid, **pose, **kw)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def assert_outputs(got, want, what):
    assert set(got) == set(OUT), (what, sorted(got))
    for k in OUT:
        a, b = got[k], cuda(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        a, b = bits(a), bits(b)
        assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def tables(ws, p):
    """lo, hi and n as the last call left them in the workspace (the header's layout)."""
    cells = 4 * p["M"] * p["nx"] * p["ny"]
    part = (cells + 15) & ~15
    return {k: ws.cells[i * part:i * part + cells].view(torch.int32).view(p["M"], p["nx"], p["ny"]) for i, k in enumerate(("lo", "hi", "n"))}


def assert_state(tmap, state, what):
    for k, t in (("ground", tmap.ground), ("top", tmap.top), ("weight", tmap.weight), ("prev_origin", tmap.prev_origin),
                 ("cur_origin", tmap.cur_origin), ("initialised", tmap.initialised), ("status", tmap.status_word)):
        assert torch.equal(t, cuda(state[k])), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """Every call of the sequence: the ten outputs, lo, hi and n behind them, and after each call the three state tensors as the
    torus; then the origins and the status."""
    from camradepth_amd import terrain
    case = CASES[name]
    p = case["params"]
    want, final = want_of(name)
    state = terrain_ref.new_state(p)
    tmap = new_map(p)
    ws = terrain.TerrainWorkspace(tmap, case["B"])
    assert ws.cells.numel() == terrain_ref.workspace_bytes(case["B"], tmap.M, tmap.nx, tmap.ny)
    for step, frame in enumerate(case["frames"]):
        terrain_ref.update(p, state, B=case["B"], **frame)                  # the torus after this call
        for t in ws.out.values():
            t.fill_(SENTINEL)
        got = feed(tmap, case, frame, workspace=ws, out=ws.out)
        assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in OUT)
        assert_outputs(got, want[step], f"{name}, call {step}")
        for k, t in tables(ws, p).items():
            assert torch.equal(t, cuda(want[step][k])), (name, step, k)
        assert_state(tmap, state, f"{name}, call {step}")
    assert_state(tmap, final, name)
    assert tmap.status() == final["status"].tolist()


def test_a_pose_that_is_not_finite():
    """Three maps; a NaN centre for map 1 in the third call: the others update, map 1 is left as it was with evidence 0, and status
    bit SKIPPED is set; an infinite sensor for frame 2 in the fourth: it contributes nothing, bit SENSOR_NOT_FINITE."""
    from camradepth_amd import terrain
    case = CASES["bad poses"]
    want, state = want_of("bad poses")
    tmap = new_map(case["params"])
    seen = []
    for step, frame in enumerate(case["frames"]):
        got = feed(tmap, case, frame)
        assert_outputs(got, want[step], f"call {step}")
        seen.append({k: v.clone() for k, v in got.items()})
        assert tmap.status() == [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 2], [0, 1, 2]][step]
    for k in ("ground", "top", "weight", "state", "hazard", "origin"):
        assert torch.equal(seen[2][k][1], seen[1][k][1]), k
    assert int(seen[2]["evidence"][1].sum()) == 0 and int(seen[2]["evidence"][0].sum()) > 0 and int(seen[2]["evidence"][2].sum()) > 0
    assert not torch.equal(seen[2]["weight"][0], seen[1]["weight"][0])
    assert int(seen[3]["evidence"][2].sum()) == 0 and int(seen[3]["evidence"][1].sum()) > 0
    assert (terrain.SKIPPED, terrain.SENSOR_NOT_FINITE) == (1, 2)
    assert_state(tmap, state, "bad poses")


def test_two_runs_stale_state_and_wrong_maps():
    """Runs from reset() give the same bits, the same call twice from the same state as well; garbage in the workspace, the outputs
    and the torus of a reset map does not show; a call without workspace= and out= gives the same; M maps that fit no B are refused."""
    from camradepth_amd import terrain
    from camradepth_amd import lib as L
    name = "5 x 7, one rig, compact"
    case = CASES[name]
    want, _ = want_of(name)
    tmap = new_map(case["params"])
    ws = terrain.TerrainWorkspace(tmap, case["B"])
    runs = []
    for run in range(3):
        tmap.reset()
        if run == 2:
            ws.cells.fill_(0xA5)
            tmap.ground.fill_(-12345), tmap.top.fill_(23456), tmap.weight.fill_(9)
            tmap.prev_origin.fill_(3)
            for t in ws.out.values():
                t.fill_(SENTINEL)
        kw = dict(workspace=ws, out=ws.out) if run else {}
        runs.append([{k: v.clone() for k, v in feed(tmap, case, frame, **kw).items()} for frame in case["frames"]])
    for run in runs:
        for step, got in enumerate(run):
            assert_outputs(got, want[step], f"{name}, call {step}")
    big = CASES["contention"]
    twice = []
    for _ in range(2):                                                         # the same call from the same (empty) state
        tmap2 = new_map(big["params"])
        twice.append({k: v.clone() for k, v in feed(tmap2, big, big["frames"][0]).items()})
    assert all(torch.equal(bits(twice[0][k]), bits(twice[1][k])) for k in OUT)
    two = new_map(dict(case["params"], M=2))
    with pytest.raises(L.CrdError, match="2 maps for 3 frames"):
        feed(two, case, case["frames"][0])
    with pytest.raises(L.CrdError, match="workspace"):
        feed(new_map(dict(case["params"], nx=9)), case, case["frames"][0], workspace=ws)
    with pytest.raises(L.CrdError, match="out="):
        feed(tmap, case, case["frames"][0], out={"ground": ws.out["ground"]})


def ramp_params(**kw):
    return dict(dict(M=1, nx=48, ny=24, cell=0.5), **kw)                        # everything else: the defaults of either map


def test_a_ramp_is_a_wall_to_the_occupancy_map_and_free_to_the_terrain_map():
    """The reason for the stage.  A 10 % ramp through occupancy.update with its defaults: cells beyond 3 m along it are obstacles.  The
    same cloud through terrain.update with its defaults: every observed ramp cell is FREE.  A 0.5 m box on the ramp is OCCUPIED in both."""
    from camradepth_amd import occupancy, terrain
    box = (8.0, 9.0, -0.5, 0.5, 0.5)
    xyz = terrain_cases.ramp_cloud(0.1, box=box)
    assert 5000 < len(xyz) < 8000
    cloud, off = cuda(xyz), cuda(np.array([0, len(xyz)], np.int32))
    centre = cuda(np.array([8.0, 0.0, 0.0]))
    omap, tmap = occupancy.OccupancyMap(**ramp_params()), terrain.TerrainMap(**ramp_params())
    occ, ter = occupancy.update(omap, cloud, off, centre=centre), terrain.update(tmap, cloud, off, centre=centre)
    assert torch.equal(occ["origin"], ter["origin"]) and occ["origin"].tolist() == [[16 - 24, -12]]
    ox = int(ter["origin"][0, 0])
    x_of = (torch.arange(48, device="cuda") + ox).view(48, 1).expand(48, 24) * 0.5      # the lower x of every cell
    on_ramp = (ter["evidence"][0] == 1)
    assert int(on_ramp.sum()) == 32 * 12                                        # 16 m x 6 m of 0.5 m cells
    in_box = on_ramp & (x_of >= 8.0) & (x_of < 9.0) & (torch.arange(24, device="cuda").view(1, 24) + int(ter["origin"][0, 1]) >= -1) & \
        (torch.arange(24, device="cuda").view(1, 24) + int(ter["origin"][0, 1]) < 1)
    assert int(in_box.sum()) == 4
    beyond = on_ramp & (x_of >= 3.0)
    assert (occ["evidence"][0][beyond] == occupancy.OCCUPIED).all()             # the road itself is in the obstacle band from z_lo / 10 % on
    assert (ter["state"][0][on_ramp & ~in_box] == terrain.FREE).all()          # the box leaves the ground of its cells where it was
    assert (ter["state"][0][in_box] == terrain.OCCUPIED).all() and (occ["evidence"][0][in_box] == occupancy.OCCUPIED).all()
    assert (ter["hazard"][0][in_box] == terrain.LETHAL).all() and (ter["state"][0][~on_ramp] == terrain.UNKNOWN).all()
    plain = terrain.update(terrain.TerrainMap(**ramp_params()), cuda(terrain_cases.ramp_cloud(0.1)), off, centre=centre)
    assert (plain["state"][0][plain["evidence"][0] == 1] == terrain.FREE).all() and int(plain["evidence"].sum()) == 32 * 12
    assert int(plain["slope2"].max()) == 100 and int(plain["hazard"][0][plain["evidence"][0] == 1].max()) < 64     # 2 * 0.5 * 0.1 / 0.01 = 10 quanta


def test_the_field_and_the_path_check_take_the_result_as_it_is():
    from camradepth_amd import field, terrain
    name = "40 x 36, a map per frame, compact"
    case = CASES[name]
    want, _ = want_of(name)
    tmap = new_map(case["params"])
    for frame in case["frames"][:3]:
        res = feed(tmap, case, frame)
    ref_state, ref_origin = want[2]["state"], want[2]["origin"]
    assert set(np.unique(ref_state).tolist()) == {0, 1, 2}
    R, cell = 6, case["params"]["cell"]
    spec = field.FieldSpec(cell, max_cells=R, unknown_cost=100)
    clear, cost = field_ref.tables(cell, R)
    ref = field_ref.distance_field(ref_state, 1 << terrain.OCCUPIED, R, 100, clear, cost)
    got = field.distance_field(spec, res)
    for k in ("dist2", "nearest", "clearance", "cost"):
        assert torch.equal(bits(got[k]), bits(cuda(ref[k]))), k
    rs = np.random.RandomState(4)
    K, P = 6, 9
    start = (ref_origin[rs.randint(0, 3, K)] + [[20, 18]]) * cell
    xy = start[:, None, :] + np.cumsum(rs.uniform(-0.6, 0.6, (K, P, 2)), axis=1)
    path_map = rs.randint(0, 3, K).astype(np.int32)
    n_poses = np.full(K, P, np.int32)
    ref_paths = field_ref.check_paths(xy, n_poses, path_map, ref_origin, cell, ref_state, ref["dist2"], ref["cost"], R)
    paths = field.check_paths(spec, got, res, cuda(xy), cuda(n_poses), cuda(path_map), pose_cell=True)
    for k in paths:
        assert torch.equal(paths[k], cuda(ref_paths[k])), k


def test_capture_on_a_side_stream():
    """update with a workspace, captured once; new rows, offsets and poses in the same buffers, replayed over three frames: the calls
    made one by one.  The map's state lives in its own tensors, so the replays fuse as the calls do."""
    from camradepth_amd import terrain
    rs = np.random.RandomState(90)
    B = 3
    p = terrain_cases.params(M=3, nx=16, ny=12, max_range=8.0)
    n_rows = 900
    clouds = [np.concatenate([terrain_cases.hills(rs, 300, 60, 20, 4.0) for _ in range(B)])[:n_rows] for _ in range(2)]
    assert all(len(c) == n_rows for c in clouds)
    steps = []
    for i, (x, y, heading) in enumerate(occupancy_cases.DRIVE[1:4]):
        T = np.stack([occupancy_cases.pose(x + 0.3 * b, y, heading + b, 0.125 * i) for b in range(B)])
        steps.append(dict(xyz=clouds[i % 2], frame_offsets=np.array([0, 280 + i, 600 - i, n_rows - 4], np.int32), T=T,
                          centre=np.array([[1.0, 0.25 * i, 0.0]] * B)))
    state = terrain_ref.new_state(p)
    want = [terrain_ref.update(p, state, B=B, **f) for f in steps]
    tmap = new_map(p)
    ws = terrain.TerrainWorkspace(tmap, B)
    xyz, off, T, centre = (cuda(steps[0][k]) for k in ("xyz", "frame_offsets", "T", "centre"))

    def call():
        return terrain.update(tmap, xyz, off, map_from_points=T, centre=centre, workspace=ws, out=ws.out)

    def load(f):
        xyz.copy_(cuda(f["xyz"])), off.copy_(cuda(f["frame_offsets"])), T.copy_(cuda(f["T"])), centre.copy_(cuda(f["centre"]))

    for i, f in enumerate(steps):                                              # eager, one by one: also loads the code objects
        load(f)
        assert_outputs(call(), want[i], f"eager call {i}")
    load(steps[0])
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    tmap.reset()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream, five launches in a row
        call()
    tmap.reset()                                                               # the capture runs nothing, the call before it did
    for i, f in enumerate(steps):
        load(f)
        for t in ws.out.values():
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_outputs(ws.out, want[i], f"replay {i}")
    assert_state(tmap, state, "after the replays")


def test_picture_is_colorize_of_the_ground():
    from camradepth_amd import terrain, viz
    name = "40 x 36, one rig, bare xyz"
    case = CASES[name]
    tmap = new_map(case["params"])
    for frame in case["frames"][:3]:
        res = feed(tmap, case, frame)
    got = terrain.picture(res, (-2.0, 4.0))
    assert got.dtype == torch.uint8 and got.shape == (1, 40, 36, 3)
    assert torch.equal(got, viz.colorize(res["value"], "jet", vmin=-2.0, vmax=4.0))
    known = res["weight"] > 0
    assert torch.isnan(res["value"][~known]).all() and torch.equal(res["value"][known], (res["ground"][known].double() / 64).float())
    assert (got[~known] == 0).all() and len(got.view(-1, 3).unique(dim=0)) >= 3
    canvas = torch.full((1, 40, 36, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    assert terrain.picture(res, (-1.0, 1.0), cmap="rainbow", bad_colour=(9, 8, 7), out=canvas).data_ptr() == canvas.data_ptr()
    assert torch.equal(canvas, viz.colorize(res["value"], "rainbow", vmin=-1.0, vmax=1.0, bad_colour=(9, 8, 7))) and (canvas[~known] != 0).all()
