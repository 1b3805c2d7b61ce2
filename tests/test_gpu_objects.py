"""GPU: camradepth_amd.objects -- the connected obstacle cells of a state map as a label map and an object table -- against
tests/objects_ref.py, the NumPy restatement of include/camradepth_hip.h (itself held to scipy in tests/test_objects_ref_cpu.py).
Everything is compared bit for bit with torch.equal, the centres through an int64 view."""
import numpy as np
import pytest
import torch

from tests import objects_cases, objects_ref

pytestmark = pytest.mark.gpu

CASES = objects_cases.all_cases()
OUT = ("label", "objects", "sums", "centre", "info")
_WANT = {}
SENTINEL = 7


def cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def want_of(name):
    """The restatement's outputs of case `name`, computed once and left unchanged."""
    if name not in _WANT:
        c = CASES[name]
        _WANT[name] = objects_ref.map_objects(c["state"], c["sources"], c["connectivity"], c["min_cells"], c["max_objects"], c["origin"], c["cell"])
    return _WANT[name]


def spec_of(c, **kw):
    from camradepth_amd import objects
    sources = tuple(s for s in range(8) if (c["sources"] >> s) & 1)
    return objects.ObjectSpec(c["cell"], **dict(dict(sources=sources, connectivity=c["connectivity"], min_cells=c["min_cells"],
                                                     max_objects=c["max_objects"]), **kw))


def same(a, b, what):
    b = cuda(b) if isinstance(b, np.ndarray) else b
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    assert torch.equal(a, b), f"{what} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def assert_objects(got, want, what, centre=True):
    assert set(got) == set(OUT), (what, sorted(got))
    assert bool((got["info"][:, 3] == 0).all()), f"{what}: the guard is raised: {got['info'].tolist()}"
    for k in OUT:
        if k != "centre" or centre:
            same(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """All outputs written into buffers full of a sentinel; a second run and a call without workspace= and out= give the same bits."""
    from camradepth_amd import objects
    c, want = CASES[name], want_of(name)
    spec = spec_of(c)
    state, origin = cuda(c["state"]), cuda(c["origin"])
    ws = objects.ObjectWorkspace(spec, *state.shape)
    for t in list(ws.out.values()) + [ws.buf]:
        t.fill_(SENTINEL)
    got = objects.map_objects(spec, state, origin, workspace=ws)
    assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in OUT)
    assert_objects(got, want, name)
    first = {k: v.clone() for k, v in got.items()}
    again = objects.map_objects(spec, {"state": state}, {"origin": origin}, workspace=ws, out=ws.out)
    fresh = objects.map_objects(spec, state, (state, origin))
    for k in OUT:
        same(again[k], first[k], f"{name}, second run: {k}")
        same(fresh[k], first[k], f"{name}, without workspace= and out=: {k}")
        assert fresh[k].data_ptr() != first[k].data_ptr()


def test_centre_left_out_and_arguments_refused():
    from camradepth_amd import lib as L
    from camradepth_amd import objects
    name = "three maps of 40 x 70, 4-connected"
    c, want = CASES[name], want_of(name)
    spec = spec_of(c)
    state, origin = cuda(c["state"]), cuda(c["origin"])
    ws = objects.ObjectWorkspace(spec, *state.shape)
    out = dict(ws.out, centre=None)
    for k in OUT:
        if out[k] is not None:
            out[k].fill_(SENTINEL)
    got = objects.map_objects(spec, state, origin, workspace=ws, out=out)                  # NULL for the kernels: no centre launch
    assert got["centre"] is None
    assert_objects(got, want, "without centre", centre=False)
    with pytest.raises(L.CrdError, match="label"):
        objects.map_objects(spec, state, origin, out=dict(out, label=None))
    with pytest.raises(L.CrdError, match="exactly"):
        objects.map_objects(spec, state, origin, out={k: v for k, v in ws.out.items() if k != "sums"})
    with pytest.raises(L.CrdError, match="workspace"):
        objects.map_objects(spec, state[:1], origin[:1], workspace=ws)
    with pytest.raises(L.CrdError, match="workspace"):
        objects.map_objects(spec_of(c, max_objects=5), state, origin, workspace=ws)
    with pytest.raises(L.CrdError, match="origin"):
        objects.map_objects(spec, state, origin[:1])
    with pytest.raises(L.CrdError, match="state"):
        objects.map_objects(spec, state.int(), origin)


def test_the_centres_pass_check_paths():
    """The centres, as they are, through field.check_paths as one-pose paths: each lands on a cell of the window inside its object's box.
    This is the frame convention, not the mean: the centre of a concave object may lie off it."""
    from camradepth_amd import field, objects
    name = "three maps of 40 x 70, 8-connected"
    c = CASES[name]
    spec = spec_of(c)
    state, origin = cuda(c["state"]), cuda(c["origin"])
    M, nx, ny = state.shape
    got = objects.map_objects(spec, state, origin)
    rows = got["info"][:, 0].tolist()
    assert rows[0] > 10 and rows[1] == 0 and rows[2] == 1
    fspec = field.FieldSpec(c["cell"], max_cells=4)
    f = field.distance_field(fspec, state)
    N = spec.max_objects
    xy = got["centre"].reshape(M * N, 1, 2)
    path_map = torch.arange(M, dtype=torch.int32, device="cuda").repeat_interleave(N)
    checked = field.check_paths(fspec, f, (state, origin), xy, path_map=path_map, pose_cell=True)
    cells = checked["pose_cell"].view(M, N)
    table, label = got["objects"], got["label"]
    for m in range(M):
        used = cells[m, :rows[m]]
        assert bool((used >= 0).all()) and bool((cells[m, rows[m]:] == -1).all())           # NaN in unused rows: outside
        i, j = used // ny, used % ny
        t = table[m, :rows[m]]
        assert bool(((i >= t[:, 2]) & (i <= t[:, 3]) & (j >= t[:, 4]) & (j <= t[:, 5])).all())
        one = t[:, 1] == 1                                                              # an object of one cell: the centre is that cell's
        assert bool(one.any()) or m != 0
        assert torch.equal(used[one].int(), t[one, 0]) and torch.equal(label[m].view(-1)[used[one].long()], torch.nonzero(one).view(-1).int())
    assert bool((checked["n_outside"].view(M, N)[0, :rows[0]] == 0).all())


def test_capture_on_a_side_stream():
    """map_objects with its workspace, captured once; the state and the origin changed in place, replayed: the calls made one by one."""
    from camradepth_amd import objects
    name = "three maps of 40 x 70, 8-connected"
    c = CASES[name]
    spec = spec_of(c)
    steps = []
    for s in range(3):
        state_np = c["state"] if s == 0 else objects_cases.states(objects_cases.random_map(60 + s, c["state"].shape, 0.15 * (s + 1)))
        origin_np = c["origin"] + 11 * s
        steps.append((state_np, origin_np, objects_ref.map_objects(state_np, c["sources"], c["connectivity"], c["min_cells"], c["max_objects"],
                                                                   origin_np, c["cell"])))
    state, origin = cuda(c["state"]), cuda(c["origin"])
    ws = objects.ObjectWorkspace(spec, *state.shape)

    def call():
        return objects.map_objects(spec, state, origin, workspace=ws)

    call()                                                                     # eager: also loads the code objects
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    eager = {k: v.clone() for k, v in ws.out.items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream, eight launches in a row
        call()
    for s, (state_np, origin_np, want) in enumerate(steps):
        state.copy_(cuda(state_np)), origin.copy_(cuda(origin_np))
        for t in list(ws.out.values()) + [ws.buf]:
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_objects(ws.out, want, f"replay {s}")
        if s == 0:
            for k in OUT:
                same(ws.out[k], eager[k], f"replay 0 and the eager call: {k}")
    assert not np.array_equal(steps[0][2]["label"], steps[1][2]["label"]) and not np.array_equal(steps[1][2]["centre"], steps[2][2]["centre"])


def test_live_pipeline_with_map_objects():
    """LivePipeline(cloud=, occupancy=, objects=) over three frames: run()['objects'] has the bits of map_objects called alone on the
    run's own state and origin, and everything else equals a pipeline built without objects=."""
    from camradepth_amd import bev, objects
    from camradepth_amd import lib as L
    from camradepth_amd.live import LivePipeline
    from tests.occupancy_cases import pose as pose_of
    from tests.test_gpu_live import B, CLOUD, CUT, N_SWEEPS, S, SIZE, assert_same, flat, sensor_set, small_model
    model = small_model()
    opts = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=120.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
                occupied_at=3, free_at=1, centre=(20.0, 0.0, 0.0))
    oopts = dict(sources=(1, 2), connectivity=8, min_cells=2, max_objects=64)     # FREE and OCCUPIED, as the distance field's live test
    with pytest.raises(L.CrdError, match="objects= needs occupancy="):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, objects=oopts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, objects=oopts)      # no field=
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts)
    assert live.object_spec.cell == 2.0 and live.object_spec.max_objects == 64 and plain.object_spec is None
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)
    out_from_cam = out_from_cam.cuda()
    spec = objects.ObjectSpec(2.0, **oopts)
    views, found = [], 0
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = None if i == 0 else cuda(pose_of(3.0 * i, -2.5 * i, 0.2 * i))
        res = live.run(map_from_out=pose, **c)
        assert "objects" in res and set(res["objects"]) == set(OUT) and "field" not in res
        views.append({k: v.data_ptr() for k, v in res["objects"].items()})
        got_objects = {k: v.clone() for k, v in res["objects"].items()}
        occ_out = {k: v.clone() for k, v in res["occupancy"].items()}
        got = {k: v.clone() for k, v in flat(dict((k, v) for k, v in res.items() if k != "objects")).items()}
        torch.cuda.synchronize()
        other = plain.run(map_from_out=pose, **c)
        assert "objects" not in other
        assert_same(got, {k: v.clone() for k, v in flat(other).items()}, f"frame {i}: with and without objects=")
        alone = objects.map_objects(spec, occ_out, occ_out)
        assert_objects(got_objects, alone, f"frame {i}")
        found += int(alone["info"][:, :2].sum())
    assert found > 0 and views[0] == views[1] == views[2]
