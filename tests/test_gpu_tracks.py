"""GPU: camradepth_amd.tracks -- the object tables of map_objects followed over the frames with ids that stay -- against
tests/tracks_ref.py, the Python restatement of include/camradepth_hip.h (itself held to a sorted greedy loop and to scipy in
tests/test_tracks_ref_cpu.py).  Every state tensor and output is compared bit for bit with torch.equal after every frame, fp64
through an int64 view, so a NaN is compared by its bit pattern."""
import numpy as np
import pytest
import torch

from tests import tracks_cases, tracks_ref

pytestmark = pytest.mark.gpu

CASES = tracks_cases.all_cases()
_WANT = {}
SENTINEL = 7
TABLE = ("objects", "centre", "info")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def want_of(name):
    """The restatement's states and outputs of case `name`, frame by frame, computed once and left unchanged."""
    if name not in _WANT:
        _WANT[name] = tracks_ref.run_case(CASES[name])
    return _WANT[name]


def same(a, b, what):
    b = cuda(b) if isinstance(b, np.ndarray) else b
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    assert torch.equal(a, b), f"{what} differs in {int((a != b).sum())} of {a.numel()} values, first at {(a != b).nonzero()[:3].tolist()}"


def assert_frame(got, state, out, what):
    assert set(got) == set(tracks_ref.STATE) | set(tracks_ref.OUT), (what, sorted(got))
    assert bool((got["info"][:, 7] == 0).all()), f"{what}: the guard is raised: {got['info'].tolist()}"
    for k in tracks_ref.OUT:
        same(got[k], out[k], f"{what}: {k}")
    for k in tracks_ref.STATE:
        same(got[k], state[k], f"{what}: {k}")


def made(c):
    from camradepth_amd import tracks
    spec = tracks.TrackSpec(**c["spec"])
    held = tracks.ObjectTracks(spec, c["M"], c["nx"], c["ny"], c["cell"])
    return spec, held, tracks.TrackWorkspace(spec, held, c["N"])


def run_eager(c, workspace=True):
    """The frames of a case one call each -> per frame every returned tensor, cloned."""
    from camradepth_amd import tracks
    spec, held, ws = made(c)
    frames = []
    for f in c["frames"]:
        if f["reset"]:
            held.reset()
        for t in ws.out.values():
            t.fill_(SENTINEL)
        table = {k: cuda(f[k]) for k in TABLE}
        got = tracks.track_objects(spec, held, table, cuda(f["origin"]), workspace=ws if workspace else None)
        if workspace:
            assert all(got[k].data_ptr() == ws.out[k].data_ptr() for k in tracks_ref.OUT)
        assert all(got[k].data_ptr() == getattr(held, k).data_ptr() for k in tracks_ref.STATE)      # the state: views, updated in place
        frames.append({k: v.clone() for k, v in got.items()})
    return frames


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equality_with_the_restatement(name):
    """After every frame: every state tensor and every output, the outputs written into buffers full of a sentinel."""
    for i, (got, (state, out)) in enumerate(zip(run_eager(CASES[name]), want_of(name))):
        assert_frame(got, state, out, f"{name}, frame {i}")


def test_two_runs_give_identical_bits():
    name = "a crowd on a lattice, two maps"
    first, again = run_eager(CASES[name]), run_eager(CASES[name], workspace=False)
    for i, (a, b) in enumerate(zip(first, again)):
        for k in a:
            same(a[k], b[k], f"{name}, frame {i}, second run without workspace=: {k}")


def test_capture_on_a_side_stream():
    """track_objects with its workspace, captured once; the table and the origin changed in place and the graph replayed per frame: the
    calls made one by one.  A call allocates nothing."""
    from camradepth_amd import tracks
    name = "a crowd on a lattice, two maps"
    c, want = CASES[name], want_of(name)
    spec, held, ws = made(c)
    first = c["frames"][0]
    table, origin = {k: cuda(first[k]) for k in TABLE}, cuda(first["origin"])

    def call():
        return tracks.track_objects(spec, held, table, origin, workspace=ws)

    call()                                                                     # eager: also loads the code object
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                  # captures on a side stream
        got = call()
    reset = torch.cuda.CUDAGraph()
    with torch.cuda.graph(reset):                                              # fills only
        held.reset()
    reset.replay()
    for i, f in enumerate(c["frames"]):
        for k in TABLE:
            table[k].copy_(cuda(f[k]))
        origin.copy_(cuda(f["origin"]))
        for t in ws.out.values():
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert_frame(got, *want[i], f"replay {i}")
    assert int(want[-1][0]["next_id"].sum()) > 40


def blob_state(origin, blobs, nx=33, ny=65):
    """uint8 [1,nx,ny]: FREE, OCCUPIED on the world cells of the blobs (i0, i1, j0, j1, inclusive) seen from the origin."""
    from camradepth_amd.occupancy import FREE, OCCUPIED
    state = np.full((1, nx, ny), FREE, np.uint8)
    for i0, i1, j0, j1 in blobs:
        state[0, i0 - origin[0]:i1 + 1 - origin[0], j0 - origin[1]:j1 + 1 - origin[1]] = OCCUPIED
    return state


def test_end_to_end_through_map_objects():
    """Two blobs on a 33 x 65 state, one shifted a cell per frame, the origin moved once: both keep their ids, the moving one's velocity
    has the right sign, and the tracks equal the restatement fed with the device's own tables."""
    from camradepth_amd import objects, tracks
    cell = 0.5
    ospec, spec = objects.ObjectSpec(cell, max_objects=16), tracks.TrackSpec(max_tracks=8, confirm_hits=3)
    held = tracks.ObjectTracks(spec, 1, 33, 65, cell)
    ref_state = tracks_ref.new_state(1, 8)
    vel = None
    for s in range(6):
        origin = np.array([[100, -50]] if s < 3 else [[101, -52]], np.int64)
        still, moving = (110, 112, -40, -37), (120, 121, -20 + s, -18 + s)
        state = cuda(blob_state(origin[0], (still, moving)))
        table = objects.map_objects(ospec, state, cuda(origin))
        got = tracks.track_objects(spec, held, table, cuda(origin))
        assert table["info"][0].tolist() == [2, 0, 0, 0]
        assert got["id_of"][0, :3].tolist() == [0, 1, -1] and got["track_of"][0, :3].tolist() == [0, 1, -1]
        assert got["info"][0].tolist() == [2, 0 if s == 0 else 2, 2 if s == 0 else 0, 0, 0, 0, 1 if s == 0 else 2, 0]
        assert got["box"][0, :2].tolist() == [[110, 112, -40, -37], [120, 121, -20 + s, -18 + s]]          # world cells, whatever the origin
        assert got["tracks"][0, :2, :4].tolist() == [[2 if s >= 2 else 1, s + 1, s + 1, 0]] * 2
        out = tracks_ref.track_objects(ref_state, table["objects"].cpu().numpy(), table["centre"].cpu().numpy(), table["info"].cpu().numpy(), origin, 33,
                                       65, cell, spec.gate, spec.alpha, spec.beta, spec.confirm_hits, spec.max_misses)
        assert_frame(got, ref_state, out, f"frame {s}")
        vel = got["vel"][0, :2].tolist()
    assert vel[0] == [0.0, 0.0] and vel[1][0] == 0.0 and vel[1][1] == 0.54541015625      # towards +j; 0.5 m per frame, which the filter overshoots at first


def test_live_pipeline_with_tracks():
    """LivePipeline(cloud=, occupancy=, objects=, tracks=) over three frames: run()['tracks'] has the bits of track_objects called alone,
    frame after frame, on the run's own object table and origin, and everything else equals a pipeline built without tracks=."""
    from camradepth_amd import bev, tracks
    from camradepth_amd import lib as L
    from camradepth_amd.live import LivePipeline
    from tests.occupancy_cases import pose as pose_of
    from tests.test_gpu_live import B, CLOUD, CUT, N_SWEEPS, S, SIZE, assert_same, flat, sensor_set, small_model
    model = small_model()
    opts = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=120.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
                occupied_at=3, free_at=1, centre=(20.0, 0.0, 0.0))
    oopts = dict(sources=(1, 2), connectivity=8, min_cells=2, max_objects=64)     # as the objects' live test
    topts = dict(max_tracks=32, gate=6.0, confirm_hits=2, max_misses=1)
    with pytest.raises(L.CrdError, match="tracks= needs objects="):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, tracks=topts)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, objects=oopts, tracks=topts)
    plain = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, occupancy=opts, objects=oopts)
    assert live.track_spec.max_tracks == 32 and live.object_tracks.cell == 2.0 and plain.track_spec is None and plain.object_tracks is None
    assert not bool(live.object_tracks.next_id.any()) and bool((live.object_tracks.ids == -1).all())      # the warm-up pass left nothing
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)
    out_from_cam = out_from_cam.cuda()
    spec = tracks.TrackSpec(**topts)
    alone = tracks.ObjectTracks(spec, live.occupancy_map.M, 64, 48, 2.0)
    views, born, matched = [], 0, 0
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = None if i == 0 else cuda(pose_of(3.0 * i, -2.5 * i, 0.2 * i))
        res = live.run(map_from_out=pose, **c)
        assert "tracks" in res and set(res["tracks"]) == set(tracks_ref.STATE) | set(tracks_ref.OUT)
        views.append({k: v.data_ptr() for k, v in res["tracks"].items()})
        got_tracks = {k: v.clone() for k, v in res["tracks"].items()}
        table = {k: v.clone() for k, v in res["objects"].items()}
        origin = res["occupancy"]["origin"].clone()
        got = {k: v.clone() for k, v in flat(dict((k, v) for k, v in res.items() if k != "tracks")).items()}
        torch.cuda.synchronize()
        other = plain.run(map_from_out=pose, **c)
        assert "tracks" not in other
        assert_same(got, {k: v.clone() for k, v in flat(other).items()}, f"frame {i}: with and without tracks=")
        for k, v in table.items():
            same(v, other["objects"][k], f"frame {i}: objects.{k} with and without tracks=")
        same(origin, other["occupancy"]["origin"], f"frame {i}: the origin with and without tracks=")
        want = tracks.track_objects(spec, alone, table, origin)
        assert bool((got_tracks["info"][:, 7] == 0).all())
        for k in want:
            same(got_tracks[k], want[k], f"frame {i}: {k}")
        born, matched = born + int(want["info"][:, 2].sum()), matched + int(want["info"][:, 1].sum())
    assert born > 0 and matched > 0 and views[0] == views[1] == views[2]
