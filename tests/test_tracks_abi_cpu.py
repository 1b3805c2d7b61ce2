"""CPU: the C ABI of the object tracks without a GPU.  crd_track_objects is declared, exported and bound with the same argument count; it
refuses every bad argument the header lists before any GPU call, with the documented status and a crd_last_error text that names the
entry and the argument; the Python interface refuses host tensors, bad numbers, tables of more than 1024 rows or without centres,
workspaces of another shape, unknown option names and tracks= without objects=."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "crd_track_objects"
ORDER = ("objects", "centre", "objects_info", "origin", "M", "N", "T", "nx", "ny", "cell", "gate", "alpha", "beta", "confirm_hits", "max_misses",
         "ids", "tracks", "pos", "vel", "box", "next_id", "track_of", "id_of", "info")
BITS = ("cell", "gate", "alpha", "beta")
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_the_new_symbol_is_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, h), f"{ENTRY} is not declared"
    assert hasattr(raw, ENTRY), f"{ENTRY} is not exported"
    assert ENTRY in built._SIGS and getattr(L, ENTRY).argtypes is not None, f"{ENTRY} is not bound"
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % ENTRY, h, flags=re.S).group(1)
    assert len(args.split(",")) == len(built._SIGS[ENTRY]) == len(ORDER) + 1 == 25
    assert not [a for a in args.split(",") if "double" in a and "*" not in a]                  # fp64 through memory or as bit patterns
    assert built._SIGS[ENTRY].count("L") == len(BITS) == len([a for a in args.split(",") if "_f64_bits" in a])
    assert L.crd_version() == 13 and built.ABI_VERSION == 13                                   # no struct, no changed signature
    assert re.search(r"#define\s+CRD_ABI_VERSION\s+13\b", h)


def test_track_objects_refuses_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    base = dict(objects=a, centre=a, objects_info=a, origin=a, M=3, N=64, T=32, nx=40, ny=36, cell=0.5, gate=2.0, alpha=0.5, beta=0.25,
                confirm_hits=3, max_misses=3, ids=a, tracks=a, pos=a, vel=a, box=a, next_id=a, track_of=a, id_of=a, info=a)
    assert set(base) == set(ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, ENTRY)(*[built.f64_bits(v[k]) if k in BITS else v[k] for k in ORDER], None)

    pointers = [k for k in ORDER if base[k] == a]
    four = ("objects", "objects_info", "tracks", "track_of", "info")
    assert len(pointers) == 13
    refusals = [(dict({k: None}), b"null") for k in pointers]
    refusals += [(dict({k: a + (2 if k in four else 4)}), k.encode()) for k in pointers] + [(dict(tracks=a + 1), b"aligned"), (dict(pos=a + 4), b"aligned")]
    refusals += [
        (dict(M=0), b"M 0"), (dict(M=-2), b"M -2"), (dict(N=0), b"N 0"), (dict(N=1025), b"N 1025"), (dict(N=-1), b"N -1"),
        (dict(T=0), b"T 0"), (dict(T=1025), b"T 1025"), (dict(T=-7), b"T -7"),
        (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=-4), b"ny -4"), (dict(ny=65536), b"ny 65536"),
        (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=INF), b"cell"), (dict(cell=NAN), b"cell"),
        (dict(gate=0.0), b"gate"), (dict(gate=-1.0), b"gate"), (dict(gate=INF), b"gate"), (dict(gate=NAN), b"gate"), (dict(gate=1e200), b"gate"),
        (dict(alpha=0.0), b"alpha"), (dict(alpha=-0.5), b"alpha"), (dict(alpha=1.0000001), b"alpha"), (dict(alpha=NAN), b"alpha"),
        (dict(alpha=INF), b"alpha"),
        (dict(beta=-0.25), b"beta"), (dict(beta=2.5), b"beta"), (dict(beta=NAN), b"beta"), (dict(beta=INF), b"beta"),
        (dict(confirm_hits=0), b"confirm_hits 0"), (dict(confirm_hits=-3), b"confirm_hits -3"),
        (dict(max_misses=-1), b"max_misses -1")]
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and ENTRY.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, ENTRY)


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import tracks
    from camradepth_amd.live import TRACK_OPTIONS, LivePipeline
    spec = tracks.TrackSpec()
    assert (spec.max_tracks, spec.gate, spec.alpha, spec.beta, spec.confirm_hits, spec.max_misses) == (256, 2.0, 0.5, 0.25, 3, 3)
    assert tracks.SPEC_OPTIONS == dict(max_tracks=256, gate=2.0, alpha=0.5, beta=0.25, confirm_hits=3, max_misses=3) and TRACK_OPTIONS is tracks.SPEC_OPTIONS
    assert (tracks.FREE, tracks.TENTATIVE, tracks.CONFIRMED) == (0, 1, 2)
    assert (tracks.STATUS, tracks.AGE, tracks.HITS, tracks.MISSES, tracks.OBJECT, tracks.N_CELLS, tracks.FLAGS) == tuple(range(7))
    assert (tracks.N_LIVE, tracks.N_MATCHED, tracks.N_BORN, tracks.N_MISSED_OUT, tracks.N_LEFT, tracks.N_OVERFLOW, tracks.ROUNDS, tracks.GUARD) == tuple(range(8))
    tracks.TrackSpec(max_tracks=1024, gate=1e150, alpha=1.0, beta=2.0, confirm_hits=1, max_misses=0)
    tracks.TrackSpec(max_tracks=1, beta=0.0, confirm_hits=2 ** 31 - 1, max_misses=2 ** 31 - 1)
    for kw, word in ((dict(max_tracks=0), "max_tracks"), (dict(max_tracks=1025), "max_tracks"), (dict(max_tracks=2.5), "max_tracks"),
                     (dict(max_tracks=True), "max_tracks"), (dict(gate=0.0), "gate"), (dict(gate=-2.0), "gate"), (dict(gate=INF), "gate"),
                     (dict(gate=NAN), "gate"), (dict(gate=1e200), "gate"), (dict(gate="x"), "gate"), (dict(alpha=0.0), "alpha"),
                     (dict(alpha=1.5), "alpha"), (dict(alpha=NAN), "alpha"), (dict(alpha=None), "alpha"), (dict(beta=-0.1), "beta"),
                     (dict(beta=2.1), "beta"), (dict(beta=NAN), "beta"), (dict(confirm_hits=0), "confirm_hits"), (dict(confirm_hits=1.5), "confirm_hits"),
                     (dict(confirm_hits=2 ** 31), "confirm_hits"), (dict(max_misses=-1), "max_misses"), (dict(max_misses=2 ** 31), "max_misses"),
                     (dict(max_misses=None), "max_misses")):
        with pytest.raises(built.CrdError, match=word):
            tracks.TrackSpec(**kw)
    small = tracks.TrackSpec(max_tracks=5)
    held = tracks.ObjectTracks(small, 2, 9, 7, 0.5, device="cpu")
    assert {k: (tuple(v.shape), v.dtype) for k, v in held.state().items()} == {
        "ids": ((2, 5), torch.int64), "tracks": ((2, 5, 8), torch.int32), "pos": ((2, 5, 2), torch.float64), "vel": ((2, 5, 2), torch.float64),
        "box": ((2, 5, 4), torch.int64), "next_id": ((2,), torch.int64)}
    held.ids.fill_(4), held.tracks.fill_(3), held.pos.zero_(), held.vel.zero_(), held.box.fill_(9), held.next_id.fill_(11)
    held.reset()
    assert bool((held.ids == -1).all()) and held.tracks[1, 3].tolist() == list(tracks.FREE_ROW) and bool(held.pos.isnan().all())
    assert bool(held.vel.isnan().all()) and not bool(held.box.any()) and not bool(held.next_id.any())
    assert bool((held.pos.view(torch.int64) == 0x7FF8000000000000).all())
    for bad in (dict(M=0), dict(nx=0), dict(ny=65536), dict(cell=0.0), dict(cell=NAN), dict(cell="x")):
        with pytest.raises(built.CrdError, match="cell"):
            tracks.ObjectTracks(small, **dict(dict(M=2, nx=9, ny=7, cell=0.5, device="cpu"), **bad))
    with pytest.raises(built.CrdError, match="TrackSpec"):
        tracks.ObjectTracks(None, 2, 9, 7, 0.5, device="cpu")
    ws = tracks.TrackWorkspace(small, held, 12)
    assert {k: (tuple(v.shape), v.dtype) for k, v in ws.out.items()} == {"track_of": ((2, 12), torch.int32), "id_of": ((2, 12), torch.int64),
                                                                          "info": ((2, 8), torch.int32)}
    for N in (0, 1025, 2.5):
        with pytest.raises(built.CrdError, match="N"):
            tracks.TrackWorkspace(small, held, N)
    with pytest.raises(built.CrdError, match="ObjectTracks"):
        tracks.TrackWorkspace(small, None, 12)

    def table(N, M=2, centre=True):
        return {"objects": torch.zeros(M, N, 8, dtype=torch.int32), "centre": torch.zeros(M, N, 2, dtype=torch.float64) if centre else None,
                "info": torch.zeros(M, 4, dtype=torch.int32), "label": None, "sums": None}

    origin = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(built.CrdError, match="cuda"):                             # host tensors
        tracks.track_objects(small, held, table(12), origin)
    with pytest.raises(built.CrdError, match="1 .. 1024"):
        tracks.track_objects(small, held, table(1025), origin)
    with pytest.raises(built.CrdError, match="workspace"):
        tracks.track_objects(small, held, table(11), origin, workspace=ws)
    with pytest.raises(built.CrdError, match="workspace"):
        tracks.track_objects(small, held, table(12), origin, workspace=tracks.TrackWorkspace(small, tracks.ObjectTracks(small, 3, 9, 7, 0.5, device="cpu"), 12))
    with pytest.raises(built.CrdError, match="workspace"):
        tracks.track_objects(small, held, table(12), origin, workspace=ws.out)
    with pytest.raises(built.CrdError, match="centre"):
        tracks.track_objects(small, held, table(12, centre=False), origin)
    with pytest.raises(built.CrdError, match="centre"):
        tracks.track_objects(small, held, {"objects": None, "info": None}, origin)
    with pytest.raises(built.CrdError, match="TrackSpec"):
        tracks.track_objects(None, held, table(12), origin)
    with pytest.raises(built.CrdError, match="max_tracks"):
        tracks.track_objects(tracks.TrackSpec(max_tracks=6), held, table(12), origin)
    with pytest.raises(built.CrdError, match="ObjectTracks"):
        tracks.track_objects(small, {"ids": None}, table(12), origin)
    with pytest.raises(built.CrdError, match="tracks= needs objects="):
        LivePipeline(None, 2, cloud={}, occupancy={}, tracks={})                   # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="tracks="):
        LivePipeline(None, 2, cloud={}, occupancy={}, objects={}, tracks=dict(max_track=4))
    with pytest.raises(built.CrdError, match="tracks="):
        LivePipeline(None, 2, cloud={}, occupancy={}, objects={}, tracks=[8])
