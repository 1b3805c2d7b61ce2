"""CPU: the C ABI of the scan matcher without a GPU.  crd_match_scan is declared, exported and bound with the same argument count; it
refuses every bad argument the header lists before any GPU call, with the documented status and a crd_last_error text that names the
entry and the argument; the workspace formula of the binding equals the restatement's; the Python interface refuses host tensors, bad
numbers, workspaces of another shape, unknown option names and match= without occupancy=."""
import ctypes
import math
import os
import re

import pytest

from tests import match_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "crd_match_scan"
ORDER = ("xyz", "valid", "frame_offsets", "rows_per_frame", "B", "n_rows", "map_from_points", "t_stride", "sensor", "sensor_stride", "M", "nx", "ny",
         "cell", "max_range", "z_lo", "z_hi", "min_points", "map", "cur_origin", "initialised", "n_xy", "n_theta", "rot", "min_cells", "min_score",
         "workspace", "workspace_bytes", "pose", "pick", "score", "prior_score", "n_cells", "status", "scores")
BITS = ("cell", "max_range", "z_lo", "z_hi")
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
    assert len(args.split(",")) == len(built._SIGS[ENTRY]) == len(ORDER) + 1 == 36
    assert not [a for a in args.split(",") if "double" in a and "*" not in a]                  # fp64 through memory or as bit patterns
    assert built._SIGS[ENTRY].count("L") == len(BITS) == len([a for a in args.split(",") if "_f64_bits" in a])
    assert L.crd_version() == 13 and built.ABI_VERSION == 13                                   # no struct, no changed signature
    assert re.search(r"#define\s+CRD_ABI_VERSION\s+13\b", h)


def test_match_scan_refuses_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    need = match_ref.workspace_bytes(3, 3, 40, 36, 4, 5)
    base = dict(xyz=a, valid=None, frame_offsets=a, rows_per_frame=0, B=3, n_rows=100, map_from_points=a, t_stride=12, sensor=a, sensor_stride=3,
                M=3, nx=40, ny=36, cell=0.5, max_range=12.0, z_lo=0.25, z_hi=2.0, min_points=2, map=a, cur_origin=a, initialised=a, n_xy=4,
                n_theta=5, rot=a, min_cells=8, min_score=1, workspace=a, workspace_bytes=need, pose=a, pick=a, score=a, prior_score=a, n_cells=a,
                status=a, scores=a)
    assert set(base) == set(ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, ENTRY)(*[built.f64_bits(v[k]) if k in BITS else v[k] for k in ORDER], None)

    required = ("workspace", "map", "cur_origin", "initialised", "rot", "pose", "pick", "score", "prior_score", "n_cells", "status", "xyz")
    refusals = [(dict({k: None}), b"null") for k in required]
    four, two = ("xyz", "frame_offsets", "initialised", "pick", "n_cells", "status"), ("map",)
    eight = ("map_from_points", "sensor", "cur_origin", "rot", "pose", "score", "prior_score", "scores")
    refusals += [(dict({k: a + 2}), k.encode()) for k in four] + [(dict({k: a + 1}), k.encode()) for k in two]
    refusals += [(dict({k: a + 4}), k.encode()) for k in eight] + [(dict(workspace=a + 8), b"16-byte aligned")]
    refusals += [
        (dict(B=0, M=0), b"B 0"), (dict(B=65536, M=1), b"B 65536"), (dict(n_rows=-1), b"n_rows -1"), (dict(M=2), b"M 2"), (dict(M=0), b"M 0"),
        (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=65536), b"ny 65536"),
        (dict(B=1, M=1, nx=65535, ny=65535, workspace_bytes=2 ** 62), b"cells"),
        (dict(n_xy=-1), b"n_xy -1"), (dict(n_xy=17), b"n_xy 17"), (dict(n_theta=-1), b"n_theta -1"), (dict(n_theta=33), b"n_theta 33"),
        (dict(B=1, M=1, nx=8000, ny=8000, n_theta=32, workspace_bytes=2 ** 62), b"counts"),
        (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=INF), b"cell"), (dict(cell=NAN), b"cell"),
        (dict(max_range=0.0), b"max_range"), (dict(max_range=-1.0), b"max_range"), (dict(max_range=1e200), b"max_range"), (dict(max_range=NAN), b"max_range"),
        (dict(z_lo=NAN), b"z_lo"), (dict(z_hi=NAN), b"z_hi"), (dict(z_lo=2.5), b"z_lo"),
        (dict(t_stride=3), b"t_stride 3"), (dict(sensor_stride=12), b"sensor_stride 12"),
        (dict(rows_per_frame=5), b"rows_per_frame 5"), (dict(frame_offsets=None), b"frame_offsets NULL"), (dict(frame_offsets=None, rows_per_frame=-3), b"rows_per_frame -3"),
        (dict(min_points=0), b"min_points 0"), (dict(min_cells=-1), b"min_cells -1"),
        (dict(workspace_bytes=need - 1), b"workspace holds"), (dict(workspace_bytes=0), b"workspace holds"), (dict(n_xy=5), b"workspace holds"),
        (dict(n_theta=6), b"workspace holds")]
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and ENTRY.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, ENTRY)


def test_the_workspace_formula_equals_the_restatements(built):
    from camradepth_amd import match
    for args in ((1, 1, 1, 1, 0, 0), (3, 3, 40, 36, 4, 5), (3, 1, 37, 53, 16, 2), (8, 8, 400, 400, 16, 32), (2, 2, 65, 64, 0, 32), (5, 1, 7, 5, 3, 0)):
        assert match.workspace_bytes(*args) == match_ref.workspace_bytes(*args) and match.workspace_bytes(*args) % 16 == 0, args
    assert match_ref.workspace_bytes(8, 8, 400, 400, 16, 32) == 96 * 8 * 65 + 192 + 4 * 8 * 65 * 432 * 432 + 8 * 8 * 65 * 33 * 33


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import match, occupancy
    from camradepth_amd.live import MATCH_OPTIONS, LivePipeline
    spec = match.MatchSpec(device="cpu")
    assert (spec.n_xy, spec.n_theta, spec.d_theta, spec.min_points, spec.min_cells, spec.min_score) == (4, 4, math.radians(0.25), None, 8, 1)
    assert match.SPEC_OPTIONS == dict(n_xy=4, n_theta=4, d_theta=math.radians(0.25), min_points=None, min_cells=8, min_score=1)
    assert MATCH_OPTIONS is match.SPEC_OPTIONS
    assert (match.UNINITIALISED, match.NOT_FINITE, match.FEW_CELLS, match.LOW_SCORE, match.ON_BORDER, match.KEEPS_PRIOR) == (1, 2, 4, 8, 16, 15)
    assert tuple(spec.rot.shape) == (9, 2) and spec.rot.dtype == torch.float64 and spec.rot[4].tolist() == [1.0, 0.0]
    assert spec.rot.numpy().tobytes() == match_ref.rot_table(4, math.radians(0.25)).tobytes()                # math.cos and math.sin, row by row
    wide = match.MatchSpec(n_xy=16, n_theta=32, d_theta=0.01, min_points=3, min_cells=0, min_score=-2 ** 63, device="cpu")
    assert wide.table_shape(2) == (2, 65, 33, 33) and tuple(match.MatchSpec(n_xy=0, n_theta=0, device="cpu").rot.shape) == (1, 2)
    for kw, word in ((dict(n_xy=-1), "n_xy"), (dict(n_xy=17), "n_xy"), (dict(n_xy=2.5), "n_xy"), (dict(n_xy=True), "n_xy"), (dict(n_theta=-1), "n_theta"),
                     (dict(n_theta=33), "n_theta"), (dict(d_theta=0.0), "d_theta"), (dict(d_theta=-0.1), "d_theta"), (dict(d_theta=NAN), "d_theta"),
                     (dict(d_theta=INF), "d_theta"), (dict(d_theta="x"), "d_theta"), (dict(n_theta=32, d_theta=0.1), "d_theta"),
                     (dict(min_points=0), "min_points"), (dict(min_points=1.5), "min_points"), (dict(min_cells=-1), "min_cells"),
                     (dict(min_cells=None), "min_cells"), (dict(min_score=2 ** 63), "min_score"), (dict(min_score=0.5), "min_score")):
        with pytest.raises(built.CrdError, match=word):
            match.MatchSpec(device="cpu", **kw)
    omap = occupancy.OccupancyMap(2, 9, 7, 0.5, device="cpu")
    ws = match.MatchWorkspace(omap, spec, 2, scores=True)
    assert ws.buf.numel() == match_ref.workspace_bytes(2, 2, 9, 7, 4, 4)
    assert {k: (tuple(v.shape), v.dtype) for k, v in ws.out.items()} == {
        "pose": ((2, 3, 4), torch.float64), "pick": ((2, 3), torch.int32), "score": ((2,), torch.int64), "prior_score": ((2,), torch.int64),
        "n_cells": ((2,), torch.int32), "status": ((2,), torch.int32), "scores": ((2, 9, 9, 9), torch.int64)}
    assert "scores" not in match.MatchWorkspace(omap, spec, 2).out
    for bad in (dict(B=3), dict(B=0), dict(omap=None), dict(spec=None)):
        with pytest.raises(built.CrdError, match="MatchWorkspace"):
            match.MatchWorkspace(**dict(dict(omap=omap, spec=spec, B=2), **bad))
    xyz, off = torch.zeros(10, 3), torch.tensor([0, 5, 10], dtype=torch.int32)
    with pytest.raises(built.CrdError, match="cuda"):                             # host tensors
        match.match_scan(omap, spec, xyz, frame_offsets=off)
    with pytest.raises(built.CrdError, match="OccupancyMap"):
        match.match_scan(None, spec, xyz, frame_offsets=off)
    with pytest.raises(built.CrdError, match="MatchSpec"):
        match.match_scan(omap, None, xyz, frame_offsets=off)
    with pytest.raises(built.CrdError, match="match= needs occupancy="):
        LivePipeline(None, 2, cloud={}, match={})                                 # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="match="):
        LivePipeline(None, 2, cloud={}, occupancy={}, match=dict(n_xz=4))
    with pytest.raises(built.CrdError, match="match="):
        LivePipeline(None, 2, cloud={}, occupancy={}, match=[4])
