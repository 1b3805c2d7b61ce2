"""CPU: the C ABI of the distance field without a GPU.  tests/test_abi.py parses the header against the library and the binding and so
covers the new declarations; here crd_distance_field and crd_field_paths refuse every bad argument the header lists before any GPU
call, with the documented status and a crd_last_error text that names the entry and the argument, and the Python interface refuses
host tensors, bad numbers, field= without occupancy= and unknown option names."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD, PATHS = "crd_distance_field", "crd_field_paths"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_new_symbols_are_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name, n_args in ((FIELD, 16), (PATHS, 23)):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in built._SIGS and getattr(L, name).argtypes is not None, f"{name} is not bound"
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, h, flags=re.S).group(1)
        assert len(args.split(",")) == len(built._SIGS[name]) == n_args
        assert not [a for a in args.split(",") if "double" in a and "*" not in a]              # fp64 through memory or as bit patterns
    assert L.crd_version() == 13                                                               # no struct, no changed signature


F_ORDER = ("state", "M", "nx", "ny", "sources", "R", "unknown_cost", "clear_table", "cost_table", "ws", "ws_bytes", "dist2", "nearest", "clearance",
           "cost")
P_ORDER = ("xy", "n_poses", "path_map", "K", "P", "origin", "cell", "state", "dist2", "cost", "M", "nx", "ny", "R", "blocked_at", "outside_blocks",
           "first_blocked", "max_cost", "min_dist2", "n_outside", "n_unknown", "pose_cell")
SHAPE_REFUSALS = (
    (dict(M=0), b"M 0"), (dict(M=-2), b"M -2"), (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=-4), b"ny -4"),
    (dict(ny=65536), b"ny 65536"), (dict(M=1, nx=65535, ny=32769), b"cells"), (dict(M=40000, nx=1000, ny=1000), b"cells"),
    (dict(R=0), b"max_cells 0"), (dict(R=256), b"max_cells 256"), (dict(R=-1), b"max_cells -1"))


def refused(built, name, call, refusals):
    L = built.load()
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and name.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, name)


def test_distance_field_refuses_without_a_gpu(built):
    from tests import field_ref
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    base = dict(state=a, M=3, nx=40, ny=36, sources=4, R=32, unknown_cost=0, clear_table=a, cost_table=a, ws=a, ws_bytes=1 << 40, dist2=a,
                nearest=a, clearance=a, cost=a)
    assert set(base) == set(F_ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, FIELD)(*[v[k] for k in F_ORDER], None)

    need = field_ref.workspace_bytes(3, 40, 36)
    assert need == 17280
    refused(built, FIELD, call, SHAPE_REFUSALS + (
        (dict(state=None), b"null"), (dict(clear_table=None), b"null"), (dict(cost_table=None), b"null"), (dict(ws=None), b"null"),
        (dict(dist2=None), b"null"), (dict(nearest=None), b"null"),
        (dict(clear_table=a + 2), b"aligned"), (dict(dist2=a + 1), b"aligned"), (dict(nearest=a + 2), b"aligned"), (dict(clearance=a + 3), b"aligned"),
        (dict(ws=a + 8), b"aligned"), (dict(ws=a + 4), b"workspace"),
        (dict(sources=0), b"sources 0"), (dict(sources=256), b"sources 256"), (dict(sources=-4), b"sources -4"),
        (dict(unknown_cost=-1), b"unknown_cost -1"), (dict(unknown_cost=256), b"unknown_cost 256"),
        (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(M=1, nx=1, ny=1, ws_bytes=15), b"workspace"),
        (dict(M=1, nx=1, ny=5, ws_bytes=31), b"workspace")))


def test_field_paths_refuses_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15
    inf, nan = float("inf"), float("nan")
    base = dict(xy=a, n_poses=a, path_map=a, K=5, P=130, origin=a, cell=0.5, state=a, dist2=a, cost=a, M=3, nx=40, ny=36, R=32, blocked_at=253,
                outside_blocks=1, first_blocked=a, max_cost=a, min_dist2=a, n_outside=a, n_unknown=a, pose_cell=a)
    assert set(base) == set(P_ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, PATHS)(*[built.f64_bits(v[k]) if k == "cell" else v[k] for k in P_ORDER], None)

    refused(built, PATHS, call, SHAPE_REFUSALS + (
        (dict(xy=None), b"null"), (dict(origin=None), b"null"), (dict(state=None), b"null"), (dict(dist2=None), b"null"), (dict(cost=None), b"null"),
        (dict(first_blocked=None), b"null"), (dict(max_cost=None), b"null"), (dict(min_dist2=None), b"null"), (dict(n_outside=None), b"null"),
        (dict(n_unknown=None), b"null"),
        (dict(xy=a + 4), b"aligned"), (dict(origin=a + 4), b"aligned"), (dict(n_poses=a + 2), b"aligned"), (dict(path_map=a + 1), b"aligned"),
        (dict(dist2=a + 2), b"aligned"), (dict(first_blocked=a + 2), b"aligned"), (dict(min_dist2=a + 1), b"aligned"), (dict(n_outside=a + 2), b"aligned"),
        (dict(n_unknown=a + 3), b"aligned"), (dict(pose_cell=a + 2), b"aligned"),
        (dict(K=0), b"K 0"), (dict(K=-1), b"K -1"), (dict(P=0), b"P 0"), (dict(P=-7), b"P -7"),
        (dict(blocked_at=0), b"blocked_at 0"), (dict(blocked_at=256), b"blocked_at 256"), (dict(blocked_at=-1), b"blocked_at -1"),
        (dict(outside_blocks=2), b"outside_blocks 2"), (dict(outside_blocks=-1), b"outside_blocks -1"),
        (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=inf), b"cell"), (dict(cell=nan), b"cell")))


def test_python_interface_refuses_without_a_gpu(built):
    import numpy as np
    import torch
    from camradepth_amd import field
    from camradepth_amd.live import LivePipeline
    from tests import field_ref
    spec = field.FieldSpec(0.5, max_cells=4, device="cpu")              # the numbers are judged on the host; the calls then want a device
    assert spec.far == 17 and spec.source_mask == 4 and spec.sources == (field.OCCUPIED,) and spec.inflation == 2.0
    assert spec.clear_table.dtype == torch.float32 and spec.cost_table.dtype == torch.uint8 and spec.cost_table.shape == (18,)
    own = np.arange(18, dtype=np.uint8)
    assert torch.equal(field.FieldSpec(0.5, 4, cost_table=own, device="cpu").cost_table, torch.from_numpy(own))
    assert field.FieldSpec(0.5, 4, sources=(1, 2, 7), device="cpu").source_mask == 0b10000110
    state = torch.zeros(1, 5, 7, dtype=torch.uint8)
    with pytest.raises(built.CrdError, match="cuda"):
        field.distance_field(spec, state)
    with pytest.raises(built.CrdError, match="cuda"):
        field.distance_field(spec, {"state": state})
    with pytest.raises(built.CrdError, match="FieldSpec"):
        field.distance_field(None, state)
    f = {"dist2": torch.zeros(1, 5, 7, dtype=torch.int32), "cost": state}
    with pytest.raises(built.CrdError, match="cuda"):
        field.check_paths(spec, f, (state, torch.zeros(1, 2, dtype=torch.int64)), torch.zeros(2, 3, 2, dtype=torch.float64))
    with pytest.raises(built.CrdError, match="'cost'"):
        field.check_paths(spec, {"dist2": f["dist2"], "cost": None}, (state, None), None)
    with pytest.raises(built.CrdError, match="third argument"):
        field.check_paths(spec, f, state, None)
    with pytest.raises(built.CrdError, match="'clearance'"):
        field.picture({"clearance": None}, spec)
    with pytest.raises(built.CrdError, match="cuda"):
        field.picture({"clearance": torch.zeros(1, 4, 4)}, spec)
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(cell=0.0), "cell"), (dict(cell=nan), "cell"), (dict(cell=-1.0), "cell"), (dict(cell=inf), "cell"), (dict(cell="x"), "numbers"),
                     (dict(max_cells=0), "max_cells"), (dict(max_cells=256), "max_cells"), (dict(max_cells=2.5), "max_cells"),
                     (dict(inscribed=-0.1), "inscribed"), (dict(inscribed=nan), "inscribed"), (dict(inscribed=3.0), "inscribed"),
                     (dict(inflation=2.5), "inflation"), (dict(inflation=-1.0), "inflation"), (dict(inflation=inf), "inflation"),
                     (dict(inscribed=1.5, inflation=1.0), "inscribed"), (dict(scale=-1.0), "scale"), (dict(scale=nan), "scale"),
                     (dict(sources=()), "sources"), (dict(sources=(8,)), "sources"), (dict(sources=(-1,)), "sources"), (dict(sources=4), "sources"),
                     (dict(sources=(1.5,)), "sources"), (dict(unknown_cost=-1), "unknown_cost"), (dict(unknown_cost=256), "unknown_cost"),
                     (dict(unknown_cost=0.5), "unknown_cost"), (dict(cost_table=np.zeros(17, np.uint8)), "cost_table"),
                     (dict(cost_table=np.zeros(18, np.int32)), "cost_table"), (dict(cost_table=np.zeros((18, 1), np.uint8)), "cost_table")):
        with pytest.raises(built.CrdError, match=word):
            field.FieldSpec(**dict(dict(cell=0.5, max_cells=4, device="cpu"), **kw))
    for kw in (dict(inflation=2.5), dict(inscribed=-1.0), dict(scale=inf), dict(max_cells=0)):
        with pytest.raises(built.CrdError, match="tables"):
            field.tables(**dict(dict(cell=0.5, max_cells=4), **kw))
    with pytest.raises(built.CrdError, match="cells"):
        field.FieldWorkspace(spec, 1, 0, 7)
    with pytest.raises(built.CrdError, match="FieldSpec"):
        field.FieldWorkspace(None, 1, 5, 7)
    ws = field.FieldWorkspace(spec, 1, 5, 7)
    assert ws.row_near.shape == (1, 5, 7) and ws.row_near.dtype == torch.int32 and set(ws.out) == {"dist2", "nearest", "clearance", "cost"}
    assert ws.buf.numel() == field_ref.workspace_bytes(1, 5, 7) == 144 and ws.row_near.data_ptr() == ws.buf.data_ptr()
    with pytest.raises(built.CrdError, match="field= needs occupancy="):
        LivePipeline(None, 2, cloud={}, field={})                           # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="field="):
        LivePipeline(None, 2, cloud={}, occupancy={}, field=dict(radius=3))
    for shape in ((1, 1, 1), (3, 40, 36), (2, 13, 17)):                     # the header's formula
        assert field.workspace_bytes(*shape) == field_ref.workspace_bytes(*shape)
    assert field.workspace_bytes(1, 1, 1) == 16
