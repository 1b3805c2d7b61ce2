"""CPU: the C ABI of the occupancy map without a GPU.  tests/test_abi.py parses the header against the library and the binding and so
covers the new declaration; here crd_occupancy_update refuses every bad argument the header lists before any GPU call, with the
documented status and a crd_last_error text, and the Python interface refuses host tensors, bad maps and occupancy= without cloud=."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "crd_occupancy_update"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_new_symbol_is_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, h), f"{NAME} is not declared"
    assert hasattr(raw, NAME), f"{NAME} is not exported"
    assert NAME in built._SIGS and getattr(L, NAME).argtypes is not None, f"{NAME} is not bound"
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, h, flags=re.S).group(1)
    assert len(args.split(",")) == len(built._SIGS[NAME]) == 40
    assert not [a for a in args.split(",") if "double" in a and "*" not in a]                  # fp64 through memory or as bit patterns
    assert L.crd_version() == 13                                                               # no struct, no changed signature


ORDER = ("xyz", "valid", "off", "rows_per_frame", "B", "n", "T", "t_stride", "sensor", "s_stride", "centre", "c_stride", "M", "nx", "ny", "cell",
         "n_bins", "max_range", "z_floor", "z_lo", "z_hi", "min_points", "l_occ", "l_free", "l_max", "occupied_at", "free_at", "map", "prev", "cur",
         "initialised", "status", "ws", "ws_bytes", "log_odds", "state", "evidence", "value", "origin")
AS_BITS = ("cell", "max_range", "z_floor", "z_lo", "z_hi")


def test_invalid_arguments_are_reported_without_a_gpu(built):
    from tests import occupancy_ref
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    inf, nan = float("inf"), float("nan")
    base = dict(xyz=a, valid=None, off=a, rows_per_frame=0, B=3, n=1000, T=None, t_stride=0, sensor=None, s_stride=0, centre=None, c_stride=0,
                M=3, nx=40, ny=36, cell=0.5, n_bins=720, max_range=80.0, z_floor=-inf, z_lo=0.3, z_hi=2.5, min_points=2, l_occ=6, l_free=2,
                l_max=60, occupied_at=12, free_at=6, map=a, prev=a, cur=a, initialised=a, status=a, ws=a, ws_bytes=1 << 40, log_odds=a,
                state=a, evidence=a, value=a, origin=a)
    assert set(base) == set(ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, NAME)(*[built.f64_bits(v[k]) if k in AS_BITS else v[k] for k in ORDER], None)

    need = occupancy_ref.workspace_bytes(3, 720, 3, 40, 36)
    assert need == 2 * 17280 + 80 + 17280 + 16
    refusals = (
        (dict(xyz=None), b"null"), (dict(ws=None), b"null"), (dict(map=None), b"null"), (dict(prev=None), b"null"), (dict(cur=None), b"null"),
        (dict(initialised=None), b"null"), (dict(status=None), b"null"), (dict(log_odds=None), b"null"), (dict(state=None), b"null"),
        (dict(evidence=None), b"null"), (dict(origin=None), b"null"),
        (dict(xyz=a + 2), b"aligned"), (dict(off=a + 2), b"aligned"), (dict(initialised=a + 2), b"aligned"), (dict(status=a + 1), b"aligned"),
        (dict(value=a + 2), b"aligned"), (dict(map=a + 1), b"aligned"), (dict(log_odds=a + 1), b"aligned"), (dict(T=a + 4), b"aligned"),
        (dict(sensor=a + 4), b"aligned"), (dict(centre=a + 2), b"aligned"), (dict(prev=a + 4), b"aligned"), (dict(cur=a + 4), b"aligned"),
        (dict(origin=a + 4), b"aligned"), (dict(ws=a + 8), b"aligned"),
        (dict(B=0, M=0), b"B 0"), (dict(B=-1), b"B -1"), (dict(n=-1), b"n_rows -1"),
        (dict(M=2), b"M 2"), (dict(M=0), b"M 0"), (dict(M=4), b"M 4"), (dict(B=1, M=3), b"M 3"),
        (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=-4), b"ny -4"), (dict(ny=65536), b"ny 65536"),
        (dict(B=1, M=1, nx=65535, ny=32769), b"cells"), (dict(B=40000, M=40000, nx=1000, ny=1000), b"cells"),
        (dict(n_bins=0), b"n_bins"), (dict(n_bins=6), b"n_bins"), (dict(n_bins=-4), b"n_bins"), (dict(n_bins=65540), b"n_bins"), (dict(n_bins=3), b"n_bins"),
        (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=inf), b"cell"), (dict(cell=nan), b"cell"),
        (dict(max_range=0.0), b"max_range"), (dict(max_range=-1.0), b"max_range"), (dict(max_range=nan), b"max_range"),
        (dict(max_range=inf), b"max_range"), (dict(max_range=1e200), b"max_range"),
        (dict(z_floor=nan), b"z_floor"), (dict(z_lo=nan), b"z_lo"), (dict(z_hi=nan), b"z_hi"), (dict(z_lo=3.0), b"z_lo"), (dict(z_floor=1.0), b"z_floor"),
        (dict(t_stride=9), b"t_stride"), (dict(T=a, t_stride=3), b"t_stride"), (dict(t_stride=-12), b"t_stride"),
        (dict(s_stride=1), b"sensor_stride"), (dict(sensor=a, s_stride=12), b"sensor_stride"), (dict(c_stride=2), b"centre_stride"),
        (dict(centre=a, c_stride=-3), b"centre_stride"),
        (dict(rows_per_frame=500), b"rows_per_frame"), (dict(off=None), b"rows_per_frame"), (dict(off=None, rows_per_frame=-5), b"rows_per_frame"),
        (dict(min_points=0), b"min_points"), (dict(min_points=-2), b"min_points"),
        (dict(l_occ=0), b"l_occ"), (dict(l_free=0), b"l_free"), (dict(l_occ=61), b"l_occ"), (dict(l_free=61), b"l_free"), (dict(l_max=32768), b"l_max"),
        (dict(l_max=0), b"l_max"), (dict(l_occ=-1), b"l_occ"),
        (dict(occupied_at=0), b"occupied_at"), (dict(occupied_at=61), b"occupied_at"), (dict(free_at=0), b"free_at"), (dict(free_at=61), b"free_at"),
        (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
        (dict(B=1, M=1, nx=1, ny=1, n_bins=4, ws_bytes=127), b"workspace"),
    )
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and NAME.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, NAME)


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import occupancy
    from camradepth_amd.live import LivePipeline
    from tests import occupancy_ref
    omap = occupancy.OccupancyMap(1, 5, 7, 0.5, device="cpu")          # the numbers are judged on the host; update() then wants a device
    assert omap.status() == [0] and omap.log_odds.shape == (1, 5, 7) and omap.log_odds.dtype == torch.int16
    xyz, off = torch.zeros(10, 3), torch.tensor([0, 10], dtype=torch.int32)
    for first, kw in ((xyz, dict(frame_offsets=off)), ({"xyz": xyz, "frame_offsets": off}, {}),
                      ({"points": torch.zeros(1, 2, 5, 3), "valid": torch.ones(1, 2, 5, dtype=torch.uint8)}, {})):
        with pytest.raises(built.CrdError, match="cuda"):
            occupancy.update(omap, first, **kw)
    with pytest.raises(built.CrdError, match="OccupancyMap"):
        occupancy.update(None, xyz, off)
    with pytest.raises(built.CrdError, match="frame_offsets"):
        occupancy.update(omap, {"xyz": xyz, "frame_offsets": off}, off)
    with pytest.raises(built.CrdError, match="dictionary"):
        occupancy.update(omap, {"xyz": xyz})
    good = dict(M=1, nx=5, ny=7, cell=0.5, device="cpu")
    for kw, word in ((dict(M=0), "M 0"), (dict(M=-3), "M -3"), (dict(M=1.5), "M must be an integer"), (dict(nx=0), "cells"), (dict(ny=65536), "cells"),
                     (dict(M=40000, nx=1000, ny=1000), "cells"), (dict(cell=0.0), "cell"), (dict(cell=float("nan")), "cell"),
                     (dict(n_bins=0), "n_bins"), (dict(n_bins=6), "n_bins"), (dict(n_bins=65540), "n_bins"), (dict(n_bins=7.5), "n_bins"),
                     (dict(max_range=0.0), "max_range"), (dict(max_range=float("inf")), "max_range"), (dict(z_lo=3.0), "z_lo"),
                     (dict(z_floor=float("nan")), "z_floor"), (dict(min_points=0), "min_points"), (dict(min_points=1.5), "min_points"),
                     (dict(l_occ=0), "l_occ"), (dict(l_free=0), "l_free"), (dict(l_occ=61), "l_occ"), (dict(l_max=32768), "l_max"),
                     (dict(l_free=2.5), "l_free"), (dict(occupied_at=0), "occupied_at"), (dict(free_at=61), "free_at"), (dict(l_max="x"), "l_max")):
        with pytest.raises(built.CrdError, match=word):
            occupancy.OccupancyMap(**dict(good, **kw))
    with pytest.raises(built.CrdError, match="OccupancyWorkspace"):
        occupancy.OccupancyWorkspace(occupancy.OccupancyMap(2, 5, 7, 0.5, device="cpu"), 3)        # two maps for three frames
    with pytest.raises(built.CrdError, match="update's dictionary"):
        occupancy.picture({}, 60)
    with pytest.raises(built.CrdError, match="cuda"):
        occupancy.picture({"value": torch.zeros(1, 4, 4)}, omap)
    with pytest.raises(built.CrdError, match="occupancy= needs cloud="):
        LivePipeline(None, 2, occupancy={})                                 # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="occupancy="):
        LivePipeline(None, 2, cloud={}, occupancy=dict(colour=True))
    for shape in ((1, 4, 1, 1, 1), (3, 720, 3, 40, 36), (3, 8, 1, 5, 7)):  # the header's formula
        assert occupancy.workspace_bytes(*shape) == occupancy_ref.workspace_bytes(*shape)
    assert occupancy.workspace_bytes(1, 4, 1, 1, 1) == 128
    assert (occupancy.UNKNOWN, occupancy.FREE, occupancy.OCCUPIED) == (0, 1, 2)
