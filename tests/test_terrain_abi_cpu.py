"""CPU: the C ABI of the terrain map without a GPU.  tests/test_abi.py parses the header against the library and the binding and so
covers the new declaration; here crd_terrain_update refuses every bad argument the header lists before any GPU call, with the
documented status and a crd_last_error text, and the Python interface refuses host tensors, bad maps, terrain= without occupancy=
and unknown keys."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "crd_terrain_update"


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
    assert len(args.split(",")) == len(built._SIGS[NAME]) == 45
    assert not [a for a in args.split(",") if "double" in a and "*" not in a]                  # fp64 through memory or as bit patterns
    assert L.crd_version() == 13                                                               # no struct, no changed signature


ORDER = ("xyz", "valid", "off", "rows_per_frame", "B", "n", "T", "t_stride", "sensor", "s_stride", "centre", "c_stride", "M", "nx", "ny", "cell",
         "z_quantum", "z_min", "z_max", "max_range", "head_q", "min_points", "w_max", "step_max_q", "slope2_max", "map_ground", "map_top",
         "map_weight", "prev", "cur", "initialised", "status", "ws", "ws_bytes", "ground", "top", "step", "slope2", "weight", "state", "hazard",
         "evidence", "value", "origin")
AS_BITS = ("cell", "z_quantum", "z_min", "z_max", "max_range")


def test_invalid_arguments_are_reported_without_a_gpu(built):
    from tests import terrain_ref
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    inf, nan = float("inf"), float("nan")
    base = dict(xyz=a, valid=None, off=a, rows_per_frame=0, B=3, n=1000, T=None, t_stride=0, sensor=None, s_stride=0, centre=None, c_stride=0,
                M=3, nx=40, ny=36, cell=0.5, z_quantum=0.01, z_min=-50.0, z_max=50.0, max_range=80.0, head_q=250, min_points=2, w_max=15,
                step_max_q=25, slope2_max=1225, map_ground=a, map_top=a, map_weight=a, prev=a, cur=a, initialised=a, status=a, ws=a,
                ws_bytes=1 << 40, ground=a, top=a, step=a, slope2=a, weight=a, state=a, hazard=a, evidence=a, value=a, origin=a)
    assert set(base) == set(ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, NAME)(*[built.f64_bits(v[k]) if k in AS_BITS else v[k] for k in ORDER], None)

    need = terrain_ref.workspace_bytes(3, 3, 40, 36)
    assert need == 3 * 17280 + 80 + 16
    pointers = ("ws", "map_ground", "map_top", "map_weight", "prev", "cur", "initialised", "status", "ground", "top", "step", "slope2", "weight", "state",
                "hazard", "evidence", "value", "origin")
    refusals = tuple((dict([(k, None)]), b"null") for k in pointers + ("xyz",)) + (
        (dict(xyz=a + 2), b"aligned"), (dict(off=a + 2), b"aligned"), (dict(initialised=a + 2), b"aligned"), (dict(status=a + 1), b"aligned"),
        (dict(value=a + 2), b"aligned"), (dict(map_ground=a + 2), b"aligned"), (dict(map_top=a + 1), b"aligned"), (dict(ground=a + 2), b"aligned"),
        (dict(top=a + 2), b"aligned"), (dict(step=a + 1), b"aligned"), (dict(map_weight=a + 1), b"aligned"), (dict(weight=a + 1), b"aligned"),
        (dict(T=a + 4), b"aligned"), (dict(sensor=a + 4), b"aligned"), (dict(centre=a + 2), b"aligned"), (dict(prev=a + 4), b"aligned"),
        (dict(cur=a + 4), b"aligned"), (dict(origin=a + 4), b"aligned"), (dict(slope2=a + 4), b"aligned"), (dict(ws=a + 8), b"aligned"),
        (dict(B=0, M=0), b"B 0"), (dict(B=-1), b"B -1"), (dict(n=-1), b"n_rows -1"),
        (dict(M=2), b"M 2"), (dict(M=0), b"M 0"), (dict(M=4), b"M 4"), (dict(B=1, M=3), b"M 3"),
        (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=-4), b"ny -4"), (dict(ny=65536), b"ny 65536"),
        (dict(B=1, M=1, nx=65535, ny=32769), b"cells"), (dict(B=40000, M=40000, nx=1000, ny=1000), b"cells"),
        (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=inf), b"cell"), (dict(cell=nan), b"cell"),
        (dict(z_quantum=0.0), b"z_quantum"), (dict(z_quantum=-0.01), b"z_quantum"), (dict(z_quantum=inf), b"z_quantum"), (dict(z_quantum=nan), b"z_quantum"),
        (dict(z_min=1.0, z_max=-1.0), b"z_range"), (dict(z_min=nan), b"z_range"), (dict(z_max=nan), b"z_range"), (dict(z_min=-inf), b"z_range"),
        (dict(z_max=inf), b"z_range"), (dict(z_max=0.01 * 2 ** 24), b"z_range"), (dict(z_min=-0.01 * 2 ** 24), b"z_range"),
        (dict(z_quantum=1e-6), b"z_range"),
        (dict(max_range=0.0), b"max_range"), (dict(max_range=-1.0), b"max_range"), (dict(max_range=nan), b"max_range"),
        (dict(max_range=inf), b"max_range"), (dict(max_range=1e200), b"max_range"),
        (dict(t_stride=9), b"t_stride"), (dict(T=a, t_stride=3), b"t_stride"), (dict(t_stride=-12), b"t_stride"),
        (dict(s_stride=1), b"sensor_stride"), (dict(sensor=a, s_stride=12), b"sensor_stride"), (dict(c_stride=2), b"centre_stride"),
        (dict(centre=a, c_stride=-3), b"centre_stride"),
        (dict(rows_per_frame=500), b"rows_per_frame"), (dict(off=None), b"rows_per_frame"), (dict(off=None, rows_per_frame=-5), b"rows_per_frame"),
        (dict(min_points=0), b"min_points"), (dict(min_points=-2), b"min_points"),
        (dict(w_max=0), b"w_max"), (dict(w_max=32768), b"w_max"), (dict(w_max=-1), b"w_max"),
        (dict(head_q=-1), b"head_q"), (dict(head_q=2 ** 30 + 1), b"head_q"),
        (dict(step_max_q=0), b"step_max_q"), (dict(step_max_q=-3), b"step_max_q"), (dict(step_max_q=2 ** 30 + 1), b"step_max_q"),
        (dict(slope2_max=0), b"slope2_max"), (dict(slope2_max=-1), b"slope2_max"), (dict(slope2_max=2 ** 62 + 1), b"slope2_max"),
        (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
        (dict(B=1, M=1, nx=1, ny=1, ws_bytes=95), b"workspace"),
    )
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and NAME.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, NAME)


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import occupancy, terrain
    from camradepth_amd.live import LivePipeline
    from tests import terrain_ref
    tmap = terrain.TerrainMap(1, 5, 7, 0.5, device="cpu")              # the numbers are judged on the host; update() then wants a device
    assert tmap.status() == [0] and tmap.ground.shape == tmap.top.shape == tmap.weight.shape == (1, 5, 7)
    assert (tmap.ground.dtype, tmap.top.dtype, tmap.weight.dtype) == (torch.int32, torch.int32, torch.int16)
    assert (tmap.head_q, tmap.step_max_q, tmap.slope2_max) == (250, 25, 1225) == terrain_ref.thresholds(dict(terrain.MAP_OPTIONS, cell=0.5))
    zero = terrain.TerrainMap(1, 5, 7, 0.5, headroom=0.0, step_max=0.0, slope_max=0.0, device="cpu")
    assert (zero.head_q, zero.step_max_q, zero.slope2_max) == (0, 1, 1)
    xyz, off = torch.zeros(10, 3), torch.tensor([0, 10], dtype=torch.int32)
    for first, kw in ((xyz, dict(frame_offsets=off)), ({"xyz": xyz, "frame_offsets": off}, {}),
                      ({"points": torch.zeros(1, 2, 5, 3), "valid": torch.ones(1, 2, 5, dtype=torch.uint8)}, {})):
        with pytest.raises(built.CrdError, match="cuda"):
            terrain.update(tmap, first, **kw)
    with pytest.raises(built.CrdError, match="TerrainMap"):
        terrain.update(None, xyz, off)
    with pytest.raises(built.CrdError, match="TerrainMap"):
        terrain.update(occupancy.OccupancyMap(1, 5, 7, 0.5, device="cpu"), xyz, off)
    with pytest.raises(built.CrdError, match="frame_offsets"):
        terrain.update(tmap, {"xyz": xyz, "frame_offsets": off}, off)
    with pytest.raises(built.CrdError, match="dictionary"):
        terrain.update(tmap, {"xyz": xyz})
    good = dict(M=1, nx=5, ny=7, cell=0.5, device="cpu")
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(M=0), "M 0"), (dict(M=-3), "M -3"), (dict(M=1.5), "M must be an integer"), (dict(nx=0), "cells"), (dict(ny=65536), "cells"),
                     (dict(M=40000, nx=1000, ny=1000), "cells"), (dict(cell=0.0), "cell"), (dict(cell=nan), "cell"),
                     (dict(z_quantum=0.0), "z_quantum"), (dict(z_quantum=-1.0), "z_quantum"), (dict(z_quantum=nan), "z_quantum"),
                     (dict(z_range=(1.0, -1.0)), "z_range"), (dict(z_range=(nan, 1.0)), "z_range"), (dict(z_range=(-inf, 1.0)), "z_range"),
                     (dict(z_range=(0.0, 0.01 * 2 ** 24)), "z_range"), (dict(z_range=(0.0,)), "z_range"), (dict(z_range=3.0), "z_range"),
                     (dict(max_range=0.0), "max_range"), (dict(max_range=inf), "max_range"), (dict(min_points=0), "min_points"),
                     (dict(min_points=1.5), "min_points"), (dict(w_max=0), "w_max"), (dict(w_max=32768), "w_max"), (dict(w_max=2.5), "w_max"),
                     (dict(headroom=-0.1), "headroom"), (dict(headroom=inf), "headroom"), (dict(step_max=-1.0), "step_max"),
                     (dict(step_max=nan), "step_max"), (dict(slope_max=-0.5), "slope_max"), (dict(slope_max=inf), "slope_max"),
                     (dict(slope_max="x"), "slope_max")):
        with pytest.raises(built.CrdError, match=word):
            terrain.TerrainMap(**dict(good, **kw))
    with pytest.raises(built.CrdError, match="TerrainWorkspace"):
        terrain.TerrainWorkspace(terrain.TerrainMap(2, 5, 7, 0.5, device="cpu"), 3)                # two maps for three frames
    with pytest.raises(built.CrdError, match="TerrainWorkspace"):
        terrain.TerrainWorkspace(occupancy.OccupancyMap(1, 5, 7, 0.5, device="cpu"), 1)
    with pytest.raises(built.CrdError, match="update's dictionary"):
        terrain.picture({}, (-2.0, 4.0))
    with pytest.raises(built.CrdError, match="two numbers"):
        terrain.picture({"value": torch.zeros(1, 4, 4)}, 3.0)
    with pytest.raises(built.CrdError, match="cuda"):
        terrain.picture({"value": torch.zeros(1, 4, 4)}, (-2.0, 4.0))
    with pytest.raises(built.CrdError, match="terrain= needs occupancy="):
        LivePipeline(None, 2, cloud={}, terrain={})                         # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="terrain= holds"):
        LivePipeline(None, 2, cloud={}, occupancy={}, terrain=dict(colour=True))
    with pytest.raises(built.CrdError, match="terrain= holds"):
        LivePipeline(None, 2, cloud={}, occupancy={}, terrain=dict(nx=10))  # the window is the occupancy map's
    for shape in ((1, 1, 1, 1), (3, 3, 40, 36), (3, 1, 5, 7), (8, 8, 400, 400)):                   # the header's formula
        assert terrain.workspace_bytes(*shape) == terrain_ref.workspace_bytes(*shape)
    assert terrain.workspace_bytes(1, 1, 1, 1) == 96 and terrain.workspace_bytes(3, 1, 5, 7) == 3 * 144 + 80 + 16
    assert (terrain.UNKNOWN, terrain.FREE, terrain.OCCUPIED) == (occupancy.UNKNOWN, occupancy.FREE, occupancy.OCCUPIED) == (0, 1, 2)
    assert (terrain.SKIPPED, terrain.SENSOR_NOT_FINITE, terrain.NO_INFORMATION, terrain.LETHAL) == (1, 2, 255, 254)
