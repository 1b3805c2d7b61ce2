"""CPU: the C ABI of the bird's-eye-view back end without a GPU.  tests/test_abi.py parses the header against the library and the
binding and so covers the new declaration; here crd_bev_grid refuses every bad argument the header lists before any GPU call, with
the documented status and a crd_last_error text, and the Python interface refuses host tensors, bad ranges and bev= without cloud=."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "crd_bev_grid"


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
    assert len(args.split(",")) == len(built._SIGS[NAME]) == 28
    assert not [a for a in args.split(",") if "double" in a and "*" not in a]                  # fp64 through memory or as bit patterns
    assert L.crd_version() == 13                                                               # no struct, no changed signature


def test_invalid_arguments_are_reported_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    bits = built.f64_bits
    inf, nan = float("inf"), float("nan")
    base = dict(xyz=a, valid=None, label=None, off=a, rows_per_frame=0, B=2, n=1000, T=None, t_stride=0, x_min=0.0, y_min=-40.0, cell=0.5,
                nx=160, ny=160, z_lo=-inf, z_hi=inf, min_points=1, flip_x=0, flip_y=0, ws=a, ws_bytes=1 << 40, count=a, z_max=a, z_min=a,
                top_index=a, top_label=None, occupancy=a)

    def call(**kw):
        v = dict(base, **kw)
        return L.crd_bev_grid(v["xyz"], v["valid"], v["label"], v["off"], v["rows_per_frame"], v["B"], v["n"], v["T"], v["t_stride"],
                              bits(v["x_min"]), bits(v["y_min"]), bits(v["cell"]), v["nx"], v["ny"], bits(v["z_lo"]), bits(v["z_hi"]),
                              v["min_points"], v["flip_x"], v["flip_y"], v["ws"], v["ws_bytes"], v["count"], v["z_max"], v["z_min"],
                              v["top_index"], v["top_label"], v["occupancy"], None)

    need = 2 * 8 * 51200 + 4 * 51200                     # B * nx * ny = 51,200 cells: every section is a multiple of 16 bytes already
    refusals = (
        (dict(xyz=None), b"null"), (dict(ws=None), b"null"), (dict(count=None), b"null"), (dict(z_max=None), b"null"),
        (dict(xyz=a + 2), b"aligned"), (dict(count=a + 1), b"aligned"), (dict(z_max=a + 2), b"aligned"), (dict(ws=a + 8), b"aligned"),
        (dict(off=a + 2), b"aligned"), (dict(z_min=a + 3), b"aligned"), (dict(top_index=a + 2), b"aligned"), (dict(T=a + 4), b"aligned"),
        (dict(B=0), b"B 0"), (dict(B=-1), b"B -1"), (dict(n=-1), b"n_rows -1"),
        (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=-4), b"ny -4"), (dict(ny=65536), b"ny 65536"),
        (dict(B=1, nx=65535, ny=32769), b"cells"), (dict(B=40000, nx=1000, ny=1000), b"cells"),
        (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=inf), b"cell"), (dict(cell=nan), b"cell"),
        (dict(x_min=nan), b"x_min"), (dict(y_min=inf), b"y_min"),
        (dict(z_lo=nan), b"z_lo"), (dict(z_hi=nan), b"z_hi"), (dict(z_lo=1.0, z_hi=0.5), b"z_lo"), (dict(z_lo=inf, z_hi=-inf), b"z_lo"),
        (dict(t_stride=9), b"t_stride"), (dict(T=a, t_stride=3), b"t_stride"), (dict(t_stride=-12), b"t_stride"),
        (dict(rows_per_frame=500), b"rows_per_frame"), (dict(off=None), b"rows_per_frame"), (dict(off=None, rows_per_frame=-5), b"rows_per_frame"),
        (dict(rows_per_frame=-5), b"rows_per_frame"),
        (dict(top_label=a), b"top_label without label"),
        (dict(min_points=0), b"min_points"), (dict(min_points=-2), b"min_points"),
        (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(B=1, nx=3, ny=1, ws_bytes=79), b"workspace"),
    )
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and NAME.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, NAME)


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import bev
    from camradepth_amd.live import LivePipeline
    from tests import bev_ref
    xyz, off = torch.zeros(10, 3), torch.tensor([0, 10], dtype=torch.int32)
    for first, kw in ((xyz, dict(frame_offsets=off)), ({"xyz": xyz, "frame_offsets": off}, {}),
                      ({"points": torch.zeros(1, 2, 5, 3), "valid": torch.ones(1, 2, 5, dtype=torch.uint8)}, {})):
        with pytest.raises(built.CrdError, match="cuda"):
            bev.bev_grid(first, **kw)
    for kw, word in ((dict(x_range=(0, 80.2)), "x_range"), (dict(y_range=(40, -40)), "y_range"), (dict(cell=0.0), "x_range"),
                     (dict(cell=float("nan")), "x_range"), (dict(x_range=(0, float("inf"))), "x_range"), (dict(x_range=(0, 80), cell=1e-4), "x_range"),
                     (dict(x_range=(0, 1, 2)), "x_range"), (dict(z_range=(1.0, 0.0)), "z_range"), (dict(z_range=(float("nan"), 0.0)), "z_range"),
                     (dict(min_points=0), "min_points"), (dict(min_points=1.5), "min_points")):
        with pytest.raises(built.CrdError, match=word):                    # judged before the tensors: no device is needed
            bev.bev_grid(xyz, off, **kw)
    with pytest.raises(built.CrdError, match="frame_offsets"):
        bev.bev_grid({"xyz": xyz, "frame_offsets": off}, off)
    with pytest.raises(built.CrdError, match="dictionary"):
        bev.bev_grid({"xyz": xyz})
    with pytest.raises(built.CrdError, match="z_range"):
        bev.picture({"z_max": torch.zeros(1, 4, 4)}, (0.0,))
    with pytest.raises(built.CrdError, match="cuda"):
        bev.picture({"z_max": torch.zeros(1, 4, 4)}, (-2.0, 4.0))
    with pytest.raises(built.CrdError, match="bev= needs cloud="):
        LivePipeline(None, 2, bev={})                                       # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="bev="):
        LivePipeline(None, 2, cloud={}, bev=dict(colour=True))
    assert bev.grid_shape() == (160, 160) and bev.grid_shape((0, 80), (-40, 40), 0.2) == (400, 400) and bev.grid_shape((-1, 0.5), (2, 5.5), 0.5) == (3, 7)
    assert bev.grid_shape((-1.3, -1.3 + 16 * 0.2), (0.7, 0.7 + 12 * 0.2), 0.2) == (16, 12)
    for shape in ((1, 3, 1), (2, 160, 160)):                               # the header's formula, at two sizes
        cells = shape[0] * shape[1] * shape[2]
        assert bev.workspace_bytes(*shape) == 2 * ((8 * cells + 15) & ~15) + ((4 * cells + 15) & ~15) == bev_ref.workspace_bytes(*shape)
    assert bev.workspace_bytes(1, 3, 1) == 80 and bev.workspace_bytes(2, 160, 160) == 1024000
    T = bev.CAM_TO_BEV
    assert T.dtype == torch.float64 and tuple(T.shape) == (3, 4)
    right, down, forward = (T[:, :3] @ torch.tensor(v, dtype=torch.float64) for v in ((1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0)))
    assert forward.tolist() == [1, 0, 0] and right.tolist() == [0, -1, 0] and down.tolist() == [0, 0, -1] and T[:, 3].abs().sum() == 0
