"""CPU: the C ABI of the map objects without a GPU.  crd_map_objects is declared, exported and bound with the same argument count; it
refuses every bad argument the header lists before any GPU call, with the documented status and a crd_last_error text that names the
entry and the argument; the Python interface refuses host tensors, bad numbers, unknown option names and objects= without occupancy=."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "crd_map_objects"
ORDER = ("state", "M", "nx", "ny", "sources", "connectivity", "min_cells", "max_objects", "origin", "cell", "workspace", "workspace_bytes", "label",
         "objects", "sums", "centre", "info")
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
    assert len(args.split(",")) == len(built._SIGS[ENTRY]) == len(ORDER) + 1 == 18
    assert not [a for a in args.split(",") if "double" in a and "*" not in a]                  # fp64 through memory or as bit patterns
    assert L.crd_version() == 13 and built.ABI_VERSION == 13                                   # no struct, no changed signature
    assert re.search(r"#define\s+CRD_ABI_VERSION\s+13\b", h)


def test_map_objects_refuses_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    base = dict(state=a, M=3, nx=40, ny=36, sources=4, connectivity=8, min_cells=1, max_objects=256, origin=a, cell=0.5, workspace=a,
                workspace_bytes=8 * 3 * 40 * 36, label=a, objects=a, sums=a, centre=a, info=a)
    assert set(base) == set(ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, ENTRY)(*[built.f64_bits(v[k]) if k == "cell" else v[k] for k in ORDER], None)

    refusals = (
        (dict(state=None), b"null"), (dict(origin=None), b"null"), (dict(workspace=None), b"null"), (dict(label=None), b"null"),
        (dict(objects=None), b"null"), (dict(sums=None), b"null"), (dict(info=None), b"null"),
        (dict(label=a + 2), b"label"), (dict(objects=a + 1), b"objects"), (dict(info=a + 2), b"info"), (dict(sums=a + 4), b"sums"),
        (dict(centre=a + 4), b"centre"), (dict(origin=a + 4), b"origin"), (dict(label=a + 2), b"aligned"), (dict(sums=a + 4), b"aligned"),
        (dict(workspace=a + 8), b"workspace"), (dict(workspace=a + 8), b"16-byte"),
        (dict(M=0), b"M 0"), (dict(M=-2), b"M -2"), (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=-4), b"ny -4"),
        (dict(ny=65536), b"ny 65536"), (dict(M=4096, nx=1024, ny=512, workspace_bytes=1 << 40), b"cells"),
        (dict(M=1, nx=65535, ny=32769, workspace_bytes=1 << 40), b"cells"),
        (dict(sources=0), b"sources 0"), (dict(sources=256), b"sources 256"), (dict(sources=-1), b"sources -1"),
        (dict(connectivity=6), b"connectivity 6"), (dict(connectivity=0), b"connectivity 0"), (dict(connectivity=-8), b"connectivity -8"),
        (dict(min_cells=0), b"min_cells 0"), (dict(min_cells=-1), b"min_cells -1"),
        (dict(max_objects=0), b"max_objects 0"), (dict(max_objects=65536), b"max_objects 65536"), (dict(max_objects=-1), b"max_objects -1"),
        (dict(workspace_bytes=8 * 3 * 40 * 36 - 1), b"workspace"), (dict(workspace_bytes=0), b"workspace"), (dict(workspace_bytes=-16), b"workspace"),
        (dict(nx=41, ny=37), b"are needed"),
        (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=INF), b"cell"), (dict(cell=NAN), b"cell"))
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and ENTRY.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, ENTRY)


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import objects
    from camradepth_amd.live import OBJECT_OPTIONS, LivePipeline
    spec = objects.ObjectSpec(0.5)
    assert (spec.cell, spec.sources, spec.source_mask, spec.connectivity, spec.min_cells, spec.max_objects) == (0.5, (2,), 4, 8, 1, 256)
    assert objects.ObjectSpec(0.5, sources=(2, 5)).source_mask == 36
    assert (objects.BACKGROUND, objects.SMALL, objects.OVERFLOW) == (-1, -2, -3)
    assert objects.SPEC_OPTIONS == {"sources": (2,), "connectivity": 8, "min_cells": 1, "max_objects": 256} and OBJECT_OPTIONS is objects.SPEC_OPTIONS
    assert objects.workspace_bytes(1, 1, 1) == 16 and objects.workspace_bytes(8, 400, 400) == 8 * 8 * 400 * 400
    assert all(objects.workspace_bytes(M, nx, ny) % 16 == 0 and 8 * M * nx * ny <= objects.workspace_bytes(M, nx, ny) <= (8 * nx * ny + 64) * M
               for M, nx, ny in ((1, 1, 1), (3, 5, 7), (2, 33, 65)))
    for kw, word in ((dict(cell=0.0), "cell"), (dict(cell=NAN), "cell"), (dict(cell=-1.0), "cell"), (dict(cell=INF), "cell"), (dict(cell="x"), "cell"),
                     (dict(sources=()), "sources"), (dict(sources=(8,)), "sources"), (dict(sources=(-1,)), "sources"), (dict(sources=2), "sources"),
                     (dict(sources=(1.5,)), "sources"), (dict(connectivity=6), "connectivity"), (dict(connectivity=8.5), "connectivity"),
                     (dict(connectivity=None), "connectivity"), (dict(min_cells=0), "min_cells"), (dict(min_cells=True), "min_cells"),
                     (dict(min_cells=2 ** 31), "min_cells"), (dict(max_objects=0), "max_objects"), (dict(max_objects=65536), "max_objects"),
                     (dict(max_objects=2.5), "max_objects")):
        with pytest.raises(built.CrdError, match=word):
            objects.ObjectSpec(**dict(dict(cell=0.5), **kw))
    state, origin = torch.zeros(1, 5, 7, dtype=torch.uint8), torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(built.CrdError, match="cuda"):
        objects.map_objects(spec, state, origin)
    with pytest.raises(built.CrdError, match="cuda"):
        objects.map_objects(spec, {"state": state, "origin": origin}, {"state": state, "origin": origin})
    with pytest.raises(built.CrdError, match="ObjectSpec"):
        objects.map_objects(None, state, origin)
    for shape in ((0, 5, 7), (1, 0, 7), (1, 5, 65536), (4096, 1024, 512)):
        with pytest.raises(built.CrdError, match="cells"):
            objects.ObjectWorkspace(spec, *shape, device="cpu")
        with pytest.raises(built.CrdError, match="cells"):
            objects.workspace_bytes(*shape)
    with pytest.raises(built.CrdError, match="ObjectSpec"):
        objects.ObjectWorkspace(None, 1, 5, 7, device="cpu")
    ws = objects.ObjectWorkspace(objects.ObjectSpec(0.5, max_objects=9), 2, 5, 7, device="cpu")
    assert {k: (tuple(v.shape), v.dtype) for k, v in ws.out.items()} == {
        "label": ((2, 5, 7), torch.int32), "objects": ((2, 9, 8), torch.int32), "sums": ((2, 9, 2), torch.int64),
        "centre": ((2, 9, 2), torch.float64), "info": ((2, 4), torch.int32)}
    assert ws.buf.numel() == objects.workspace_bytes(2, 5, 7) == 560 and ws.buf.dtype == torch.uint8
    with pytest.raises(built.CrdError, match="objects= needs occupancy="):
        LivePipeline(None, 2, cloud={}, objects={})                            # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="objects="):
        LivePipeline(None, 2, cloud={}, occupancy={}, objects=dict(max_object=4))
    with pytest.raises(built.CrdError, match="objects="):
        LivePipeline(None, 2, cloud={}, occupancy={}, objects=[8])
