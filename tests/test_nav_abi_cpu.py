"""CPU: the C ABI of the navigation field without a GPU.  crd_nav_field and crd_nav_paths are declared, exported and bound with the same
argument counts; both refuse every bad argument the header lists before any GPU call, with the documented status and a crd_last_error
text that names the entry and the argument; the Python interface refuses host tensors, bad numbers, nav= without field= and unknown
option names."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD, PATHS = "crd_nav_field", "crd_nav_paths"


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
    for name, n_args in ((FIELD, 16), (PATHS, 17)):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in built._SIGS and getattr(L, name).argtypes is not None, f"{name} is not bound"
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, h, flags=re.S).group(1)
        assert len(args.split(",")) == len(built._SIGS[name]) == n_args
        assert not [a for a in args.split(",") if "double" in a and "*" not in a]              # fp64 through memory or as bit patterns
    assert L.crd_version() == 13                                                               # no struct, no changed signature


F_ORDER = ("cost", "M", "nx", "ny", "goals", "n_goals", "G", "origin", "cell", "neutral", "blocked_at", "max_rounds", "togo", "next", "info")
P_ORDER = ("starts", "path_map", "K", "P", "origin", "cell", "togo", "next", "M", "nx", "ny", "cells", "xy", "n_cells", "start_togo", "status")
INF, NAN = float("inf"), float("nan")
SHAPE_REFUSALS = (
    (dict(M=0), b"M 0"), (dict(M=-2), b"M -2"), (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"), (dict(ny=-4), b"ny -4"),
    (dict(ny=65536), b"ny 65536"), (dict(nx=1024, ny=513), b"2^19"), (dict(nx=65535, ny=9), b"2^19"), (dict(M=4096, nx=1024, ny=512), b"cells"),
    (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=INF), b"cell"), (dict(cell=NAN), b"cell"))


def refused(built, name, call, refusals):
    L = built.load()
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and name.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, name)


def test_nav_field_refuses_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    base = dict(cost=a, M=3, nx=40, ny=36, goals=a, n_goals=a, G=2, origin=a, cell=0.5, neutral=50, blocked_at=253, max_rounds=64, togo=a, next=a,
                info=a)
    assert set(base) == set(F_ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, FIELD)(*[built.f64_bits(v[k]) if k == "cell" else v[k] for k in F_ORDER], None)

    refused(built, FIELD, call, SHAPE_REFUSALS + (
        (dict(cost=None), b"null"), (dict(goals=None), b"null"), (dict(origin=None), b"null"), (dict(togo=None), b"null"), (dict(info=None), b"null"),
        (dict(goals=a + 4), b"goals"), (dict(origin=a + 4), b"origin"), (dict(n_goals=a + 2), b"n_goals"), (dict(togo=a + 1), b"togo"),
        (dict(info=a + 2), b"info"), (dict(goals=a + 4), b"aligned"), (dict(togo=a + 2), b"aligned"),
        (dict(G=0), b"G 0"), (dict(G=-1), b"G -1"),
        (dict(neutral=0), b"neutral 0"), (dict(neutral=256), b"neutral 256"), (dict(neutral=-1), b"neutral -1"),
        (dict(blocked_at=0), b"blocked_at 0"), (dict(blocked_at=256), b"blocked_at 256"), (dict(blocked_at=-1), b"blocked_at -1"),
        (dict(max_rounds=0), b"max_rounds 0"), (dict(max_rounds=4097), b"max_rounds 4097"), (dict(max_rounds=-3), b"max_rounds -3")))


def test_nav_paths_refuses_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15
    base = dict(starts=a, path_map=a, K=5, P=130, origin=a, cell=0.5, togo=a, next=a, M=3, nx=40, ny=36, cells=a, xy=a, n_cells=a, start_togo=a,
                status=a)
    assert set(base) == set(P_ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, PATHS)(*[built.f64_bits(v[k]) if k == "cell" else v[k] for k in P_ORDER], None)

    refused(built, PATHS, call, SHAPE_REFUSALS + (
        (dict(starts=None), b"null"), (dict(origin=None), b"null"), (dict(togo=None), b"null"), (dict(next=None), b"null"), (dict(cells=None), b"null"),
        (dict(n_cells=None), b"null"), (dict(start_togo=None), b"null"), (dict(status=None), b"null"),
        (dict(starts=a + 4), b"aligned"), (dict(origin=a + 4), b"aligned"), (dict(xy=a + 4), b"aligned"), (dict(path_map=a + 2), b"aligned"),
        (dict(togo=a + 1), b"aligned"), (dict(cells=a + 2), b"aligned"), (dict(n_cells=a + 3), b"aligned"), (dict(start_togo=a + 2), b"aligned"),
        (dict(status=a + 2), b"aligned"),
        (dict(K=0), b"K 0"), (dict(K=-1), b"K -1"), (dict(P=0), b"P 0"), (dict(P=-7), b"P -7"), (dict(K=1 << 15, P=1 << 15), b"K * P")))


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import nav
    from camradepth_amd.live import NAV_OPTIONS, LivePipeline
    spec = nav.NavSpec(0.5)
    assert (spec.cell, spec.neutral, spec.blocked_at, spec.max_rounds) == (0.5, 50, 253, 64)
    assert nav.UNREACHED == 0x7FFFFFFF and len(nav.NEIGHBOURS) == 8 and nav.workspace_bytes(8, 400, 400) == 0
    for kw, word in ((dict(cell=0.0), "cell"), (dict(cell=NAN), "cell"), (dict(cell=-1.0), "cell"), (dict(cell=INF), "cell"), (dict(cell="x"), "cell"),
                     (dict(neutral=0), "neutral"), (dict(neutral=256), "neutral"), (dict(neutral=1.5), "neutral"), (dict(blocked_at=0), "blocked_at"),
                     (dict(blocked_at=256), "blocked_at"), (dict(blocked_at=True), "blocked_at"), (dict(max_rounds=0), "max_rounds"),
                     (dict(max_rounds=4097), "max_rounds"), (dict(max_rounds=None), "max_rounds")):
        with pytest.raises(built.CrdError, match=word):
            nav.NavSpec(**dict(dict(cell=0.5), **kw))
    cost = torch.zeros(1, 5, 7, dtype=torch.uint8)
    origin, goals = torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 1, 2, dtype=torch.float64)
    with pytest.raises(built.CrdError, match="cuda"):
        nav.nav_field(spec, cost, origin, goals)
    with pytest.raises(built.CrdError, match="cuda"):
        nav.nav_field(spec, {"cost": cost}, {"origin": origin}, goals)
    with pytest.raises(built.CrdError, match="'cost'"):
        nav.nav_field(spec, {"cost": None}, origin, goals)
    with pytest.raises(built.CrdError, match="NavSpec"):
        nav.nav_field(None, cost, origin, goals)
    res = {"togo": torch.zeros(1, 5, 7, dtype=torch.int32), "next": cost}
    with pytest.raises(built.CrdError, match="cuda"):
        nav.plan_paths(spec, res, origin, torch.zeros(3, 2, dtype=torch.float64), 9)
    with pytest.raises(built.CrdError, match="'next'"):
        nav.plan_paths(spec, {"togo": res["togo"], "next": None}, origin, None, 9)
    with pytest.raises(built.CrdError, match="NavSpec"):
        nav.plan_paths(0.5, res, origin, None, 9)
    for shape in ((0, 5, 7), (1, 0, 7), (1, 5, 65536), (1, 1024, 513), (4096, 1024, 512)):
        with pytest.raises(built.CrdError, match="cells"):
            nav.NavWorkspace(spec, *shape, device="cpu")
    with pytest.raises(built.CrdError, match="NavSpec"):
        nav.NavWorkspace(None, 1, 5, 7, device="cpu")
    ws = nav.NavWorkspace(spec, 2, 5, 7, device="cpu")
    assert {k: (tuple(v.shape), v.dtype) for k, v in ws.out.items()} == {
        "togo": ((2, 5, 7), torch.int32), "next": ((2, 5, 7), torch.uint8), "info": ((2, 4), torch.int32)}
    out = nav.path_outputs(3, 9, device="cpu")
    assert {k: tuple(v.shape) for k, v in out.items()} == {"cells": (3, 9), "xy": (3, 9, 2), "n_cells": (3,), "start_togo": (3,), "status": (3,)}
    assert "xy" not in nav.path_outputs(3, 9, xy=False, device="cpu")
    assert set(NAV_OPTIONS) == {"goals", "starts", "neutral", "blocked_at", "max_rounds", "xy"}
    with pytest.raises(built.CrdError, match="nav= needs field="):
        LivePipeline(None, 2, cloud={}, occupancy={}, nav=dict(goals=1))   # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="nav="):
        LivePipeline(None, 2, cloud={}, occupancy={}, field={}, nav=dict(goal=1))
