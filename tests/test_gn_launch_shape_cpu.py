"""CPU: crd_gn_launch_shape -- the partition of the two elementwise GroupNorm passes (crd_gn_apply: kind 0, crd_gn_bwd_apply: kind 1).

For every (P, C, B) the training plans at the benchmark's size (base and supervised segmentation) and the 928 x 1600 plan launch,
and for pixel counts around a batch: the chunks tile [0, P) exactly once, every chunk but a sample's last is a whole number of
batches, the grid never exceeds the cap, and grids that do not fill the chip keep the small-grid rule (fewer pixels per lane)."""
import importlib.util
import os

import pytest

TPB, CAP, SMALL, MINPIX = 256, 2048, 256, 2          # camradepth_amd/csrc/norm.hip: TPB, gn_knobs()
SLOTS = {0: 4, 1: 2}                                 # U_APPLY, U_BWD: pixels per lane of one batch
KINDS = {"crd_gn_apply": 0, "crd_gn_apply_fp8": 0, "crd_gn_bwd_apply": 1, "crd_gn_bwd_apply_fp8": 1}


def cdiv(a, b):
    return -(-a // b)


def lanes(C):
    return max(1, TPB // (C // 8))


def small_grid(P, C, B):
    """The rule the elementwise passes have always had: fewer than SMALL workgroups at 8 pixels per lane."""
    return cdiv(P, lanes(C) * 8) * B < SMALL


def small_grid_rule(P, C, B):
    """(nblk, chunk) of a small grid: MINPIX pixels per lane, so that more CUs get a workgroup."""
    nblk = max(1, min(cdiv(P, lanes(C) * MINPIX), max(1, CAP // B)))
    chunk = cdiv(P, nblk)
    return cdiv(P, chunk), chunk


def check(lib, P, C, B, kind):
    nblk, chunk, batch = lib.gn_launch_shape(P, C, B, kind)
    where = f"P={P} C={C} B={B} kind={kind}: nblk={nblk} chunk={chunk} batch={batch}"
    assert batch == SLOTS[kind] * lanes(C), where
    assert nblk >= 1 and chunk >= 1, where
    assert (nblk - 1) * chunk < P <= nblk * chunk, "the chunks tile [0, P) exactly once: " + where
    assert nblk * B <= max(CAP, B), "cap: " + where
    if small_grid(P, C, B):
        assert (nblk, chunk) == small_grid_rule(P, C, B), "small-grid rule: " + where
    else:
        assert nblk == 1 or chunk % batch == 0, "every chunk but the last is whole batches: " + where
        assert chunk >= min(P, 8 * lanes(C)), "at least 8 pixels per lane: " + where
        # no fewer workgroups than the cap allows: the next smaller whole-batch chunk (if 8 pixels per lane allow one) would exceed it
        smaller = chunk - batch
        assert chunk >= P or smaller < 8 * lanes(C) or cdiv(P, smaller) * B > CAP, "grid smaller than the cap asks for: " + where
    return nblk, chunk, batch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


@pytest.fixture(scope="module")
def plan_shapes(built):
    spec = importlib.util.spec_from_file_location(
        "plan_fingerprint_gn", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "plan_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    out = {}
    for name, make in (("C2", lambda: fp.build(8, 256, 416)), ("C3", lambda: fp.build(8, 256, 416, supervised_seg=True)),
                       ("928x1600", lambda: fp.build(1, 928, 1600, supervised_seg=True))):
        plan = make()
        shapes = set()
        for op in list(plan.fwd) + list(plan.bwd):
            if op.name in KINDS:
                a = op.args[4:7] if KINDS[op.name] == 0 else op.args[8:11]
                shapes.add((int(a[1]), int(a[2]), int(a[0]), KINDS[op.name]))
        out[name] = sorted(shapes)
    return out


@pytest.mark.parametrize("config", ["C2", "C3", "928x1600"])
def test_partition_of_every_plan_shape(built, plan_shapes, config):
    shapes = plan_shapes[config]
    assert len(shapes) >= 8 and {k for *_, k in shapes} == {0, 1}, shapes
    big = 0
    for P, C, B, kind in shapes:
        nblk, chunk, batch = check(built, P, C, B, kind)
        big += not small_grid(P, C, B)
    assert big >= 2, "the plan has grids that fill the chip"


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("C,B", [(16, 2), (64, 8), (128, 2), (128, 16), (320, 2), (512, 8), (2048, 2), (2048, 300)])
def test_partition_around_a_batch(built, C, B, kind):
    batch = SLOTS[kind] * lanes(C)
    for P in (1, batch - 1, batch, batch + 1, 3 * batch + batch // 4, 1000 * batch + 1, 100003, 2 ** 31 - 1):
        if P >= 1:
            check(built, P, C, B, kind)


def test_large_grid_is_capped_with_whole_batches(built):
    """The decoder's widest tensors: the cap is active, a workgroup runs several batches, only the last chunk is ragged."""
    for P, C, B in ((106496, 128, 8), (106496 + 77, 128, 16), (6656, 512, 8)):
        nblk, chunk, batch = check(built, P, C, B, 1)
        assert not small_grid(P, C, B) and chunk >= 2 * batch and CAP // 2 < nblk * B <= CAP, (P, C, B, nblk, chunk)


def test_query_refuses_bad_arguments(built):
    import ctypes as Ct
    L = built.load()
    out = (Ct.c_int32 * 3)()
    ptr = [Ct.cast(Ct.byref(out, 4 * i), Ct.c_void_p) for i in range(3)]
    assert L.crd_gn_launch_shape(64, 128, 2, 0, *ptr) == 0
    for args in ((0, 128, 2, 0), (64, 128, 0, 0), (64, 128, 2, 2), (64, 24, 2, 0), (64, 4096, 2, 1)):
        assert L.crd_gn_launch_shape(*args, *ptr) != 0, args
    assert L.crd_gn_launch_shape(64, 128, 2, 0, None, ptr[1], ptr[2]) != 0
