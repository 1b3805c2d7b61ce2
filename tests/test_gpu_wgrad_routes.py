"""Every launch route of the weight-gradient kernels -- crd_conv_wgrad (generic split-K and streaming 3x3), crd_conv_wgrad_grouped,
crd_dwconv3x3_wgrad -- against a float64 reference, BIT FOR BIT (tests/test_wgrad_routes_cpu.py: the tables, the descriptors, the
operands and the references live there, and the conditions under which every fp32 partial sum is exact are checked there on the CPU).
The Gaussian-operand tests of tests/test_gpu_ops.py cover realistic magnitudes under a tolerance of 2e-3; one missing border pixel,
halo column, tap or split tail is one term of hundreds and passes there.  Here it cannot.

Per dense case: the route is asserted through crd_conv_wgrad_route on the very descriptor that is launched; dw and dbias, from zero and
from a preloaded state, equal the reference; the operands are slices of wider buffers whose other channels are NaN, and the channels
of dy between Cout and its round-up to 8 are NaN as well (they may be read, they feed accumulator rows that are never stored).
Streaming cases run under every planning variant (partial-copy capacities, workgroup budgets), with atomics and with per-split copies."""
import ctypes as C

import pytest
import torch

from tests.test_wgrad_routes_cpu import (DENSE, DW_REPLICAS, DWC, GENERIC, STREAM, VARIANTS, dense_reference, dw_reference, generic_parts, rup8,
                                         slice_geometry, stream_parts, wgrad_desc)
from tests.util import to_grad, zsum

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _poisoned(t, ld, coff):
    """NCHW float64 on the CPU -> pixel-major bf16 [B][H][W][ld] on the GPU with t at channel offset coff and NaN everywhere else"""
    B, Cc, H, W = t.shape
    buf = torch.full((B, H, W, ld), NAN, dtype=torch.bfloat16)
    buf[..., coff:coff + Cc] = t.permute(0, 2, 3, 1).to(torch.bfloat16)
    return buf.cuda()


def _operands(c, r):
    x_ld, x_coff, dy_ld, dy_coff = slice_geometry(c)
    assert dy_ld >= dy_coff + rup8(c["Cout"])
    return _poisoned(r["x"], x_ld, x_coff), _poisoned(r["dy"], dy_ld, dy_coff)


def _same(got, want, what, index):
    """torch.equal with a message that names how many elements differ and the first of them"""
    if torch.equal(got, want):
        return
    wrong = (got != want).nonzero()
    raise AssertionError(f"{what}: {len(wrong)} of {want.numel()} elements differ from the float64 reference, the first at {index} = "
                         f"{wrong[0].tolist()}: got {got[tuple(wrong[0])].item()!r}, reference {want[tuple(wrong[0])].item()!r}")


def _launch(lib, d, what):
    lib.check(lib.load().crd_conv_wgrad(C.byref(d), lib.stream()), what)
    torch.cuda.synchronize()


def _desc(lib, c, variant, x, dy, dw, db, parts=None, capacity=0):
    d = wgrad_desc(lib, c, dict(x=x.data_ptr(), dy=dy.data_ptr(), dw=dw.data_ptr(), dbias=db.data_ptr()))
    d.wg_budget = VARIANTS[variant][1]
    if parts is not None:
        d.dw_partials, d.dw_partial_capacity = parts.data_ptr(), capacity
    return d


def _accumulating_runs(lib, c, r, variant, label, x, dy):
    """crd_conv_wgrad into zeroed and into preloaded accumulators"""
    for what, old_w, old_b in (("zeroed", None, None), ("preloaded", r["old_dw"], r["old_db"])):
        dw = zsum(*r["dw"].shape) if old_w is None else to_grad(old_w).cuda()
        db = zsum(c["Cout"]) if old_b is None else to_grad(old_b).cuda()
        d = _desc(lib, c, variant, x, dy, dw, db)
        assert lib.wgrad_route(d) == label
        _launch(lib, d, f"crd_conv_wgrad {c['name']} {variant} {what}")
        want_w = to_grad(r["dw"] if old_w is None else old_w + r["dw"])
        want_b = to_grad(r["dbias"] if old_b is None else old_b + r["dbias"])
        _same(dw.cpu(), want_w, f"{c['name']} {variant} {what}: dw", "[co, tap, ci]")
        _same(db.cpu(), want_b, f"{c['name']} {variant} {what}: dbias", "[co]")


@pytest.mark.parametrize("name", GENERIC)
def test_generic_route_is_exact(name):
    from camradepth_amd import lib
    c, r = DENSE[name], dense_reference(name)
    assert generic_parts(c["label"]) is not None
    x, dy = _operands(c, r)
    _accumulating_runs(lib, c, r, "default", c["label"], x, dy)
    assert lib.load().crd_conv_wgrad_splits(C.byref(_desc(lib, c, "default", x, dy, zsum(1), zsum(1)))) == 0


def test_wide_3x3_layer_takes_the_generic_kernel():
    """3x3 / stride 1 / pad 1 on a 9 x 40 grid towards 160 channels: the streaming kernel covers 128 (under the earlier routing rows
    128.. of dw were never written and dbias[128..] summed other pixels' data); every row and every bias channel is exact"""
    from camradepth_amd import lib
    c, r = DENSE["g128_cout160_3x3_former_stream"], dense_reference("g128_cout160_3x3_former_stream")
    assert (c["Cout"], c["k"], c["s"], c["p"], c["H"], c["W"]) == (160, 3, 1, 1, 9, 40)
    x, dy = _operands(c, r)
    dw, db = zsum(*r["dw"].shape), zsum(160)
    d = _desc(lib, c, "default", x, dy, dw, db)
    assert lib.wgrad_route(d).startswith("k_wgrad<2,2,4,4>/") and lib.load().crd_conv_wgrad_splits(C.byref(d)) == 0
    _launch(lib, d, "crd_conv_wgrad")
    assert (r["dw"][128:].abs().sum((1, 2)) > 0).all() and (r["dbias"] != 0).any()
    assert torch.equal(dw.cpu()[128:], to_grad(r["dw"])[128:]) and torch.equal(dw.cpu(), to_grad(r["dw"]))
    assert torch.equal(db.cpu(), to_grad(r["dbias"])) and db.numel() == 160


@pytest.mark.parametrize("name", STREAM)
def test_streaming_route_is_exact(name):
    from camradepth_amd import lib
    c, r = DENSE[name], dense_reference(name)
    x, dy = _operands(c, r)
    for variant, (cap, budget) in VARIANTS.items():
        label = c["labels"][variant]
        _, S, rows, chunks = stream_parts(label)
        if not cap:                    # (a capacity means nothing without the copies)
            _accumulating_runs(lib, c, r, variant, label, x, dy)
        # ---- per-split copies: plain stores into S copies, dw untouched, dbias through its accumulator as before
        parts = torch.full((S + 1,) + tuple(r["dw"].shape), NAN, device="cuda")
        dw, db = torch.full(tuple(r["dw"].shape), 7, dtype=torch.int64, device="cuda"), zsum(c["Cout"])
        d = _desc(lib, c, variant, x, dy, dw, db, parts, cap or S)
        assert lib.wgrad_route(d) == label and lib.load().crd_conv_wgrad_splits(C.byref(d)) == S
        _launch(lib, d, f"crd_conv_wgrad {name} {variant} partials")
        assert bool((dw == 7).all()), f"{name} {variant}: dw was written although dw_partials is given"
        assert bool(torch.isnan(parts[S]).all()), f"{name} {variant}: a copy beyond the {S} splits was written"
        assert not bool(torch.isnan(parts[:S]).any()), f"{name} {variant}: {int(torch.isnan(parts[:S]).sum())} elements of the {S} copies not written"
        _same(parts[:S].double().sum(0).cpu(), r["dw"], f"{name} {variant}: float64 sum of the {S} copies", "[co, tap, ci]")
        _same(db.cpu(), to_grad(r["dbias"]), f"{name} {variant}: dbias of the partials run", "[co]")


def test_grouped_dispatch_of_every_generic_case_is_exact():
    """crd_wgrad_group_build + crd_conv_wgrad_grouped over all generic-route cases at once (its own split planning: 8 K-steps per
    workgroup), slices included"""
    from camradepth_amd import lib
    lb = lib.load()
    cases = [DENSE[n] for n in GENERIC]
    refs = [dense_reference(n) for n in GENERIC]
    keep = []
    descs = (lib.WgradDesc * len(cases))()
    for i, (c, r) in enumerate(zip(cases, refs)):
        x, dy = _operands(c, r)
        dw, db = zsum(*r["dw"].shape), zsum(c["Cout"])
        keep.append((x, dy, dw, db))
        descs[i] = _desc(lib, c, "default", x, dy, dw, db)
    info = lib.WgradGroupInfo()
    lib.check(lb.crd_wgrad_group_build(descs, len(cases), None, 0, C.byref(info)), "size query")
    assert info.n_problems == len(cases) and all(n > 0 for n in info.n_items)          # every tile configuration has work
    host = (C.c_uint8 * info.bytes)()
    lib.check(lb.crd_wgrad_group_build(descs, len(cases), host, info.bytes, C.byref(info)), "build")
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    lib.check(lb.crd_conv_wgrad_grouped(table.data_ptr(), C.byref(info), lib.stream()), "crd_conv_wgrad_grouped")
    torch.cuda.synchronize()
    for c, r, (_, _, dw, db) in zip(cases, refs, keep):
        _same(dw.cpu(), to_grad(r["dw"]), f"grouped {c['name']}: dw", "[co, tap, ci]")
        _same(db.cpu(), to_grad(r["dbias"]), f"grouped {c['name']}: dbias", "[co]")


@pytest.mark.parametrize("name", list(DWC))
def test_depthwise_wgrad_is_exact(name):
    """crd_dwconv3x3_wgrad: the nine shifted products and sum dy, spread over R accumulator copies whose sum is the gradient"""
    from camradepth_amd import lib
    c, r = DWC[name], dw_reference(name)
    B, H, W, C_ = c["B"], c["H"], c["W"], c["C"]
    x, dy = (t.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous().cuda() for t in (r["x"], r["dy"]))
    for R in DW_REPLICAS:
        for what, old in (("zeroed", None), ("preloaded", r["old"][:R])):
            dw10 = zsum(R, 10, C_) if old is None else to_grad(old).cuda()
            lib.check(lib.load().crd_dwconv3x3_wgrad(x.data_ptr(), dy.data_ptr(), B, H, W, C_, dw10.data_ptr(), R, None, 1, None, None, lib.stream()),
                      "crd_dwconv3x3_wgrad")
            torch.cuda.synchronize()
            want = to_grad(r["dw10"] if old is None else old.sum(0) + r["dw10"])
            _same(dw10.sum(0).cpu(), want, f"{name} R = {R} {what}: sum of the copies", "[tap, channel]")
