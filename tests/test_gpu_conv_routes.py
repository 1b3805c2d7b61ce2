"""Every launch route of crd_conv_igemm against a float64 reference (tests/test_conv_routes_cpu.py: ROUTE_CASES -- the table, the
descriptors, the operands, the reference and the error bound live there and are checked on the CPU).  tests/test_gpu_igemm.py runs
small shapes, which all take the 64 x 64 tiles; the 128-row tiles the training step runs at its own size -- two row tiles per wave,
three / five column tiles with the statistics fold over four row waves, their own fp32 epilogue branch -- are reached here by shape
alone, just above the dispatch thresholds, with ragged edges.

Per case: the route is asserted through crd_conv_igemm_route on the very descriptor that is launched; the output is compared
elementwise with the float64 reference under the derived bound (sigmoid cases: the relative pair of test_gpu_igemm.assert_close, the
kernel's sigmoid being an unbounded approximation); channels of the wider output buffer outside the slice come back bit-unchanged
(buffers are NaN-filled, 7.0 under accumulation); GroupNorm and channel sums are compared with float64 sums of the stored tensor;
the fused GroupNorm-backward reduce with a float64 reduce of the stored gradient; and a second launch gives the same bits."""
import ctypes as C

import pytest
import torch

from tests.test_conv_routes_cpu import CASES, cdiv, descriptor, label_parts, partial_capacity, reduce_reference, reference, tile_rows, y_geometry
from tests.test_gpu_igemm import assert_close, to_pm
from tests.util import GRAD_BITS, STAT_BITS, to_stat, zsum

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _buffers(c, o):
    """Device buffers of a case in their initial state, and the address table of its descriptor."""
    B, N = c["B"], c["N"]
    generic = label_parts(c["label"]) is not None
    xl, xo = c["Cx"] + c["x_pad"][0], c["x_pad"][1]
    # the channels around the operand slice are poison: a read outside [x_coff, x_coff + Cin) shows in the result
    x = to_pm(o["x"], ld=xl, coff=xo)
    if generic:
        x[..., :xo] = NAN
        x[..., xo + c["Cx"]:] = NAN
    YH, YW, yc = y_geometry(c)
    yl, yo = yc + c["y_pad"][0], c["y_pad"][1]
    ydt = torch.float32 if c["y_f32"] else torch.bfloat16
    y = torch.full((B, YH, YW, yl), 7.0 if c["acc"] else NAN, dtype=ydt)
    if c["acc"]:
        y[..., yo:yo + yc] = o["old"].to(ydt)
    t = {"x": x, "w": o["w"].to(torch.bfloat16).cuda(), "y": y.cuda()}
    if c["bias"]:
        t["bias"] = o["bias"].contiguous().cuda()
    if c["res"]:
        res = torch.full((B, YH, YW, yc + 4), NAN)
        res[..., :yc] = o["res"]
        t["res"] = res.cuda()
    if c["res_scale"]:
        t["res_scale"] = o["res_scale"].cuda()
    if c["stats"]:
        t["stats"] = zsum(B, N // 16, 2)
        if c["stats"] != "atomics":
            t["partial"] = torch.full((partial_capacity(c),), NAN, device="cuda")          # every row that is read must have been written
    if c["chan"]:
        t["chan"] = zsum(B, N, 2)
    if c["red"]:
        gmul, _, xf32 = c["red"]
        rx = torch.zeros(B, c["OH"], c["OW"], N + 8, dtype=torch.float32 if xf32 else torch.bfloat16)
        rx[..., :N] = o["red_x"].view(B, c["OH"], c["OW"], N)
        t["red_x"] = rx.cuda()
        slab, _ = reduce_reference(c, o, torch.zeros(B, c["OH"] * c["OW"], N))
        t["red_stats"] = to_stat(slab).cuda()
        t["red_gamma"], t["red_beta"] = o["red_gamma"].cuda(), o["red_beta"].cuda()
        t["red_r"] = zsum(B * N * 2 + B * (N // (16 * gmul)) * 2)
    return t, {k: v.data_ptr() for k, v in t.items()}


def _launch(lib, c, o):
    t, ptr = _buffers(c, o)
    d = descriptor(lib, c, ptr)
    assert lib.conv_route(d) == c["label"]
    before = t["y"].clone()
    lib.check(lib.load().crd_conv_igemm(C.byref(d), lib.stream()), "crd_conv_igemm")
    torch.cuda.synchronize()
    return t, before


def _sum_bound(v, n, adds, square):
    """Error bound of an fp32 sum of the n values v (or their squares) that leaves the GPU through `adds` fixed-point conversions."""
    mag = (v * v if square else v.abs()).sum()
    return n * 2.0 ** -23 * mag + adds * 2.0 ** -STAT_BITS


@pytest.mark.parametrize("name", list(CASES))
def test_route_against_float64(name):
    from camradepth_amd import lib
    c = CASES[name]
    o, stored, bound = reference(name)
    t, before = _launch(lib, c, o)
    B, N = c["B"], c["N"]
    YH, YW, yc = y_geometry(c)
    yo = c["y_pad"][1]
    y = t["y"]
    got = y[..., yo:yo + yc].double().cpu()

    # ---- what lies around the slice is untouched, bit for bit
    outside = torch.ones(y.shape[-1], dtype=torch.bool, device="cuda")
    outside[yo:yo + yc] = False
    assert torch.equal(_bits(y)[..., outside], _bits(before)[..., outside]), f"{name}: channels outside the output slice were written"

    # ---- the stored values
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} output elements not written or not finite"
    if c["act"]:
        assert_close(got, stored, name)
    else:
        ratio = (got - stored).abs() / bound
        worst = ratio.max().item()
        print(f"{name}: worst error {worst:.3f} of the bound, {int((ratio > 1).sum())} of {ratio.numel()} elements outside")
        at = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
        assert worst <= 1.0, (f"{name}: element {at} (b, y, x, channel): got {got[tuple(at)].item():.8g}, reference "
                              f"{stored[tuple(at)].item():.8g}, bound {bound[tuple(at)].item():.3g}; {int((ratio > 1).sum())} elements outside")

    # ---- GroupNorm sums and channel sums of the stored tensor
    if c["stats"] or c["chan"]:
        assert not c["scatter"] and not (c["acc"] and not c["y_f32"])     # (bf16 sums are taken before the accumulation: not asked for here)
        P = YH * YW
        adds = 4 * cdiv(P, tile_rows(c["label"])) if label_parts(c["label"]) else 4 * P       # at most one conversion per wave and tile
        g = got.view(B, P, N)
        if c["stats"]:
            sv = t["stats"].double().cpu() * 2.0 ** -STAT_BITS
            g16 = g.view(B, P, N // 16, 16)
            for which, ref_s in enumerate((g16.sum((1, 3)), (g16 * g16).sum((1, 3)))):
                for b in range(B):
                    for s in range(N // 16):
                        tol = _sum_bound(g16[b, :, s], P * 16, adds, which == 1)
                        err = abs(sv[b, s, which] - ref_s[b, s])
                        assert err <= tol, f"{name}: GroupNorm sum [{b}][{s}][{which}] = {sv[b, s, which]:.8g}, stored values give {ref_s[b, s]:.8g} (bound {tol:.3g})"
        if c["chan"]:
            cv = t["chan"].double().cpu() * 2.0 ** -STAT_BITS
            for which, ref_c in enumerate((g.sum(1), (g * g).sum(1))):
                mag = (g * g if which else g.abs()).sum(1)
                tol = P * 2.0 ** -23 * mag + adds * 2.0 ** -STAT_BITS
                err = (cv[..., which] - ref_c).abs()
                assert (err <= tol).all(), f"{name}: channel sums [{which}]: worst {float((err / tol).max()):.3f} of the bound"

    # ---- the fused reduce phase of the GroupNorm backward, on the gradient that was stored
    if c["red"]:
        _, r_ref = reduce_reference(c, o, got.view(B, YH * YW, N))
        r = t["red_r"].double().cpu() * 2.0 ** -GRAD_BITS
        assert_close(r, r_ref, f"{name}: fused GroupNorm-backward reduce", rel=3e-4, elem=3e-4)

    # ---- a second launch: the same bits in the output and in every sum
    t2, _ = _launch(lib, c, o)
    for key in ("y", "stats", "chan", "red_r"):
        if key in t:
            a, b = (t[key], t2[key]) if key != "y" else (_bits(t[key]), _bits(t2[key]))
            assert torch.equal(a, b), f"{name}: {key} differs between two launches"
