"""Which kernel crd_conv_igemm launches, pinned through the host-side query crd_conv_igemm_route (no GPU: the query is host arithmetic
on the descriptor, from the same decision function and the same epilogue-branch conditions as the launch).

ROUTE_CASES is the table tests/test_gpu_conv_routes.py runs against a float64 reference: one small problem per route, each with the
label it is meant to reach.  The launcher picks the kernel from the problem size, so a retune of the dispatch rule moves a case off its
route without failing any numeric test; it fails here instead.  This file also holds what both files share -- the descriptor of a case,
its operands, its float64 reference and its error bound -- so that the bound can be checked against a float32 recomputation here, before
it costs a GPU run.

A case is written in LAUNCH terms (include/camradepth_hip.h: crd_conv_desc): x is [B][IH x IW][Cx] (Cx_ref real channels, the rest
padding with zero weights), the output [B][OH x OW][N]; gather 0 is a forward convolution, gather 1 the data gradient of a convolution
with this k / stride / pad whose INPUT grid is OH x OW (x is then dy on the IH x IW output grid of that convolution)."""
import ctypes as C
import functools
import importlib.util
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_args_cpu import IGEMM, RED, A, conv_desc


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ the cases
_DEFAULTS = dict(k=1, stride=1, pad=0, gather=0, Cx_ref=None, x_pad=(16, 8), y_pad=(16, 8), y_f32=0, bias=None, act=0, res=False,
                 res_scale=False, acc=0, stats=None, chan=False, scatter=None, red=None)


def _case(name, label, B, IH, IW, Cx, OH, OW, N, **kw):
    """bias: None / "shared" / "image"; stats: None / "atomics" / "partials" (a buffer of the documented size) / "fallback" (a buffer one
    float too small for the tile that runs: the launch falls back to atomics); scatter: (patch_k, patch_c); red: (gmul, act, x_f32);
    x_pad / y_pad: (extra channels of the buffer row, channel offset of the slice)."""
    bad = set(kw) - set(_DEFAULTS)
    assert not bad, bad
    c = dict(_DEFAULTS, name=name, label=label, B=B, IH=IH, IW=IW, Cx=Cx, OH=OH, OW=OW, N=N)
    c.update(kw)
    c["Cx_ref"] = c["Cx_ref"] or Cx
    return c


def fwd(name, label, B, Cref, Cpad, H, W, N, k=1, s=1, p=0, **kw):
    """forward convolution of a [B][Cref][H][W] input"""
    return _case(name, label, B, H, W, Cpad, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, N, k=k, stride=s, pad=p, Cx_ref=Cref, **kw)


def dgrad(name, label, B, N, H, W, Cdy, k=1, s=1, p=0, **kw):
    """data gradient, towards the [B][N][H][W] input, of a convolution with Cdy output channels"""
    return _case(name, label, B, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, Cdy, H, W, N, k=k, stride=s, pad=p, gather=1, **kw)


def scatter(name, label, B, PH, PW, Cx, pk, pc, **kw):
    """data gradient of a k = stride patch convolution: a pointwise GEMM towards pk * pk * pc columns, scattered to pk x pk patches"""
    return _case(name, label, B, PH, PW, Cx, PH, PW, pk * pk * pc, scatter=(pk, pc), **kw)


def K(t, mode, nst, kg=1):
    return "k_igemm<%s,MODE=%d,NST=%d,KG=%d>" % (t, mode, nst, kg)


S64, T32, T64, T96, T160, T128 = "2,2,1,1", "4,1,1,1", "2,2,2,1", "4,1,1,3", "4,1,1,5", "2,2,2,2"
RES = dict(y_f32=1, res=True, res_scale=True)
# Pixel grids just above the 192-tile threshold at B = 3, with ragged last tiles: 63 x 131 = 8253 pixels = 65 row tiles of 128 (195 tiles
# with one column tile), 50 x 83 = 4150 pixels = 33 row tiles (198 tiles with two column tiles).  As inputs of the strided layers:
# 250 x 522 -> 7x7 / 4 / pad 3 -> 63 x 131;  125 x 261 -> 3x3 / 2 / pad 1 -> 63 x 131;  198 x 330 -> 50 x 83;  99 x 165 -> 50 x 83.
# A stride-1 3x3 layer narrower than 32 pixels (wider ones are the halo kernel's) is tall instead: 31 x 267 = 8277 pixels, 65 row tiles.

ROUTE_CASES = [
    # ---- 128 x 64 tiles (k_igemm<2,2,2,1>: two row tiles per wave; fp32 output through the LDS-staged branch)
    fwd("t64_7x7s4_bias_atomics", K(T64, 0, 3) + "/vec+atomics", 3, 7, 8, 250, 522, 64, 7, 4, 3, bias="shared", stats="atomics"),
    fwd("t64_3x3s2_sigmoid_partials", K(T64, 0, 3) + "/vec+partials", 3, 20, 24, 125, 261, 48, 3, 2, 1, bias="image", act=1, stats="partials"),
    dgrad("t64_1x1_acc", K(T64, 1, 3) + "/vec", 3, 64, 63, 131, 72, acc=1),
    dgrad("t64_1x1_red", K(T64, 1, 3) + "/vec", 3, 64, 63, 131, 40, red=(2, 1, 0)),
    dgrad("t64_1x1_res_vecf", K(T64, 1, 3) + "/vecf", 3, 64, 63, 131, 40, bias="shared", y_pad=(12, 4), **RES),
    dgrad("t64_3x3s2_res_acc_fallback_chan", K(T64, 2, 3) + "/vecf+atomics", 3, 64, 63, 131, 40, 3, 2, 1, acc=1, stats="fallback", chan=True, **RES),
    dgrad("t64_7x7s4_f32_scalar_partials_chan", K(T64, 2, 3) + "/scalar+partials", 3, 48, 63, 131, 24, 7, 4, 3, y_f32=1, y_pad=(5, 3),
          stats="partials", chan=True),
    dgrad("t64_3x3s2_f32_vecf", K(T64, 2, 3) + "/vecf", 3, 56, 63, 131, 40, 3, 2, 1, y_f32=1, y_pad=(12, 4)),
    fwd("t64_1x1_bf16_scalar_acc", K(T64, 0, 3) + "/scalar", 3, 16, 16, 63, 131, 40, bias="image", acc=1, y_pad=(6, 4)),
    # ---- 128 x 96 tiles (k_igemm<4,1,1,3>: three column tiles per wave, four row waves; no LDS-staged fp32 branch, no fused reduce)
    fwd("t96_7x7s4_bias_partials", K(T96, 0, 2) + "/vec+partials", 3, 7, 8, 250, 522, 96, 7, 4, 3, bias="image", stats="partials"),
    fwd("t96_3x3s2_sigmoid_fallback", K(T96, 0, 2) + "/vec+atomics", 3, 20, 24, 125, 261, 80, 3, 2, 1, bias="shared", act=1, stats="fallback"),
    dgrad("t96_3x3_tall_acc", K(T96, 1, 2) + "/vec", 3, 72, 267, 31, 24, 3, 1, 1, acc=1),
    dgrad("t96_1x1_atomics", K(T96, 1, 2) + "/vec+atomics", 3, 96, 63, 131, 72, stats="atomics"),
    dgrad("t96_3x3s2_res_acc_atomics_chan", K(T96, 2, 2) + "/scalar+atomics", 3, 80, 63, 131, 40, 3, 2, 1, acc=1, stats="atomics", chan=True, **RES),
    dgrad("t96_7x7s4_res_partials_chan", K(T96, 2, 2) + "/scalar+partials", 3, 96, 63, 131, 24, 7, 4, 3, bias="shared", stats="partials",
          chan=True, y_pad=(5, 3), **RES),
    # ---- 128 x 160 tiles (k_igemm<4,1,1,5>)
    fwd("t160_7x7s4_bias_fallback", K(T160, 0, 2) + "/vec+atomics", 3, 7, 8, 198, 330, 160, 7, 4, 3, bias="shared", stats="fallback"),
    fwd("t160_3x3s2_sigmoid_partials", K(T160, 0, 2) + "/vec+partials", 3, 20, 24, 99, 165, 144, 3, 2, 1, bias="image", act=1, stats="partials"),
    dgrad("t160_1x1_acc", K(T160, 1, 2) + "/vec", 3, 136, 50, 83, 72, acc=1),
    dgrad("t160_1x1_atomics", K(T160, 1, 2) + "/vec+atomics", 3, 160, 50, 83, 40, stats="atomics"),
    dgrad("t160_3x3s2_res_acc_partials_chan", K(T160, 2, 2) + "/scalar+partials", 3, 144, 50, 83, 40, 3, 2, 1, acc=1, stats="partials", chan=True, **RES),
    dgrad("t160_7x7s4_res_atomics_chan", K(T160, 2, 2) + "/scalar+atomics", 3, 160, 50, 83, 24, 7, 4, 3, bias="image", stats="atomics", chan=True,
          y_pad=(5, 3), **RES),
    # ---- 128 x 128 tiles (k_igemm<2,2,2,2>: the LDS of two stages is too small for the fp32 staging tile -> scalar branch)
    fwd("t128_7x7s4_bias_partials", K(T128, 0, 2) + "/vec+partials", 3, 7, 8, 250, 522, 128, 7, 4, 3, bias="shared", stats="partials"),
    fwd("t128_3x3s2_sigmoid_atomics_two_column_tiles", K(T128, 0, 2) + "/vec+atomics", 3, 20, 24, 99, 165, 192, 3, 2, 1, bias="image", act=1,
        stats="atomics"),
    dgrad("t128_1x1_acc", K(T128, 1, 2) + "/vec", 3, 104, 63, 131, 72, acc=1),
    dgrad("t128_1x1_red", K(T128, 1, 2) + "/vec", 3, 128, 63, 131, 40, red=(4, 1, 0)),
    dgrad("t128_1x1_red_f32_stream", K(T128, 1, 2) + "/vec", 3, 176, 50, 83, 24, red=(1, 0, 1)),
    dgrad("t128_3x3s2_res_acc_fallback_chan", K(T128, 2, 2) + "/scalar+atomics", 3, 112, 63, 131, 40, 3, 2, 1, acc=1, stats="fallback", chan=True, **RES),
    dgrad("t128_7x7s4_res_partials_chan", K(T128, 2, 2) + "/scalar+partials", 3, 128, 63, 131, 24, 7, 4, 3, bias="image", stats="partials", chan=True,
          y_pad=(5, 3), **RES),
    # the sr patch scatter of encoder stage 1 at B = 8: 64 x 64 columns = 32 column tiles, one ragged row tile, 256 workgroups
    scatter("t128_scatter_k8_b8", K(T128, 0, 2) + "/vec", 8, 7, 11, 64, 8, 64),
    scatter("t128_scatter_k8_b8_acc", K(T128, 0, 2) + "/vec", 8, 7, 11, 64, 8, 64, acc=1),
    # ---- 128 x 32 tiles (k_igemm<4,1,1,1>: every launch towards <= 32 channels: the depth / seg heads, the gradient of the input image)
    fwd("t32_3x3_tall_sigmoid", K(T32, 0, 3) + "/scalar", 2, 20, 24, 23, 13, 1, 3, 1, 1, bias="shared", act=1, y_pad=(3, 2)),
    fwd("t32_1x1_f32_vecf_atomics", K(T32, 0, 3) + "/vecf+atomics", 2, 40, 40, 9, 37, 32, bias="image", stats="atomics", chan=True, y_f32=1, y_pad=(12, 4)),
    dgrad("t32_3x3_tall_vec_partials", K(T32, 1, 3) + "/vec+partials", 2, 32, 19, 17, 24, 3, 1, 1, stats="partials"),
    dgrad("t32_7x7s4_image_gradient", K(T32, 2, 3) + "/vec", 2, 8, 45, 61, 40, 7, 4, 3, acc=1),
    dgrad("t32_3x3s2_scalar", K(T32, 2, 3) + "/scalar", 2, 21, 21, 33, 24, 3, 2, 1, y_pad=(3, 1)),
    # ---- 64 x 64 tiles: stages by K depth, split-K, register epilogue
    fwd("s64_nst2_rege_bias_atomics", K(S64, 0, 2) + "/rege+atomics", 2, 72, 72, 9, 13, 80, bias="image", stats="atomics"),
    dgrad("s64_nst2_rege_acc", K(S64, 1, 2) + "/rege", 2, 72, 9, 13, 128, acc=1),
    dgrad("s64_nst2_vecf_res", K(S64, 1, 2) + "/vecf", 2, 72, 9, 13, 128, y_pad=(12, 4), **RES),
    dgrad("s64_nst2_mode2_scalar", K(S64, 2, 2) + "/scalar", 2, 40, 9, 13, 8, 3, 2, 1, y_pad=(3, 1)),
    scatter("s64_nst2_scatter_vec", K(S64, 0, 2) + "/vec", 2, 3, 5, 64, 2, 40),
    scatter("s64_nst2_scatter_scalar_acc", K(S64, 0, 2) + "/scalar", 2, 3, 5, 64, 2, 20, acc=1, y_pad=(6, 2)),
    fwd("s64_nst3_rege_sigmoid", K(S64, 0, 3) + "/rege", 2, 20, 24, 9, 13, 72, 3, 1, 1, bias="shared", act=1),
    fwd("s64_nst3_rege_partials", K(S64, 0, 3) + "/rege+partials", 2, 200, 200, 9, 13, 80, stats="partials"),
    fwd("s64_nst3_rege_atomics", K(S64, 0, 3) + "/rege+atomics", 2, 200, 200, 9, 13, 80, bias="shared", stats="atomics"),
    dgrad("s64_nst3_rege_red", K(S64, 1, 3) + "/rege", 2, 160, 9, 13, 200, red=(2, 1, 0)),
    dgrad("s64_nst3_vecf_res_acc", K(S64, 1, 3) + "/vecf", 2, 72, 9, 13, 160, acc=1, y_pad=(12, 4), **RES),
    dgrad("s64_nst3_mode2_vec_chanless", K(S64, 2, 3) + "/rege", 2, 72, 9, 13, 24, 3, 2, 1),
    fwd("s64_nst4_rege_atomics_3x3s2", K(S64, 0, 4) + "/rege+atomics", 2, 40, 40, 17, 25, 80, 3, 2, 1, bias="shared", stats="atomics"),
    dgrad("s64_nst4_rege_3x3_tall", K(S64, 1, 4) + "/rege", 2, 72, 23, 13, 40, 3, 1, 1),
    dgrad("s64_nst4_mode2_vecf", K(S64, 2, 4) + "/vecf", 2, 72, 17, 25, 40, 3, 2, 1, y_f32=1, y_pad=(12, 4)),
    # deep K on a grid of more than 256 small tiles stays on the plain four-stage kernel
    fwd("s64_nst4_deep_k_many_tiles", K(S64, 0, 4) + "/rege", 2, 512, 512, 65, 65, 72),
    fwd("s64_splitk_sr_conv_vec_atomics", K(S64, 0, 2, 4) + "/vec+atomics", 2, 64, 64, 24, 40, 64, 8, 8, 0, bias="shared", stats="atomics"),
    fwd("s64_splitk_vecf_res", K(S64, 0, 2, 4) + "/vecf", 2, 640, 640, 5, 7, 160, bias="shared", y_pad=(12, 4), **RES),
    fwd("s64_splitk_vecf_res_atomics_chan", K(S64, 0, 2, 4) + "/vecf+atomics", 2, 640, 640, 5, 7, 160, bias="shared", stats="atomics", chan=True,
        y_pad=(12, 4), **RES),
    fwd("s64_splitk_scalar_partials", K(S64, 0, 2, 4) + "/scalar+partials", 2, 520, 520, 5, 7, 80, stats="partials", y_f32=1, y_pad=(5, 3)),
    dgrad("s64_splitk_mode1_vec_acc", K(S64, 1, 2, 4) + "/vec", 2, 64, 13, 9, 64, 3, 1, 1, acc=1),
    dgrad("s64_splitk_mode2_vecf", K(S64, 2, 2, 4) + "/vecf", 2, 72, 9, 13, 64, 3, 2, 1, y_f32=1, y_pad=(12, 4)),
    # ---- hand-offs to the other kernel families (their own tile choices have their own tests)
    fwd("halo_3x3", "conv3x3_halo", 2, 20, 24, 9, 40, 80, 3, 1, 1, bias="shared", stats="atomics"),
    fwd("persistent_3x3", "conv3x3p", 3, 8, 8, 128, 256, 64, 3, 1, 1),
    fwd("narrow_pointwise", "pw_narrow", 2, 512, 512, 8, 12, 64, y_pad=(12, 4), **RES),
    dgrad("wide_pointwise", "pw_wide_plain", 2, 256, 9, 13, 64, x_pad=(0, 0)),
]
CASES = {c["name"]: c for c in ROUTE_CASES}
assert len(CASES) == len(ROUTE_CASES)


def label_parts(label):
    """-> (tile, mode, stages, split-K groups, epilogue branch, sums) of a generic-kernel label, None for a hand-off"""
    m = re.fullmatch(r"k_igemm<(\d,\d,\d,\d),MODE=(\d),NST=(\d),KG=(\d)>/(rege|vecf|vec|scalar)(\+partials|\+atomics)?", label)
    return None if m is None else (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5), m.group(6) or "")


def tile_rows(label):
    t = label_parts(label)[0].split(",")
    return 32 * int(t[0]) * int(t[2])


def partial_capacity(c):
    """floats of the stats_partial buffer of a case: the documented size, or one float less than the tile that runs needs"""
    G16, P = c["N"] // 16, c["OH"] * c["OW"]
    if c["stats"] == "fallback":
        return c["B"] * cdiv(P, tile_rows(c["label"])) * G16 * 2 - 1
    if c["label"] == "conv3x3p":
        return c["B"] * cdiv(c["OW"], 32) * cdiv(c["OH"], 16) * 8 * G16 * 2
    return c["B"] * cdiv(P, 64) * G16 * 2


def y_geometry(c):
    """(output image height, width, channels of the slice the launch writes)"""
    if c["scatter"]:
        pk, pc = c["scatter"]
        return c["OH"] * pk, c["OW"] * pk, pc
    return c["OH"], c["OW"], c["N"]


def descriptor(lib, c, ptr=None):
    """The crd_conv_desc of a case.  ptr: name -> device address (x, w, y, bias, res, res_scale, stats, partial, chan, red_x, red_stats,
    red_gamma, red_beta, red_r); without it every pointer is one 256-byte aligned host address that nobody reads."""
    p = (lambda n: A) if ptr is None else (lambda n: ptr[n])
    d = lib.ConvDesc()
    d.x, d.x_ld, d.x_coff = p("x"), c["Cx"] + c["x_pad"][0], c["x_pad"][1]
    d.B, d.IH, d.IW, d.Cin = c["B"], c["IH"], c["IW"], c["Cx"]
    d.w, d.Cout, d.KH, d.KW, d.stride, d.pad, d.OH, d.OW = p("w"), c["N"], c["k"], c["k"], c["stride"], c["pad"], c["OH"], c["OW"]
    d.gather_mode = c["gather"]
    yc = y_geometry(c)[2]
    d.y, d.y_ld, d.y_coff, d.y_f32 = p("y"), yc + c["y_pad"][0], c["y_pad"][1], c["y_f32"]
    if c["scatter"]:
        d.out_mode, d.patch_k, d.patch_c = 1, c["scatter"][0], c["scatter"][1]
    if c["bias"]:
        d.bias, d.bias_bstride = p("bias"), c["N"] if c["bias"] == "image" else 0
    d.act = c["act"]
    if c["res"]:
        d.res, d.res_ld = p("res"), yc + 4
    if c["res_scale"]:
        d.res_scale = p("res_scale")
    d.accumulate = c["acc"]
    if c["stats"]:
        d.stats = p("stats")
        if c["stats"] != "atomics":
            d.stats_partial, d.stats_partial_capacity = p("partial"), partial_capacity(c)
    if c["chan"]:
        d.chan_sums = p("chan")
    if c["red"]:
        gmul, act, xf32 = c["red"]
        d.red_x, d.red_x_ld, d.red_gmul, d.red_act, d.red_x_f32 = p("red_x"), c["N"] + 8, gmul, act, xf32
        d.red_stats, d.red_gamma, d.red_beta, d.red_r = p("red_stats"), p("red_gamma"), p("red_beta"), p("red_r")
    return d


# ------------------------------------------------------------------------------------------ operands, float64 reference, bound
def bf(t):
    """round to bf16 (through fp32, as the operands are made), in the dtype of t"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def operands(c):
    """Deterministic operands of a case on the CPU: bf16-representable x [B][Cx][IH][IW] (the padding channels carry data: their weights
    are zero) and w [N][k*k][Cx] (the descriptor's layout: tap-major, channel innermost, for both gather modes), fp32 epilogue inputs."""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    B, Cx, N, taps = c["B"], c["Cx"], c["N"], c["k"] * c["k"]
    o = {"x": bf(torch.randn(B, Cx, c["IH"], c["IW"], generator=g))}
    w = torch.randn(N, taps, Cx, generator=g) / (taps * c["Cx_ref"]) ** 0.5
    w[:, :, c["Cx_ref"]:] = 0
    o["w"] = bf(w)
    YH, YW, yc = y_geometry(c)
    if c["bias"]:
        o["bias"] = torch.randn(B if c["bias"] == "image" else 1, N, generator=g) * 0.3
    if c["res"]:
        o["res"] = torch.randn(B, YH, YW, yc, generator=g)
    if c["res_scale"]:
        o["res_scale"] = torch.tensor([1.25, 0.0, -0.5, 0.75, 1.0, 0.3, 2.0, 0.6])[:B].clone()        # one sample's branch is switched off
    if c["acc"]:
        old = torch.randn(B, YH, YW, yc, generator=g)
        o["old"] = old if c["y_f32"] else bf(old)
    if c["red"]:
        gmul, act, xf32 = c["red"]
        rx = torch.randn(B, c["OH"] * c["OW"], N, generator=g) * 1.3 + 0.2
        o["red_x"] = rx if xf32 else bf(rx)
        o["red_gamma"], o["red_beta"] = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    return o


def gemm(c, o, dtype):
    """(v, a): the convolution of the case as [B][OH*OW][N] in `dtype`, bias included, and the same convolution of |x| and |w| plus
    |bias| (the magnitude an accumulation-order error is relative to)."""
    x, w = o["x"].to(dtype), o["w"].to(dtype)
    B, Cx, N, k, s, p = c["B"], c["Cx"], c["N"], c["k"], c["stride"], c["pad"]
    out = []
    for xx, ww in ((x, w), (x.abs(), w.abs())):
        if c["gather"] == 0:
            cols = F.unfold(xx, k, padding=p, stride=s)                           # [B][Cx * k * k][L], channel-major rows
            assert cols.shape[2] == c["OH"] * c["OW"], (c["name"], cols.shape)
            w2 = ww.view(N, k * k, Cx).permute(0, 2, 1).reshape(N, Cx * k * k)
            v = (w2 @ cols).transpose(1, 2)
        else:
            # y[iy, ix] += w[ky, kx] x[(iy + p - ky) / s, (ix + p - kx) / s]: a transposed convolution, taps not mirrored
            wt = ww.view(N, k, k, Cx).permute(3, 0, 1, 2).contiguous()
            op = (c["OH"] - ((c["IH"] - 1) * s - 2 * p + k), c["OW"] - ((c["IW"] - 1) * s - 2 * p + k))
            v = F.conv_transpose2d(xx, wt, stride=s, padding=p, output_padding=op)
            assert v.shape[2:] == (c["OH"], c["OW"]), (c["name"], v.shape)
            v = v.reshape(B, N, -1).transpose(1, 2)
        out.append(v.contiguous())
    v, a = out
    if c["bias"]:
        bias = o["bias"].to(dtype).view(-1, 1, N)
        v, a = v + bias, a + bias.abs()
    return v, a


def to_image(c, t):
    """[B][OH*OW][N] -> the output image [B][YH][YW][channels] (the patch scatter rearranges columns into pixels)"""
    B, OH, OW = c["B"], c["OH"], c["OW"]
    if not c["scatter"]:
        return t.reshape(B, OH, OW, c["N"])
    pk, pc = c["scatter"]
    return t.reshape(B, OH, OW, pk, pk, pc).permute(0, 1, 3, 2, 4, 5).reshape(B, OH * pk, OW * pk, pc)


def epilogue(c, o, v, a, dtype, as_kernel=False):
    """(stored, bound) as output images: what the launch must leave in y from the accumulator value v, and the elementwise error bound
    of the stored value.  The kernel's documented rounding points -- bf16 of the biased / sigmoid result, res + scale * bf16(v), the
    accumulate as a read-modify-write in y's type -- are where the bound's terms come from; the float64 reference itself keeps v
    UNROUNDED in front of the residual / accumulate (as_kernel = False), because a reference that rounded v as well could land on the
    other bf16 neighbour of a value near a rounding boundary, a full ulp (up to 2^-7 relative) from the kernel's, which the bound below
    has no term for.  as_kernel = True applies the roundings, for the float32 emulation of the kernel.

    Bound (outputs without sigmoid; u = 2^-8, the rounding to bf16; e = Ktot 2^-23 a, fp32 accumulation of Ktot terms in any order):
      plain store                     |got - v| <= u |v| + e        (an fp32 output without residual is not rounded to bf16: u = 2^-23 there)
      accumulate (bf16)               got = bf16(bf16(v) + old) or bf16(v + old):  u |v| + e  +  u |stored|
      residual / fp32 read-modify-write   got = res + scale * bf16(v) (+ old) in fp32:  |scale| (u |v| + e)  +  2^-22 (|res| + |scale v| + |old|)
        (three fp32 roundings of at most 2^-24 each on partial results no larger than |res| + |scale v| + |old|: <= 1.5 * 2^-23 of that)
    """
    Ktot = c["k"] * c["k"] * c["Cx"]
    u, e = 2.0 ** (-23 if c["y_f32"] and not c["res"] else -8), Ktot * 2.0 ** -23 * a
    if c["act"]:
        v = torch.sigmoid(v)
    bound = u * v.abs() + e
    v, bound = to_image(c, v), to_image(c, bound)
    old = o["old"].to(dtype) if c["acc"] else None
    if c["res"]:
        scale = o["res_scale"].to(dtype).view(-1, 1, 1, 1) if c["res_scale"] else 1.0
        t = scale * (bf(v) if as_kernel else v)
        stored = o["res"].to(dtype) + t
        mag = o["res"].to(dtype).abs() + abs(t)
        bound = abs(scale) * bound
        if old is not None:
            stored, mag = stored + old, mag + old.abs()
        bound = bound + 2.0 ** -22 * mag
    elif c["y_f32"]:
        stored = v
        if old is not None:
            stored = stored + old
            bound = bound + 2.0 ** -22 * (v.abs() + old.abs())
    else:
        stored = v
        if old is not None:
            stored = (bf(v) if as_kernel else v) + old
            bound = bound + u * stored.abs()
    return stored, bound


@functools.lru_cache(maxsize=2)
def reference(name):
    """(operands, stored, bound) of a case in float64 -- treat as read-only.  (Each case has one consumer per process; only the last
    two are kept: the large ones hold 50 MB.)"""
    c = CASES[name]
    o = operands(c)
    v, a = gemm(c, o, torch.float64)
    stored, bound = epilogue(c, o, v, a, torch.float64)
    return o, stored, bound


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5


def reduce_reference(c, o, dx):
    """float64 sums of the reduce phase of a GroupNorm (+ GELU) backward (crd_gn_bwd_reduce) on the gradient dx [B][P][N] the launch
    stored: per channel (sum g, sum g xhat), then per group the gamma-weighted sums of its channels; and the raw slab sums of the
    GroupNorm's input that the launch is given."""
    gmul, act, _ = c["red"]
    B, N = c["B"], c["N"]
    x = o["red_x"].double()
    P = x.shape[1]
    slab = torch.stack([x.view(B, P, N // 16, 16).sum((1, 3)), (x * x).view(B, P, N // 16, 16).sum((1, 3))], -1)      # [B][N/16][2]
    grp = slab.view(B, N // (16 * gmul), gmul, 2).sum(2)
    cnt = P * 16 * gmul
    mean = grp[..., 0] / cnt
    rstd = (grp[..., 1] / cnt - mean * mean + 1e-5).rsqrt()
    mean, rstd = (t.repeat_interleave(16 * gmul, 1).view(B, 1, N) for t in (mean, rstd))
    xh = (x - mean) * rstd
    g = dx.double()
    if act:
        g = g * gelu_grad(xh * o["red_gamma"].double() + o["red_beta"].double())
    chan = torch.stack([g.sum(1), (g * xh).sum(1)], -1)                                     # [B][N][2]
    grp_r = (chan * o["red_gamma"].double().view(1, N, 1)).view(B, N // (16 * gmul), 16 * gmul, 2).sum(2)
    return slab, torch.cat([chan.reshape(-1), grp_r.reshape(-1)])


# --------------------------------------------------------------------------------------------------------------- route table
@pytest.mark.parametrize("name", list(CASES))
def test_route_of_every_case(built, name):
    assert built.conv_route(descriptor(built, CASES[name])) == CASES[name]["label"]


def test_route_table_covers_every_route_of_the_decision_function():
    labels = {c["label"] for c in ROUTE_CASES}
    assert {"conv3x3_halo", "conv3x3p", "pw_narrow", "pw_wide_plain"} <= labels
    parts = {label_parts(x) for x in labels} - {None}
    reached = {p[:4] for p in parts}
    # every instantiation the launch switch holds (csrc/igemm.hip: CRD_IGEMM_TILES), in every gather MODE
    tiles = [(S64, 2, 1), (S64, 3, 1), (S64, 4, 1), (S64, 2, 4), (T32, 3, 1), (T64, 3, 1), (T96, 2, 1), (T160, 2, 1), (T128, 2, 1)]
    assert reached == {(t, mode, nst, kg) for t, nst, kg in tiles for mode in (0, 1, 2)}
    # the register epilogue at every stage count; each epilogue branch on each tile where the kernel's own condition allows it
    # (conv_common.h: conv_use_vecf -- no LDS-staged fp32 branch on the 96-, 128- and 160-column tiles)
    branches = {}
    for t, _, _, kg, epi, _ in parts:
        branches.setdefault((t, kg), set()).add(epi)
    assert branches == {(S64, 1): {"rege", "vec", "vecf", "scalar"}, (S64, 4): {"vec", "vecf", "scalar"}, (T32, 1): {"vec", "vecf", "scalar"},
                        (T64, 1): {"vec", "vecf", "scalar"}, (T96, 1): {"vec", "scalar"}, (T160, 1): {"vec", "scalar"},
                        (T128, 1): {"vec", "scalar"}}
    assert {(nst, epi) for t, _, nst, kg, epi, _ in parts if t == S64 and kg == 1 and epi == "rege"} == {(2, "rege"), (3, "rege"), (4, "rege")}
    # both statistics exits on every tile, and the capacity fallback on every large tile
    for t in (S64, T32, T64, T96, T160, T128):
        assert {s for tt, _, _, _, _, s in parts if tt == t} == {"", "+partials", "+atomics"}, t
    for t in (T64, T96, T160, T128):
        assert any(c["stats"] == "fallback" and label_parts(c["label"])[0] == t for c in ROUTE_CASES), t


def test_large_tile_cases_cover_every_epilogue_option():
    """What tests/test_gpu_conv_routes.py promises for each large tile, as far as crd_conv_igemm accepts it there."""
    for t in (T64, T96, T160, T128):
        cs = [c for c in ROUTE_CASES if (label_parts(c["label"]) or [None])[0] == t]
        have = lambda pred: any(pred(c) for c in cs)                                                    # noqa: E731
        assert have(lambda c: c["bias"] == "shared") and have(lambda c: c["bias"] == "image") and have(lambda c: c["act"] == 1), t
        assert have(lambda c: not c["y_f32"] and not c["acc"]) and have(lambda c: not c["y_f32"] and c["acc"]), t
        assert have(lambda c: c["res"] and c["res_scale"] and c["acc"]), t
        assert {c["stats"] for c in cs} >= {"partials", "atomics", "fallback"} and have(lambda c: c["chan"]), t
        assert have(lambda c: c["k"] == 7 and c["stride"] == 4 and c["gather"] == 0) and have(lambda c: c["k"] == 7 and c["gather"] == 1), t
        assert have(lambda c: c["k"] == 3 and c["stride"] == 2 and c["gather"] == 0) and have(lambda c: c["k"] == 3 and c["stride"] == 2 and c["gather"] == 1), t
        assert have(lambda c: c["k"] * c["k"] * c["Cx"] % 64 != 0) and have(lambda c: c["Cx_ref"] < c["Cx"]), t
        assert (t not in (T64, T128)) or have(lambda c: c["red"]), t
    assert sum(1 for c in ROUTE_CASES if c["scatter"] and c["B"] == 8 and c["N"] == 4096) == 2
    for c in ROUTE_CASES:           # operands sit inside wider buffers wherever the branch allows it
        if label_parts(c["label"]):
            assert c["x_pad"][0] > 0 and c["x_pad"][1] > 0, c["name"]
            assert c["y_pad"][0] > 0 and c["y_pad"][1] > 0, c["name"]


# ---------------------------------------------------------------------------------------------------------- threshold pairs
def _generic(lib, **kw):
    """a 5 x 5 / stride 1 / pad 2 layer (no hand-off takes it) with 64 input channels"""
    base = dict(KH=5, KW=5, pad=2, B=3, IH=63, IW=131, OH=63, OW=131)
    base.update(kw)
    return lib.conv_route(conv_desc(lib, **base))


def _pointwise(lib, Cin, **kw):
    return lib.conv_route(conv_desc(lib, **dict(dict(Cin=Cin, x_ld=Cin, Cout=72, y_ld=72), **kw)))


def test_threshold_192_big_tiles(built):
    # 3 x 63 = 189 / 3 x 64 = 192 tiles of 128 rows: one pixel apart; and 2 / 3 samples of 64 row tiles
    px = lambda n, B=3: _generic(built, IH=1, IW=n, OH=1, OW=n, B=B, pad=2)                            # noqa: E731
    assert px(63 * 128) == K(S64, 0, 4) + "/rege" and px(63 * 128 + 1) == K(T64, 0, 3) + "/vec"
    assert px(8192, B=2) == K(S64, 0, 2, 4) + "/vec" and px(8192, B=3) == K(T64, 0, 3) + "/vec"
    # ... counted in column tiles as well: 33 row tiles x 3 samples x 1 / 2 column tiles
    assert _generic(built, IH=50, IW=83, OH=50, OW=83, Cout=128, y_ld=128) == K(S64, 0, 4) + "/rege"
    assert _generic(built, IH=50, IW=83, OH=50, OW=83, Cout=136, y_ld=136) == K(T160, 0, 2) + "/vec"


def test_threshold_stage_choice_by_k_slabs(built):
    """2 / 3, 4 / 5 and 7 / 8 slabs of 64: one 8-channel granule apart"""
    got = [_pointwise(built, Cin) for Cin in (128, 136, 256, 264, 448, 456)]
    assert got == [K(S64, 0, 2) + "/rege", K(S64, 0, 3) + "/rege", K(S64, 0, 3) + "/rege", K(S64, 0, 4) + "/rege", K(S64, 0, 4) + "/rege",
                   K(S64, 0, 2, 4) + "/vec"]


def test_threshold_256_small_tiles_for_split_k(built):
    """64 row tiles x 4 samples = 256 workgroups still split K; one pixel (or one sample) more and the launch covers the chip"""
    f = lambda n, B: _pointwise(built, 520, B=B, IH=1, IW=n, OH=1, OW=n, Cout=64, y_ld=64, y_f32=1)        # noqa: E731
    assert f(4096, 4) == K(S64, 0, 2, 4) + "/vecf" and f(4097, 4) == K(S64, 0, 4) + "/vecf"
    assert f(4096, 5) == K(S64, 0, 4) + "/vecf"


@pytest.mark.parametrize("cout,below,above", [(32, K(T32, 0, 3), K(T64, 0, 3)), (64, K(T64, 0, 3), K(T96, 0, 2)), (96, K(T96, 0, 2), K(T128, 0, 2)),
                                               (128, K(T128, 0, 2), K(T160, 0, 2)), (160, K(T160, 0, 2), K(T128, 0, 2))])
def test_threshold_cout_boundaries(built, cout, below, above):
    got = [_generic(built, Cout=n, y_ld=168, B=6) for n in (cout, cout + 1)]
    assert got == [below + ("/vec" if cout % 8 == 0 else "/scalar"), above + "/scalar"]


# ------------------------------------------------------------------------------------------------------------ Python mirror
GRID_COUT = [8, 24, 32, 33, 40, 64, 65, 72, 96, 97, 104, 128, 129, 136, 160, 161, 168, 256, 320]
GRID_PIX_B = [(63 * 128, 3), (63 * 128 + 1, 3), (8192, 2), (8192, 3), (4150, 3), (4096, 3), (4097, 3), (24576, 1), (24577, 1), (117, 2), (117, 200),
              (1, 191), (1, 192), (1, 96), (1, 97)]


def test_plan_values_igemm_tile_agrees_with_the_library(built):
    from camradepth_amd.plan_values import igemm_tile
    for cout in GRID_COUT:
        for ohw, B in GRID_PIX_B:
            label = _generic(built, IH=1, IW=ohw, OH=1, OW=ohw, B=B, Cout=cout, y_ld=320)
            assert label.split(",MODE=")[0] + ">" == igemm_tile(cout, ohw, B), (cout, ohw, B, label)


def test_plan_values_fused_reduce_tile_ok_agrees_with_the_library(built):
    from camradepth_amd.plan_values import fused_reduce_tile_ok
    L = built.load()
    for cout in GRID_COUT:
        if cout % 8:
            continue
        for ohw, B in GRID_PIX_B:
            d = conv_desc(built, **dict(RED, IH=1, IW=ohw, OH=1, OW=ohw, B=B, Cout=cout, y_ld=320, red_x_ld=320))
            buf = C.create_string_buffer(96)
            rc = L.crd_conv_igemm_route(C.byref(d), buf, len(buf))
            assert rc in (0, -2) and (rc == 0) == fused_reduce_tile_ok(cout, ohw, B), (cout, ohw, B, rc, L.crd_last_error())


# --------------------------------------------------------------------------------------------------------- production routes
def _plan_labels(lib, plan):
    out = {}
    for op in list(plan.fwd) + list(plan.bwd):
        if op.name == "crd_conv_igemm":
            out.setdefault(lib.conv_route(op.args[0]._obj), op.meta["shape"])
    return out


@pytest.mark.parametrize("config", ["train_b8_256x416", "train_seg_b8_256x416", "eval_b1_416x800"])
def test_every_route_of_the_model_plan_has_a_case(built, config):
    """The training step at the benchmark's size and the full-resolution inference configuration (tools/plan_fingerprint.py: build):
    every label a crd_conv_igemm descriptor of the forward and backward lists resolves to is one that ROUTE_CASES runs."""
    spec = importlib.util.spec_from_file_location(
        "plan_fingerprint_routes", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "plan_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    plan = {"train_b8_256x416": lambda: fp.build(8, 256, 416), "train_seg_b8_256x416": lambda: fp.build(8, 256, 416, supervised_seg=True),
            "eval_b1_416x800": lambda: fp.build(1, 416, 800, train=False)}[config]()
    labels = _plan_labels(built, plan)
    assert len(labels) >= 10
    missing = {k: v for k, v in labels.items() if k not in {c["label"] for c in ROUTE_CASES}}
    assert not missing, f"routes of the model without a case in ROUTE_CASES: {missing}"


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("i", [0, 1, 4, 6, 8, 9, 10, 12, 14, 16, 18, 19, 20])
def test_route_query_refuses_what_the_entry_refuses(built, i):
    mut, status, words = IGEMM[i]
    L = built.load()
    d = None if mut is None else conv_desc(built, **mut)
    buf = C.create_string_buffer(96)
    rc = L.crd_conv_igemm_route(None if d is None else C.byref(d), buf, len(buf))
    msg = L.crd_last_error().decode()
    assert rc == status and msg.startswith(words), (mut, rc, msg)
    assert L.crd_conv_igemm(None if d is None else C.byref(d), None) == rc and L.crd_last_error().decode() == msg


def test_route_query_needs_room_for_the_label(built):
    L = built.load()
    d = conv_desc(built)
    buf = C.create_string_buffer(96)
    for cap in (0, 1, 20, len("k_igemm<2,2,1,1,MODE=0,NST=2,KG=1>/rege")):
        assert L.crd_conv_igemm_route(C.byref(d), buf, cap) == -1
        assert L.crd_last_error().decode().startswith("crd_conv_igemm_route: ")
    assert L.crd_conv_igemm_route(C.byref(d), None, 96) == -1
    assert L.crd_conv_igemm_route(C.byref(d), buf, len("k_igemm<2,2,1,1,MODE=0,NST=2,KG=1>/rege") + 1) == 0
    assert buf.value == b"k_igemm<2,2,1,1,MODE=0,NST=2,KG=1>/rege"


def test_route_query_follows_the_tuning_switches_and_counts_nothing(built):
    L = built.load()
    d = conv_desc(built)
    n0 = L.crd_tune_igemm_reg_epilogue(-1)
    prev = L.crd_tune_igemm_reg_epilogue(0)
    try:
        assert built.conv_route(d) == K(S64, 0, 2) + "/vec"
    finally:
        L.crd_tune_igemm_reg_epilogue(prev)
    assert built.conv_route(d) == K(S64, 0, 2) + "/rege"
    assert L.crd_tune_igemm_reg_epilogue(-1) == n0
    narrow = descriptor(built, CASES["narrow_pointwise"])
    prev = L.crd_tune_pw_narrow(0)
    try:
        assert built.conv_route(narrow) == K(S64, 0, 2, 4) + "/vecf"
    finally:
        L.crd_tune_pw_narrow(prev)
    assert built.conv_route(narrow) == "pw_narrow"


# ------------------------------------------------------------------------------------------- the bound, before it costs a GPU run
@pytest.mark.parametrize("name", list(CASES))
def test_float32_recomputation_stays_inside_the_bound(name):
    """The float64 reference recomputed in float32 (other summation order, fp32 epilogue arithmetic) must pass the elementwise bound the
    GPU test applies: a bound that an honest fp32 implementation misses is too tight."""
    c = CASES[name]
    o, stored, bound = reference(name)
    v32, a32 = gemm(c, o, torch.float32)
    got, _ = epilogue(c, o, v32, a32, torch.float32, as_kernel=True)
    if not c["y_f32"]:
        got = bf(got)
    assert torch.isfinite(stored).all() and torch.isfinite(bound).all() and (bound > 0).all()
    if c["act"]:
        return                      # sigmoid cases use the project's relative pair, not this bound
    worst = ((got.double() - stored).abs() / bound).max().item()
    assert worst <= 1.0, f"{name}: float32 recomputation at {worst:.3f} of the bound"
