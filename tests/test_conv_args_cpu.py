"""Argument checks of the pointwise / patch GEMM entry points -- crd_conv_igemm, crd_gn_conv, crd_gn_conv2, crd_gn_bwd_conv -- without a
GPU: a table of descriptor mutations, each with the status it must return (-1 invalid, -2 unsupported) and the leading words of
crd_last_error().  Every entry is refused before any launch, so the pointers are host addresses nobody reads.  The table pins the
checks, their order and their messages across changes to how the kernel argument block is built from the descriptor."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


_BUF = C.create_string_buffer(512)
A = (C.addressof(_BUF) + 255) // 256 * 256          # a 16-byte aligned non-NULL host address
BIG = 1 << 13                                       # 8192 x 8192 pixels of 64 channels: past 32-bit byte offsets


def conv_desc(lib, **kw):
    """a valid 64 -> 64 pointwise problem on 8 x 8 pixels, then the mutation"""
    d = lib.ConvDesc()
    d.x = d.w = d.y = A
    d.B, d.IH, d.IW, d.OH, d.OW = 1, 8, 8, 8, 8
    d.Cin = d.x_ld = d.Cout = d.y_ld = 64
    d.KH = d.KW = d.stride = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def gn_input(lib, **kw):
    n = lib.GnInput()
    n.stats = n.gamma = n.beta = A
    n.gmul = 1
    for k, v in kw.items():
        setattr(n, k, v)
    return n


def gn_bwd_input(lib, **kw):
    n = lib.GnBwdInput()
    n.gx = n.stats = n.gamma = n.beta = n.r = A
    n.gx_ld, n.gmul = 64, 1
    for k, v in kw.items():
        setattr(n, k, v)
    return n


RED = dict(red_x=A, red_stats=A, red_gamma=A, red_beta=A, red_r=A, red_gmul=1, red_x_ld=64)      # a complete fused-reduce block

# (descriptor mutation, status, leading words of the message)
IGEMM = [
    (None, -1, "crd_conv_igemm: null pointer"),
    (dict(x=None), -1, "crd_conv_igemm: null pointer"),
    (dict(w=None), -1, "crd_conv_igemm: null pointer"),
    (dict(y=None), -1, "crd_conv_igemm: null pointer"),
    (dict(Cin=68, x_ld=68), -1, "crd_conv_igemm: Cin/x_ld/x_coff must be multiples of 8 (got 68/68/0)"),
    (dict(x_coff=4), -1, "crd_conv_igemm: Cin/x_ld/x_coff must be multiples of 8 (got 64/64/4)"),
    (dict(stride=0), -1, "crd_conv_igemm: bad dims"),
    (dict(B=0), -1, "crd_conv_igemm: bad dims"),
    (dict(res=A), -1, "crd_conv_igemm: residual epilogue needs fp32 output"),
    (dict(stats=A, Cout=72, y_ld=72), -1, "crd_conv_igemm: stats need Cout % 16 == 0"),
    (dict(out_mode=1, patch_k=2, patch_c=8), -1, "crd_conv_igemm: bad patch-scatter dims"),
    (dict(out_mode=1, patch_k=0, patch_c=64), -1, "crd_conv_igemm: bad patch-scatter dims"),
    (dict(IH=BIG, IW=BIG, OH=BIG, OW=BIG), -2, "crd_conv_igemm: image or weight tensor too large for 32-bit byte offsets"),
    (dict(Cin=1 << 15, x_ld=1 << 15, Cout=1 << 15), -2, "crd_conv_igemm: image or weight tensor too large for 32-bit byte offsets"),
    (dict(chan_sums=A), -2, "crd_conv_igemm: chan_sums needs stats"),
    (dict(chan_sums=A, stats=A), -2, "crd_conv_igemm: chan_sums needs stats"),             # ... and an fp32 / residual output
    (dict(red_x=A), -1, "crd_conv_igemm: incomplete fused-reduce arguments"),
    (dict(RED, red_r=None), -1, "crd_conv_igemm: incomplete fused-reduce arguments"),
    (dict(RED, red_gmul=3), -1, "crd_conv_igemm: incomplete fused-reduce arguments"),
    (dict(RED, y_f32=1), -2, "crd_conv_igemm: the fused GroupNorm-backward reduce needs"),
    (dict(RED, y_coff=4), -2, "crd_conv_igemm: the fused GroupNorm-backward reduce needs"),        # vec_ok comes from the builder
]

GN_CONV = [
    (None, {}, -1, "crd_gn_conv: null pointer"),
    (dict(x=None), {}, -1, "crd_gn_conv: null pointer"),
    ({}, None, -1, "crd_gn_conv: null pointer"),
    ({}, dict(gamma=None), -1, "crd_gn_conv: null pointer"),
    (dict(Cin=72, x_ld=72), {}, -1, "crd_gn_conv: Cin must be a multiple of 16"),
    (dict(x_coff=4), {}, -1, "crd_gn_conv: Cin must be a multiple of 16"),
    (dict(KH=2), {}, -1, "crd_gn_conv: bad dims"),
    (dict(KH=3, KW=3, pad=1), {}, -2, "crd_gn_conv: pointwise or non-overlapping patch convolutions only"),       # overlapping taps
    (dict(KH=2, KW=2, stride=2), {}, -2, "crd_gn_conv: pointwise or non-overlapping patch convolutions only"),   # IH != OH * stride
    (dict(out_mode=1, patch_k=1, patch_c=64), {}, -2, "crd_gn_conv: pointwise or non-overlapping patch convolutions only"),
    ({}, dict(gmul=3), -1, "crd_gn_conv: bad GroupNorm arguments"),
    ({}, dict(act=2), -1, "crd_gn_conv: bad GroupNorm arguments"),
    (dict(res=A), {}, -1, "crd_gn_conv: residual epilogue needs fp32 output"),
    (dict(stats=A, Cout=72, y_ld=72), {}, -1, "crd_gn_conv: stats need Cout % 16 == 0"),
    (dict(red_x=A), {}, -2, "crd_gn_conv: no fused backward reduce / partial statistics here"),
    (dict(stats=A, stats_partial=A), {}, -2, "crd_gn_conv: no fused backward reduce / partial statistics here"),
    (dict(Cin=4112, x_ld=4112), {}, -2, "crd_gn_conv: tensor too large for 32-bit byte offsets"),
    (dict(IH=BIG, IW=BIG, OH=BIG, OW=BIG), {}, -2, "crd_gn_conv: tensor too large for 32-bit byte offsets"),
    ({}, dict(xn=A + 8, xn_ld=64), -1, "crd_gn_conv: xn rows must be 16-byte aligned"),
    ({}, dict(xn=A, xn_ld=68), -1, "crd_gn_conv: xn rows must be 16-byte aligned"),
    (dict(chan_sums=A), {}, -2, "crd_gn_conv: chan_sums needs stats"),
    (dict(x=A + 8), {}, -1, "crd_gn_conv: x rows must be 16-byte aligned"),
]

GN_CONV2 = [      # (mutation of problem 0, of its GroupNorm, of problem 1, of its GroupNorm); both problems start behind an fp32 stream
    (None, {}, {}, {}, -1, "crd_gn_conv: null pointer"),
    ({}, {}, None, {}, -1, "crd_gn_conv: null pointer"),
    ({}, {}, dict(Cin=72, x_ld=72), {}, -1, "crd_gn_conv: Cin must be a multiple of 16"),
    ({}, {}, {}, dict(gmul=3), -1, "crd_gn_conv: bad GroupNorm arguments"),
    ({}, {}, dict(KH=3, KW=3, pad=1), {}, -2, "crd_gn_conv: pointwise or non-overlapping patch convolutions only"),
    ({}, {}, dict(B=2), {}, -2, "crd_gn_conv2: two problems of one batch"),
    ({}, dict(x_f32=0), {}, {}, -2, "crd_gn_conv2: two problems of one batch"),
    ({}, {}, {}, dict(act=1), -2, "crd_gn_conv2: two problems of one batch"),
    ({}, {}, dict(IH=128, IW=128, OH=128, OW=128, Cout=128, y_ld=128), {}, -2, "crd_gn_conv2: both problems must take the 64 x 64 tiles"),
]

GN_BWD = [
    (None, {}, -1, "crd_gn_bwd_conv: null pointer"),
    ({}, None, -1, "crd_gn_bwd_conv: null pointer"),
    ({}, dict(r=None), -1, "crd_gn_bwd_conv: null pointer"),
    ({}, dict(gx=None), -1, "crd_gn_bwd_conv: null pointer"),
    (dict(Cin=72, x_ld=72), {}, -1, "crd_gn_bwd_conv: Cin must be a multiple of 16"),
    ({}, dict(gx_ld=68), -1, "crd_gn_bwd_conv: Cin must be a multiple of 16"),
    (dict(B=0), {}, -1, "crd_gn_bwd_conv: bad dims"),
    (dict(KH=2, KW=2, stride=2, IH=16, IW=16), {}, -2, "crd_gn_bwd_conv: pointwise data gradients only"),       # not pointwise
    (dict(pad=1), {}, -2, "crd_gn_bwd_conv: pointwise data gradients only"),
    ({}, dict(gmul=3), -1, "crd_gn_bwd_conv: bad GroupNorm arguments"),
    (dict(y_f32=1), {}, -1, "crd_gn_bwd_conv: bf16 output without residual / activation / channel sums"),
    (dict(res=A), {}, -1, "crd_gn_bwd_conv: bf16 output without residual / activation / channel sums"),
    (dict(chan_sums=A), {}, -1, "crd_gn_bwd_conv: bf16 output without residual / activation / channel sums"),
    (dict(out_mode=1, patch_k=2, patch_c=8), {}, -1, "crd_gn_bwd_conv: bad patch-scatter dims"),
    (dict(out_mode=2), {}, -1, "crd_gn_bwd_conv: bad patch-scatter dims"),
    (dict(stats=A, Cout=72, y_ld=72), {}, -1, "crd_gn_bwd_conv: stats need Cout % 16 == 0"),
    ({}, dict(dx=A + 8, dx_ld=64), -1, "crd_gn_bwd_conv: dx rows must be 16-byte aligned"),
    ({}, dict(dx=A, dx_ld=68), -1, "crd_gn_bwd_conv: dx rows must be 16-byte aligned"),
    ({}, dict(dgamma=A), -1, "crd_gn_bwd_conv: dgamma and dbeta come together"),
    ({}, dict(dbeta=A), -1, "crd_gn_bwd_conv: dgamma and dbeta come together"),
    (dict(Cin=4112, x_ld=4112), dict(gx_ld=4112), -2, "crd_gn_bwd_conv: tensor too large for 32-bit byte offsets"),
    (dict(IH=BIG, IW=BIG, OH=BIG, OW=BIG), {}, -2, "crd_gn_bwd_conv: tensor too large for 32-bit byte offsets"),
    (dict(red_x=A), {}, -1, "crd_gn_bwd_conv: incomplete fused-reduce arguments"),
    (dict(RED, red_x_ld=68), {}, -1, "crd_gn_bwd_conv: incomplete fused-reduce arguments"),
    (dict(RED, out_mode=1, patch_k=2, patch_c=16), {}, -2, "crd_gn_bwd_conv: the fused GroupNorm-backward reduce needs"),
    (dict(RED, y_coff=4), {}, -2, "crd_gn_bwd_conv: the fused GroupNorm-backward reduce needs"),         # vec_ok comes from the builder
    (dict(x=A + 8), {}, -1, "crd_gn_bwd_conv: dy / x rows must be 16-byte aligned"),
    ({}, dict(gx=A + 8), -1, "crd_gn_bwd_conv: dy / x rows must be 16-byte aligned"),
]


def _ref(obj):
    return None if obj is None else C.byref(obj)


def _refused(lib, rc, status, words, what):
    msg = lib.load().crd_last_error().decode()
    assert rc == status and msg.startswith(words), (what, rc, msg)


@pytest.mark.parametrize("i", range(len(IGEMM)))
def test_conv_igemm_refuses_before_any_launch(built, i):
    mut, status, words = IGEMM[i]
    d = None if mut is None else conv_desc(built, **mut)
    _refused(built, built.load().crd_conv_igemm(_ref(d), None), status, words, mut)


@pytest.mark.parametrize("i", range(len(GN_CONV)))
def test_gn_conv_refuses_before_any_launch(built, i):
    dm, nm, status, words = GN_CONV[i]
    d = None if dm is None else conv_desc(built, **dm)
    n = None if nm is None else gn_input(built, **nm)
    _refused(built, built.load().crd_gn_conv(_ref(d), _ref(n), None), status, words, (dm, nm))


@pytest.mark.parametrize("i", range(len(GN_CONV2)))
def test_gn_conv2_refuses_before_any_launch(built, i):
    d0m, n0m, d1m, n1m, status, words = GN_CONV2[i]
    d0 = None if d0m is None else conv_desc(built, **d0m)
    d1 = None if d1m is None else conv_desc(built, **d1m)
    n0, n1 = gn_input(built, **dict(dict(x_f32=1), **n0m)), gn_input(built, **dict(dict(x_f32=1), **n1m))
    _refused(built, built.load().crd_gn_conv2(_ref(d0), _ref(n0), _ref(d1), _ref(n1), None), status, words, GN_CONV2[i][:4])


@pytest.mark.parametrize("i", range(len(GN_BWD)))
def test_gn_bwd_conv_refuses_before_any_launch(built, i):
    dm, nm, status, words = GN_BWD[i]
    d = None if dm is None else conv_desc(built, **dm)
    n = None if nm is None else gn_bwd_input(built, **nm)
    _refused(built, built.load().crd_gn_bwd_conv(_ref(d), _ref(n), None), status, words, (dm, nm))
