"""Which kernel crd_conv_wgrad launches, pinned through the host-side query crd_conv_wgrad_route, and the case table that
tests/test_gpu_wgrad_routes.py runs against a float64 reference -- checked here, without a GPU.

The weight-gradient kernels multiply bf16 operands exactly, accumulate in fp32 and meet in 2^-44 fixed-point sums (crd_sum_t).  The
cases use operands on a coarse binary grid, so that EVERY partial sum any kernel can form is exact and the result must equal the
reference bit for bit -- a missing or doubled border pixel, halo column, tap or split tail always changes it:

  x  = m / 128,  m in +-[1, 127]   (all 8 bits of a bf16 significand, never zero)
  dy = n / 16,   n in +-[1, 15]

Every product is a multiple of 2^-11 below 1 in magnitude; a sum of at most 8192 of them is a multiple of 2^-11 below 2^13, i.e. an
integer below 2^24 in units of 2^-11: exact in fp32 in any order and any grouping.  It is far below the 2^18 limit of the fixed-point
conversion (csrc/common.h: to_fx) and on its 2^-44 grid.  The conditions are asserted below for every case, and an fp32
recomputation in a shuffled order must reproduce the float64 reference exactly -- so the GPU file needs no tolerance.

This file holds what both files share: the tables, the descriptors, the operands and the references."""
import ctypes as C
import functools
import re
import zlib

import pytest
import torch
import torch.nn.functional as F


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


_BUF = C.create_string_buffer(512)
A = (C.addressof(_BUF) + 255) // 256 * 256          # a non-NULL host address nobody reads: the query is host arithmetic


def cdiv(a, b):
    return -(-a // b)


def rup8(n):
    return cdiv(n, 8) * 8


# ------------------------------------------------------------------------------------------------------------------ dense cases
def G(wm, wn, tm, tn, splits, chunk):
    return "k_wgrad<%d,%d,%d,%d>/splits=%d,chunk=%d" % (wm, wn, tm, tn, splits, chunk)


def S3(tco, S, rows, chunks):
    return "k_wgrad3x3<2,4,%d,2>/S=%d,rows_per_wg=%d,chunks=%d" % (tco, S, rows, chunks)


T32, T64, T96, T128 = (1, 4, 2, 2), (1, 4, 4, 2), (2, 2, 3, 4), (2, 2, 4, 4)
# how a streaming case is planned: (dw_partial_capacity -- it caps the splits only together with dw_partials --, wg_budget)
VARIANTS = {"default": (0, 0), "cap1": (1, 0), "cap2": (2, 0), "budget3": (0, 3), "budget10": (0, 10)}


def _dense(name, B, Cin, H, W, Cout, k=3, s=1, p=1, label=None, labels=None, cref=None, sliced=False):
    """A convolution of a [B][Cin][H][W] input towards Cout channels.  label: the route of a generic-kernel case; labels: the routes
    of a streaming case under each of VARIANTS; cref: real input channels (the rest of Cin is zero padding of x); sliced: both
    operands are slices of wider buffers."""
    assert (label is None) != (labels is None) and (labels is None or list(labels) == list(VARIANTS))
    return dict(name=name, B=B, Cin=Cin, H=H, W=W, Cout=Cout, k=k, s=s, p=p, OH=(H + 2 * p - k) // s + 1, OW=(W + 2 * p - k) // s + 1,
                label=label, labels=labels, cref=cref or Cin, sliced=sliced)


def _stream(name, B, Cin, H, W, Cout, tco, default, cap1, cap2, budget3, budget10, **kw):
    chunks = cdiv(Cin, 64)
    plans = dict(zip(VARIANTS, (default, cap1, cap2, budget3, budget10)))
    return _dense(name, B, Cin, H, W, Cout, labels={v: S3(tco, S, rows, chunks) for v, (S, rows) in plans.items()}, **kw)


DENSE_CASES = [
    # ---- generic split-K kernel: every tile configuration at its Cout boundaries; splits = grid.z, chunk = pixels per split
    _dense("g32_cout1_3x3_narrow", 1, 32, 13, 9, 1, label=G(*T32, 1, 128), sliced=True),
    _dense("g32_cout21_3x3_narrow", 2, 128, 10, 11, 21, label=G(*T32, 1, 256), sliced=True),
    _dense("g32_cout32_3x3_short", 2, 32, 7, 40, 32, label=G(*T32, 3, 192)),                       # H = 7 < 8 with W >= 32
    _dense("g64_cout33_3x3s2", 2, 40, 17, 25, 33, s=2, label=G(*T64, 1, 256)),                     # P = 234, no multiple of 32
    _dense("g64_cout64_7x7s4_cin8", 2, 8, 29, 45, 64, k=7, s=4, p=3, label=G(*T64, 1, 192), cref=7),
    _dense("g96_cout65_8x8s8", 2, 64, 16, 24, 65, k=8, s=8, p=0, label=G(*T96, 1, 64)),            # P = 12
    _dense("g96_cout96_3x3_splits4", 2, 136, 19, 23, 96, label=G(*T96, 4, 256), cref=129),         # 874 pixels: last split 106 = 64 + 42
    _dense("g128_cout97_2x2s2", 2, 48, 12, 14, 97, k=2, s=2, p=0, label=G(*T128, 1, 128)),
    _dense("g128_cout128_3x3_w31", 2, 72, 11, 31, 128, label=G(*T128, 3, 256)),                    # W = 31 < 32
    _dense("g128_cout129_3x3_splits5", 2, 24, 21, 30, 129, label=G(*T128, 5, 256), sliced=True),   # two co tiles, 1260 pixels
    _dense("g128_cout160_1x1_b8_p8", 8, 160, 1, 1, 160, k=1, p=0, label=G(*T128, 1, 64)),          # P = 8 < 64
    _dense("g128_cout160_3x3_former_stream", 2, 64, 9, 40, 160, label=G(*T128, 3, 256)),           # streaming before the Cout <= 128 rule
    _dense("g128_cout256_1x1", 3, 256, 4, 7, 256, k=1, p=0, label=G(*T128, 1, 128)),
    _dense("g128_cout512_1x1_splits17", 2, 64, 40, 52, 512, k=1, p=0, label=G(*T128, 17, 256)),    # four co tiles, 4160 pixels
    # ---- streaming 3x3 kernel: (S, rows_per_wg) under each of VARIANTS
    _stream("s1_cout1_cin64_9x33", 1, 64, 9, 33, 1, 1, (2, 9), (1, 18), (2, 9), (2, 9), (2, 9), sliced=True),
    _stream("s1_cout21_cin8_13x64", 2, 8, 13, 64, 21, 1, (6, 9), (1, 52), (2, 26), (3, 18), (6, 9), sliced=True),
    _stream("s2_cout64_cin200_10x70", 2, 200, 10, 70, 64, 2, (7, 9), (1, 60), (2, 30), (1, 60), (2, 30)),
    _stream("s3_cout80_cin240_17x45", 1, 240, 17, 45, 80, 3, (4, 9), (1, 34), (2, 17), (1, 34), (2, 17), sliced=True),
    _stream("s3_cout96_cin136_11x40", 2, 136, 11, 40, 96, 3, (5, 9), (1, 44), (2, 22), (1, 44), (3, 15)),
    _stream("s4_cout128_cin48_8x32", 2, 48, 8, 32, 128, 4, (2, 8), (1, 16), (2, 8), (2, 8), (2, 8)),
]
DENSE = {c["name"]: c for c in DENSE_CASES}
assert len(DENSE) == len(DENSE_CASES)
GENERIC = [c["name"] for c in DENSE_CASES if c["label"]]
STREAM = [c["name"] for c in DENSE_CASES if c["labels"]]


def slice_geometry(c):
    """(x_ld, x_coff, dy_ld, dy_coff) of a case"""
    if c["sliced"]:
        return c["Cin"] + 24, 8, rup8(c["Cout"]) + 24, 16
    return c["Cin"], 0, rup8(c["Cout"]), 0


def wgrad_desc(lib, c, ptr=None, variant="default"):
    """The crd_wgrad_desc of a dense case.  ptr: name -> device address (x, dy, dw, dbias, parts); without it every pointer is a host
    address that nobody reads."""
    p = (lambda n: A) if ptr is None else (lambda n: ptr.get(n))
    d = lib.WgradDesc()
    x_ld, x_coff, dy_ld, dy_coff = slice_geometry(c)
    d.x, d.x_ld, d.x_coff, d.B, d.IH, d.IW, d.Cin = p("x"), x_ld, x_coff, c["B"], c["H"], c["W"], c["Cin"]
    d.dy, d.dy_ld, d.dy_coff, d.OH, d.OW, d.Cout = p("dy"), dy_ld, dy_coff, c["OH"], c["OW"], c["Cout"]
    d.KH, d.KW, d.stride, d.pad, d.dw, d.dbias = c["k"], c["k"], c["s"], c["p"], p("dw"), p("dbias")
    cap, budget = VARIANTS[variant]
    d.wg_budget = budget
    if cap:                                            # the cap of the splits holds only together with a partials buffer
        d.dw_partials, d.dw_partial_capacity = p("parts"), cap
    return d


def generic_parts(label):
    """-> (tile, splits, chunk) of a generic-kernel label, None otherwise"""
    m = re.fullmatch(r"k_wgrad<(\d),(\d),(\d),(\d)>/splits=(\d+),chunk=(\d+)", label)
    return None if m is None else (tuple(int(m.group(i)) for i in (1, 2, 3, 4)), int(m.group(5)), int(m.group(6)))


def stream_parts(label):
    """-> (tile incl. rows per step, S, rows_per_wg, chunks) of a streaming-kernel label, None otherwise"""
    m = re.fullmatch(r"k_wgrad3x3<(\d),(\d),(\d),(\d)>/S=(\d+),rows_per_wg=(\d+),chunks=(\d+)", label)
    return None if m is None else (tuple(int(m.group(i)) for i in (1, 2, 3, 4)), int(m.group(5)), int(m.group(6)), int(m.group(7)))


def segments(c, S, rows_per_wg):
    """What each of the S row splits of a streaming launch walks (csrc/wgrad3x3.hip: the `while (sr < sr_end)` loop): per workgroup the
    list of (image, strip column, first row, end row).  Strip rows are numbered image-major, then strip column, then row."""
    H, strips_x = c["H"], cdiv(c["W"], 32)
    total = c["B"] * strips_x * H
    out = []
    for s in range(S):
        sr, end = s * rows_per_wg, min((s + 1) * rows_per_wg, total)
        segs = []
        while sr < end:
            strip = sr // H
            seg_end = min((strip + 1) * H, end)
            segs.append((strip // strips_x, strip % strips_x, sr - strip * H, seg_end - strip * H))
            sr = seg_end
        out.append(segs)
    return out


# ------------------------------------------------------------------------------------------------ operands and float64 references
def _grid_values(shape, levels, g):
    """+-[1, levels] / (levels + 1), uniformly: never zero"""
    m = torch.randint(1, levels + 1, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return m * sign / (levels + 1)


def old_sums(shape, g):
    """Preloaded accumulator values: multiples of 2^-11 of magnitude at most 2^9 (with a gradient below 2^13: far below 2^18)"""
    return torch.randint(-(1 << 20), (1 << 20) + 1, shape, generator=g).double() * 2.0 ** -11


@functools.lru_cache(maxsize=None)           # (all of them together hold a few MB)
def dense_reference(name):
    """float64, read-only: x [B][Cin][H][W] (channels beyond cref are zero), dy [B][Cout][OH][OW], the weight gradient as
    dw [Cout][taps][Cin] (the library's layout: zeros in the padding channels), dbias [Cout], and the preloads old_dw / old_db."""
    c = DENSE[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = _grid_values((c["B"], c["Cin"], c["H"], c["W"]), 127, g)
    x[:, c["cref"]:] = 0
    dy = _grid_values((c["B"], c["Cout"], c["OH"], c["OW"]), 15, g)
    dw, db = conv_gradients(c, x, dy)
    return dict(x=x, dy=dy, dw=dw, dbias=db, old_dw=old_sums(dw.shape, g), old_db=old_sums(db.shape, g))


def conv_gradients(c, x, dy):
    """autograd of conv2d in the dtype of x: (dw [Cout][taps][Cin], dbias [Cout])"""
    w = torch.zeros(c["Cout"], c["Cin"], c["k"], c["k"], dtype=x.dtype, requires_grad=True)
    b = torch.zeros(c["Cout"], dtype=x.dtype, requires_grad=True)
    y = F.conv2d(x, w, b, stride=c["s"], padding=c["p"])
    assert y.shape[2:] == (c["OH"], c["OW"])
    y.backward(dy)
    return w.grad.permute(0, 2, 3, 1).reshape(c["Cout"], c["k"] * c["k"], c["Cin"]).contiguous(), b.grad


# ------------------------------------------------------------------------------------------------------------- depthwise cases
def _dw(name, B, C_, H, W, multi=False):
    return dict(name=name, B=B, C=C_, H=H, W=W, multi=multi)


DW_CASES = [
    _dw("dw_c64_9x13", 2, 64, 9, 13), _dw("dw_c512_8x12", 2, 512, 8, 12), _dw("dw_c160_5x7", 2, 160, 5, 7), _dw("dw_c64_11x45", 2, 64, 11, 45),
    _dw("dw_c80_9x33", 2, 80, 9, 33), _dw("dw_c256_17x64", 2, 256, 17, 64), _dw("dw_c16_9x13", 2, 16, 9, 13),
    # runs of two tiles per workgroup, the last run one tile: 32-wide tiles with a 2-row last tile; 16-wide tiles
    _dw("dw_c1024_b4_66x20_two_tiles", 4, 1024, 66, 20, multi=True), _dw("dw_c1024_b8_34x13_two_tiles", 8, 1024, 34, 13, multi=True),
]
DWC = {c["name"]: c for c in DW_CASES}
DW_REPLICAS = (1, 5)


def dw_plan(c):
    """(tile width, tiles_y, tiles per workgroup, runs) as crd_dwconv3x3_wgrad plans them (csrc/encoder_ops.hip: 8-row tiles, 64-channel
    windows, runs as long as ~512 workgroups remain)"""
    tw = 16 if c["W"] <= 16 else 32
    tiles_x, tiles_y, wins = cdiv(c["W"], tw), cdiv(c["H"], 8), cdiv(c["C"], 64)
    ysplit = max(1, min(cdiv(512, tiles_x * wins * c["B"]), tiles_y))
    per = cdiv(tiles_y, ysplit)
    return tw, tiles_y, per, cdiv(tiles_y, per)


@functools.lru_cache(maxsize=2)              # (the two large ones hold 90 MB each)
def dw_reference(name):
    """float64, read-only: x, dy [B][C][H][W], dw10 [10][C] = the nine shifted products summed over the pixels and sum dy, and one
    preload per replica old [max replicas][10][C]."""
    c = DWC[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    shape = (c["B"], c["C"], c["H"], c["W"])
    x, dy = _grid_values(shape, 127, g), _grid_values(shape, 15, g)
    return dict(x=x, dy=dy, dw10=dw_gradients(c, x, dy), old=old_sums((max(DW_REPLICAS), 10, c["C"]), g))


def dw_gradients(c, x, dy):
    H, W = c["H"], c["W"]
    xp = F.pad(x, (1, 1, 1, 1))
    rows = [(dy * xp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3)) for ky in range(3) for kx in range(3)]
    return torch.stack(rows + [dy.sum((0, 2, 3))])


# ===================================================================================================================== tests
# ---- the route table
@pytest.mark.parametrize("name", GENERIC)
def test_route_of_every_generic_case(built, name):
    c = DENSE[name]
    assert built.wgrad_route(wgrad_desc(built, c)) == c["label"]
    assert built.load().crd_conv_wgrad_splits(C.byref(wgrad_desc(built, c))) == 0


@pytest.mark.parametrize("name", STREAM)
def test_route_of_every_streaming_case(built, name):
    c = DENSE[name]
    for v in VARIANTS:
        d = wgrad_desc(built, c, variant=v)
        label = built.wgrad_route(d)
        assert label == c["labels"][v], v
        tile, S, rows, chunks = stream_parts(label)
        assert built.load().crd_conv_wgrad_splits(C.byref(d)) == S and chunks == cdiv(c["Cin"], 64)
        segs = segments(c, S, rows)                                     # the splits cover every strip row exactly once
        assert sum(y1 - y0 for wg in segs for (_, _, y0, y1) in wg) == c["B"] * cdiv(c["W"], 32) * c["H"] and all(segs)


def test_generic_cases_cover_what_they_promise():
    cs = [DENSE[n] for n in GENERIC]
    have = lambda pred: any(pred(c) for c in cs)                                                        # noqa: E731
    parts = {c["name"]: generic_parts(c["label"]) for c in cs}
    assert {p[0] for p in parts.values()} == {T32, T64, T96, T128}
    assert {c["Cout"] for c in cs} >= {1, 21, 32, 33, 64, 65, 96, 97, 128, 129, 160, 256}
    for c in cs:                                                        # the tile follows Cout: the boundaries sit on both sides
        t = parts[c["name"]][0]
        assert 16 * t[0] * t[2] == min(128, cdiv(c["Cout"], 32) * 32), c["name"]
    assert have(lambda c: c["Cout"] <= 128) and have(lambda c: c["Cout"] > 128)                          # one co tile / several
    assert have(lambda c: c["k"] * c["k"] * c["Cin"] % 128 != 0) and have(lambda c: c["Cin"] == 8)
    kinds = {(c["k"], c["s"], c["p"]) for c in cs}
    assert kinds >= {(1, 1, 0), (2, 2, 0), (3, 1, 1), (3, 2, 1), (7, 4, 3), (8, 8, 0)}
    assert have(lambda c: (c["k"], c["s"], c["W"]) == (3, 1, 31)) and have(lambda c: (c["k"], c["s"], c["H"]) == (3, 1, 7) and c["W"] >= 32)
    P = lambda c: c["B"] * c["OH"] * c["OW"]                                                             # noqa: E731
    assert have(lambda c: P(c) < 64 and c["B"] == 8 and c["OH"] * c["OW"] == 1) and have(lambda c: P(c) % 32 != 0)
    # several K splits whose last one is shorter than the rest and ends inside a 64-pixel step
    ragged = [c["name"] for c in cs if parts[c["name"]][1] > 1 and P(c) % parts[c["name"]][2] % 64 != 0]
    assert len(ragged) >= 3 and {parts[n][1] for n in ragged} >= {3, 4, 5}, ragged
    # ... and many splits with a last one of a single 64-pixel step (4160 = 16 x 256 + 64)
    assert parts["g128_cout512_1x1_splits17"][1:] == (17, 256) and P(DENSE["g128_cout512_1x1_splits17"]) % 256 == 64
    for c in cs:
        _, splits, chunk = parts[c["name"]]
        assert chunk % 64 == 0 and (splits - 1) * chunk < P(c) <= splits * chunk, c["name"]
    assert have(lambda c: (c["B"], c["Cin"], c["H"], c["W"], c["Cout"], c["k"]) == (2, 64, 9, 40, 160, 3))
    assert sum(c["sliced"] for c in cs) >= 2 and have(lambda c: c["sliced"] and c["Cout"] % 8) and have(lambda c: c["cref"] < c["Cin"])


def test_streaming_cases_cover_what_they_promise():
    cs = [DENSE[n] for n in STREAM]
    assert {stream_parts(c["labels"]["default"])[0] for c in cs} == {(2, 4, t, 2) for t in (1, 2, 3, 4)}
    assert {c["Cout"] for c in cs} >= {1, 21, 64, 80, 96, 128} and {c["Cin"] for c in cs} >= {8, 48, 64, 136, 200, 240}
    assert {c["W"] for c in cs} >= {32, 33, 40, 45, 64, 70} and {c["H"] for c in cs} >= {8, 9, 10, 11, 13, 17}
    assert sum(c["sliced"] for c in cs) >= 2 and any(c["sliced"] and c["Cout"] % 8 for c in cs)
    # the bias gradient of a first chunk none of whose waves 1..3 have input channels: Cin = 8
    assert any(c["Cin"] == 8 for c in cs)
    seen = set()
    for c in cs:
        for v, label in c["labels"].items():
            _, S, rows, _ = stream_parts(label)
            wgs = segments(c, S, rows)
            if S == 1:
                seen.add("S = 1")
            lens = [sum(y1 - y0 for (_, _, y0, y1) in wg) for wg in wgs]
            if S > 1 and lens[-1] < lens[0]:
                seen.add("short last workgroup")
            for wg in wgs:
                if len(wg) >= 3:
                    seen.add("three segments")
                if len({b for (b, _, _, _) in wg}) > 1:
                    seen.add("crosses an image boundary")
                for (_, _, y0, y1) in wg:
                    if y1 - y0 == 1:
                        seen.add("one-row segment")
                    if (y1 - y0) % 2:
                        seen.add("odd-length segment")
                    if y0 % 2:
                        seen.add("starts on an odd row")
    assert seen == {"S = 1", "short last workgroup", "three segments", "crosses an image boundary", "one-row segment", "odd-length segment",
                    "starts on an odd row"}


# ---- thresholds and the Python mirror
def _route(lib, **kw):
    c = dict(DENSE["g128_cout160_3x3_former_stream"], **kw)
    return lib.wgrad_route(wgrad_desc(lib, c)), lib.load().crd_conv_wgrad_splits(C.byref(wgrad_desc(lib, c)))


def test_streaming_kernel_stops_at_128_output_channels(built):
    """The widest streaming instance stages and accumulates 128 output channels: one channel more and the layer is the generic kernel's"""
    label, S = _route(built, Cout=128)
    assert stream_parts(label)[0] == (2, 4, 4, 2) and S == stream_parts(label)[1] > 0
    for cout in (129, 136, 160, 256, 304):
        label, S = _route(built, Cout=cout)
        assert generic_parts(label)[0] == T128 and S == 0, cout
    # ... and the partial copies are refused there as on any generic problem, by the launch and by the query alike
    L = built.load()
    d = wgrad_desc(built, DENSE["g128_cout160_3x3_former_stream"], variant="cap2")
    buf = C.create_string_buffer(96)
    assert L.crd_conv_wgrad_route(C.byref(d), buf, len(buf)) == -1
    msg = L.crd_last_error().decode()
    assert msg.startswith("crd_conv_wgrad: dw_partials is only supported where crd_conv_wgrad_splits() > 0")
    assert L.crd_conv_wgrad(C.byref(d), None) == -1 and L.crd_last_error().decode() == msg


def test_streaming_thresholds(built):
    at = lambda **kw: stream_parts(_route(built, Cout=64, **kw)[0]) is not None                            # noqa: E731
    assert at(W=32, OW=32, H=8, OH=8) and not at(W=31, OW=31, H=8, OH=8) and not at(W=32, OW=32, H=7, OH=7)
    assert not at(s=2, OH=5, OW=20) and not at(p=0, OH=7, OW=38) and not at(k=1, p=0)


GRID_COUT = [1, 8, 21, 32, 33, 40, 64, 65, 72, 96, 97, 104, 128, 129, 136, 160, 161, 256, 320, 512]


def test_plan_values_wgrad_tiles_agree_with_the_library(built):
    from camradepth_amd.plan_values import wgrad3_tile, wgrad_tile
    for cout in GRID_COUT:
        label, _ = _route(built, Cout=cout, W=31, OW=31)
        assert label.split("/")[0] == wgrad_tile(cout), (cout, label)
        label, S = _route(built, Cout=cout)
        if cout <= 128:                                                 # the mirror names the tile, not the rows per step
            assert S > 0 and re.sub(r",\d>$", ">", label.split("/")[0]) == wgrad3_tile(cout), (cout, label)
        else:
            assert S == 0 and label.split("/")[0] == wgrad_tile(cout), (cout, label)


def test_plan_asks_the_library_which_layers_stream(built):
    from camradepth_amd.plan_tables import stream3_splits
    L = built.load()
    assert stream3_splits(L, 8, 64, 104, 304, 128) > 0 and stream3_splits(L, 8, 64, 104, 304, 136) == 0
    assert stream3_splits(L, 8, 64, 104, 304, 128, wg_budget=160) == 160 // cdiv(304, 64)
    assert stream3_splits(L, 8, 7, 104, 64, 64) == 0 and stream3_splits(L, 8, 64, 31, 64, 64) == 0
    assert stream3_splits(L, 8, 64, 104, 64, 64, k=3, stride=2, pad=1) == 0 and stream3_splits(L, 8, 64, 104, 64, 64, k=1, stride=1, pad=0) == 0


# ---- refusals
def _mutated(lib, name="g96_cout96_3x3_splits4", **kw):
    d = wgrad_desc(lib, DENSE[name])
    for k, v in kw.items():
        setattr(d, k, v)
    return d


STREAM_NAME = "s2_cout64_cin200_10x70"
REFUSALS = [
    (None, {}, -1, "crd_conv_wgrad: null pointer"),
    ("g96_cout96_3x3_splits4", dict(x=None), -1, "crd_conv_wgrad: null pointer"),
    ("g96_cout96_3x3_splits4", dict(dw=None), -1, "crd_conv_wgrad: null pointer"),
    ("g96_cout96_3x3_splits4", dict(Cout=0), -1, "crd_conv_wgrad: bad dims"),
    ("g96_cout96_3x3_splits4", dict(stride=0), -1, "crd_conv_wgrad: bad dims"),
    ("g96_cout96_3x3_splits4", dict(Cin=132), -1, "crd_conv_wgrad: x channels must be multiples of 8"),
    ("g96_cout96_3x3_splits4", dict(x_coff=4), -1, "crd_conv_wgrad: x channels must be multiples of 8"),
    ("g96_cout96_3x3_splits4", dict(dy_ld=100), -1, "crd_conv_wgrad: dy_ld/dy_coff must be multiples of 8"),
    ("g32_cout21_3x3_narrow", dict(dy_ld=32, dy_coff=16), -1, "crd_conv_wgrad: dy rows must hold Cout rounded up to 8 channels"),
    ("g96_cout96_3x3_splits4", dict(dw_partials=A, dw_partial_capacity=4), -1, "crd_conv_wgrad: dw_partials is only supported where"),
    ("g96_cout96_3x3_splits4", dict(B=1 << 20), -2, "crd_conv_wgrad: tensor too large for 32-bit byte offsets"),
    (STREAM_NAME, dict(dw_partials=A, dw_partial_capacity=0), -1, "crd_conv_wgrad: dw_partials needs a capacity >= 1"),
    (STREAM_NAME, dict(wg_budget=-1), -1, "crd_conv_wgrad: wg_budget must be >= 0"),
    (STREAM_NAME, dict(IH=1 << 13, OH=1 << 13, IW=1 << 13, OW=1 << 13), -2, "crd_conv_wgrad: image too large for 32-bit byte offsets"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_route_query_refuses_what_the_entry_refuses(built, i):
    name, mut, status, words = REFUSALS[i]
    L = built.load()
    d = None if name is None else _mutated(built, name, **mut)
    ref = None if d is None else C.byref(d)
    buf = C.create_string_buffer(96)
    rc = L.crd_conv_wgrad_route(ref, buf, len(buf))
    msg = L.crd_last_error().decode()
    assert rc == status and msg.startswith(words), (mut, rc, msg)
    assert L.crd_conv_wgrad(ref, None) == rc and L.crd_last_error().decode() == msg             # refused before any launch


def test_route_query_needs_room_for_the_label(built):
    L = built.load()
    buf = C.create_string_buffer(96)
    for name, v in (("g96_cout96_3x3_splits4", "default"), (STREAM_NAME, "budget10")):
        d = wgrad_desc(built, DENSE[name], variant=v)
        label = (DENSE[name]["label"] or DENSE[name]["labels"][v]).encode()
        for cap in (0, 1, 12, len(label)):
            assert L.crd_conv_wgrad_route(C.byref(d), buf, cap) == -1
            assert L.crd_last_error().decode().startswith("crd_conv_wgrad_route: ")
        assert L.crd_conv_wgrad_route(C.byref(d), None, 96) == -1
        assert L.crd_conv_wgrad_route(C.byref(d), buf, len(label) + 1) == 0 and buf.value == label


# ---- the exactness conditions, before they cost a GPU run
def _shuffled_fp32(c, x, dy, g):
    """The weight and bias gradient as one fp32 GEMM over the pixels in a shuffled order"""
    cols = F.unfold(x.float(), c["k"], padding=c["p"], stride=c["s"])                    # [B][Cin * taps][L], channel-major rows
    P = c["B"] * c["OH"] * c["OW"]
    cols = cols.permute(1, 0, 2).reshape(-1, P)
    d2 = dy.float().permute(1, 0, 2, 3).reshape(c["Cout"], P)
    perm = torch.randperm(P, generator=g)
    dw = d2[:, perm] @ cols[:, perm].t()                                                  # [Cout][Cin * taps]
    dw = dw.view(c["Cout"], c["Cin"], c["k"] * c["k"]).permute(0, 2, 1).contiguous()
    db = d2[:, perm] @ torch.ones(P)
    return dw, db


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_case_is_exact_in_fp32(name):
    c = DENSE[name]
    r = dense_reference(name)
    P = c["B"] * c["OH"] * c["OW"]
    assert P <= 8192
    x, dy = r["x"], r["dy"]
    assert torch.equal(x, x.to(torch.bfloat16).double()) and torch.equal(dy, dy.to(torch.bfloat16).double())       # bf16 holds them
    assert (x[:, :c["cref"]] != 0).all() and (dy != 0).all() and (x[:, c["cref"]:] == 0).all()
    assert torch.equal(x * 128, (x * 128).round()) and torch.equal(dy * 16, (dy * 16).round())
    mag_w, mag_b = conv_gradients(c, x.abs(), dy.abs())                                    # sum |dy x| per output element, float64
    assert float(mag_w.max()) * 2 ** 11 < 2 ** 24 and float(mag_b.max()) * 2 ** 11 < 2 ** 24
    assert (r["dw"][:, :, c["cref"]:] == 0).all() and (r["dw"][:, :, :c["cref"]].abs().sum((0, 1)) > 0).all()
    dw32, db32 = _shuffled_fp32(c, x, dy, torch.Generator().manual_seed(1))
    assert torch.equal(dw32.double(), r["dw"]) and torch.equal(db32.double(), r["dbias"])
    for old, new in ((r["old_dw"], r["dw"]), (r["old_db"], r["dbias"])):
        assert torch.equal(old * 2 ** 11, (old * 2 ** 11).round()) and float((old.abs() + mag_w.max()).max()) < 2 ** 18
        assert float((old + new).abs().max()) < 2 ** 18


@pytest.mark.parametrize("name", list(DWC))
def test_depthwise_case_is_exact_in_fp32(name):
    c = DWC[name]
    r = dw_reference(name)
    P = c["B"] * c["H"] * c["W"]
    assert P <= 8192 and c["C"] % 16 == 0
    x, dy = r["x"], r["dy"]
    assert torch.equal(x, x.to(torch.bfloat16).double()) and torch.equal(dy, dy.to(torch.bfloat16).double())
    assert (x != 0).all() and (dy != 0).all()
    mag = dw_gradients(c, x.abs(), dy.abs())
    assert float(mag.max()) * 2 ** 11 < 2 ** 24
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(2))
    xp = F.pad(x.float(), (1, 1, 1, 1))
    d2 = dy.float().permute(1, 0, 2, 3).reshape(c["C"], P)[:, perm]
    rows = []
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky:ky + c["H"], kx:kx + c["W"]].permute(1, 0, 2, 3).reshape(c["C"], P)[:, perm]
            rows.append((d2 * xs).sum(1))
    rows.append(d2.sum(1))
    assert torch.equal(torch.stack(rows).double(), r["dw10"])
    old = r["old"]
    assert torch.equal(old * 2 ** 11, (old * 2 ** 11).round()) and float(old.abs().sum(0).max() + mag.max()) < 2 ** 18


def test_depthwise_cases_cover_what_they_promise():
    assert {(c["C"], c["H"], c["W"]) for c in DW_CASES if c["B"] == 2} >= {(64, 9, 13), (512, 8, 12), (160, 5, 7), (64, 11, 45), (80, 9, 33),
                                                                         (256, 17, 64)}
    assert any(c["C"] == 16 for c in DW_CASES)
    for c in DW_CASES:
        tw, tiles_y, per, runs = dw_plan(c)
        if c["multi"]:                                   # runs of several tiles, the last run shorter (the kernel's `break`)
            assert per >= 2 and runs * per > tiles_y > (runs - 1) * per, c["name"]
        else:
            assert per == 1, c["name"]
    a, b = DWC["dw_c1024_b4_66x20_two_tiles"], DWC["dw_c1024_b8_34x13_two_tiles"]
    assert dw_plan(a) == (32, 9, 2, 5) and a["H"] % 8 == 2 and a["B"] * a["H"] * a["W"] == 5280
    assert dw_plan(b) == (16, 5, 2, 3)
