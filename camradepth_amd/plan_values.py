"""Plan values and labels: what a recorded plan is made of, and the names of the kernels the library will pick.

Owns the value types of a plan -- PM (a pixel-major tensor view), Op (one recorded launch), ConvW (a convolution's parameters and
packed forms), the lazy pointer arguments (_Lazy, _WPtr, _BufPtr) that Plan._finalise resolves -- the algorithmic byte / FLOP
counts (nbytes, dgrad_flops) and EVERY kernel-label rule: the *_tile functions restate the dispatch of the C library so that
bench.py and the tools can name the kernel behind a launch.  Labels never change what is launched."""
import os

import torch

BF16, F32 = torch.bfloat16, torch.float32
SUM = torch.int64    # crd_sum_t: the 64-bit fixed-point accumulators every multi-workgroup "+=" goes through (include/camradepth_hip.h)


# Encoder stages (bit s = stage s + 1) whose Blocks run the head of the attention backward as crd_attn_bwd_fused + crd_attn_dk_fold
# instead of crd_attn_out_bwd(_gn) + crd_attn_bwd + crd_sum_partials_bf16 (engine.Plan._attn_bwd; DESIGN.md section 4 has the A/B).
# CRD_ATTN_BWD_FUSED overrides it under CRD_DEV_SWITCHES=1, read when a plan is built.
ATTN_BWD_FUSED = 15


def rup(x, m=8):
    return (x + m - 1) // m * m


class PM:
    """Pixel-major view: element (b, p, c) at t[b, p, coff + c]; t has shape [B, H*W, ld]."""
    __slots__ = ("t", "ld", "coff", "C", "H", "W", "f32")

    def __init__(self, t, C_, H, W, coff=0):
        self.t, self.ld, self.coff, self.C, self.H, self.W = t, t.shape[-1], coff, C_, H, W
        self.f32 = 1 if t.dtype == F32 else 0

    def sl(self, c0, c1):
        return PM(self.t, c1 - c0, self.H, self.W, self.coff + c0)

    @property
    def P(self):
        return self.H * self.W

    @property
    def ptr(self):
        return self.t.data_ptr()


class Op:
    """One recorded kernel call.  stream: 0 = the main stream, LATE = a weight gradient nothing in the pass waits for."""
    __slots__ = ("fn", "args", "name", "region", "acc_slot", "meta", "stream", "io", "cond")

    def __init__(self, fn, args, name, region=None, acc_slot=None, meta=None, stream=0, io=None, cond=None):
        self.fn, self.args, self.name, self.region, self.acc_slot, self.meta = fn, args, name, region, acc_slot, meta
        self.stream = stream
        self.cond = cond        # None, or (plan attribute, value): the op runs only while getattr(plan, attribute) == value (Plan.live)
        self.io = io            # algorithmic HBM bytes of the launch (int, or a callable evaluated after Plan._finalise): see nbytes()


def nbytes(*ts):
    """ALGORITHMIC bytes of the tensors a launch must read or write once (bench.py's floor budget, tools/floor_table.py): a PM
    counts its own C channels of every pixel, not the row stride of the buffer it is a slice of; halo re-reads, padding channels
    and cache effects are deliberately not in here -- that is what the measured traffic is compared against."""
    n = 0
    for t in ts:
        if t is None:
            continue
        if isinstance(t, PM):
            n += t.t.shape[0] * t.P * t.C * (4 if t.f32 else 2)
        elif isinstance(t, _Lazy):
            n += t.numel * 8
        elif isinstance(t, torch.Tensor):
            n += t.numel() * t.element_size()
        else:
            n += int(t)
    return n


def igemm_tile(cout, ohw=1 << 30, batch=1):
    """Tile configuration crd_conv_igemm dispatches to (csrc/igemm.hip), as the kernel's template arguments."""
    if cout > 32 and -(-ohw // 128) * -(-cout // 128) * batch < 192:
        return "k_igemm<2,2,1,1>"
    if cout <= 32:
        return "k_igemm<4,1,1,1>"
    if cout <= 64:
        return "k_igemm<2,2,2,1>"
    if cout <= 96:
        return "k_igemm<4,1,1,3>"
    if 128 < cout <= 160:
        return "k_igemm<4,1,1,5>"
    return "k_igemm<2,2,2,2>"


def fused_reduce_tile_ok(cout, ohw, B):
    """crd_conv_igemm's rule for red_x (csrc/igemm.hip): the fused GroupNorm-backward reduce lives in the vector epilogue of the
    32 / 64 / 128-column tiles (small grids always use 64-column tiles), not the 96- and 160-column ones."""
    small = cout > 32 and -(-ohw // 128) * -(-cout // 128) * B < 192
    return cout % 16 == 0 and (small or cout <= 64 or 96 < cout <= 128 or cout > 160)


def persistent_conv3(spec, B):
    """Does crd_conv_igemm send this 3x3 launch to the persistent one-wave-per-SIMD kernel (csrc/conv3x3p.hip)?  Plain bf16
    store / accumulate (+ GroupNorm sums) on grids of >= 192 tiles of 16 x 32 pixels."""
    if os.environ.get("CRD_CONV3P", "1") == "0":
        return False
    y = spec["y"]
    plain = (not y.f32 and spec["bias"] is None and not spec["act"] and spec["res"] is None and spec["out_mode"] == 0
             and spec.get("red") is None and spec.get("chan") is None)
    halo = spec["k"] == 3 and spec["stride"] == 1 and spec["OW"] >= 32 and spec["OH"] >= 8
    tiles = -(-spec["OW"] // 32) * -(-spec["OH"] // 16) * B
    return bool(plain and halo and tiles >= 192 and spec["cout"] >= 64 and spec["cout"] % 8 == 0)


def halo_tile(cout, OH=1 << 20, OW=1 << 20, B=1):
    """Tile configuration of the halo-tile 3x3 kernel (csrc/conv3x3.hip: crd_conv3x3_halo), for the bench labels."""
    tiles = -(-OW // 32) * -(-OH // 8) * B
    if cout > 32 and tiles * -(-cout // 128) < 512:      # under-filled grid: 64- or 32-column tiles
        return "k_conv3x3<4,1,2,2>" if tiles * -(-cout // 64) >= 512 else "k_conv3x3<4,1,2,1>"
    if cout <= 32:
        return "k_conv3x3<4,1,2,1>"
    if cout <= 64:
        return "k_conv3x3<4,1,2,2>"
    if cout <= 96:
        return "k_conv3x3<4,1,2,3>"
    if 128 < cout <= 160 or 256 < cout <= 320:      # two launches: 128-wide tiles + the remaining columns
        return "k_conv3x3<4,1,2,4>+<4,1,2,1>" if cout - (256 if cout > 256 else 128) <= 32 else "k_conv3x3<4,1,2,4>+<4,1,2,2>"
    return "k_conv3x3<4,1,2,4>"


def wgrad_tile(cout):
    if cout <= 32:
        return "k_wgrad<1,4,2,2>"
    if cout <= 64:
        return "k_wgrad<1,4,4,2>"
    if cout <= 96:
        return "k_wgrad<2,2,3,4>"
    return "k_wgrad<2,2,4,4>"


class ConvW:
    """A dense convolution's parameters and packed forms."""

    def __init__(self, name, cout, cin_ref, k, cmap, bias, need_dgrad, scatter=False, dgrad_rows=None):
        self.name, self.cout, self.cin_ref, self.k, self.taps = name, cout, cin_ref, k, k * k
        self.cmap = cmap                      # list[int] internal channel -> reference channel (or -1), len = cin_pad
        self.cin_pad = len(cmap) if cmap is not None else rup(cin_ref)
        self.cout_pad = rup(cout)
        self.bias, self.need_dgrad, self.scatter = bias, need_dgrad, scatter
        self.identity = (cmap is None and self.cin_pad == cin_ref and self.taps == 1)
        self.w_fwd = self.w_dgrad = self.w_scatter = None   # bf16 tensors
        self.dw = None                                        # fp32 [cout][taps][cin_pad] (scratch or direct grad view)
        self.wg_budget = 0
        self.dw_parts, self.dw_S, self.stream3_geom = None, 0, None   # per-split copies of dw for the streaming 3x3 wgrad
        self.cmap_dev = None

    @property
    def dims(self):
        """(Cout, Cin_ref, taps, Cin_pad, Cout_pad) as the pack / unpack tables carry them."""
        return self.cout, self.cin_ref, self.taps, self.cin_pad, self.cout_pad


def wgrad3_tile(cout):
    """Tile configuration of the streaming 3x3 weight gradient (csrc/wgrad3x3.hip)."""
    return "k_wgrad3x3<2,4,%d>" % (1 if cout <= 32 else 2 if cout <= 64 else 3 if cout <= 96 else 4)


def conv3p_tile(cout):
    """Persistent 3x3 kernel (csrc/conv3x3p.hip); a ragged tail of <= 64 columns goes to a halo-tile launch."""
    if cout <= 96:
        return "k_conv3x3p<2>" if cout <= 64 else "k_conv3x3p<3>"
    rest = cout % 128
    return "k_conv3x3p<4>" + ("" if rest == 0 or rest > 64 else "+k_conv3x3<4,1,2,1>" if rest <= 32 else "+k_conv3x3<4,1,2,2>")


def fp8_tile(cout):
    return "k_conv3x3_fp8<%d>" % (2 if cout <= 64 else 3 if cout <= 96 else 4)


def gn_small_tile(cout, ohw, B):
    """crd_gn_conv / crd_gn_conv2 / crd_gn_bwd_conv: the problem runs on the 64 x 64 tiles."""
    return cout <= 64 or -(-ohw // 64) * -(-cout // 128) * B < 256


def gngemm_tile(cout, ohw, B):
    return "k_gngemm_reg" + ("<2,2,1,1>" if gn_small_tile(cout, ohw, B) else "<2,2,1,2>")


def gnbwd_tile(cout, ohw, B, out_mode):
    return "k_gnbwd_gemm" + ("<1>" if gn_small_tile(cout, ohw, B) or out_mode == 1 else "<2>")


def dgrad_flops(B, x, w, cout):
    """Algorithmic work of a data gradient = that of the forward of convolution w[1] (w = ("dgrad" | "scatter", ConvW)); x = dy."""
    cw = w[1]
    return 2.0 * B * x.H * x.W * cw.cout * cw.taps * min(cout // (cw.taps if w[0] == "scatter" else 1), cw.cin_ref)


class _WPtr:
    """Packed bf16 weights of a conv (allocated in Plan._finalise) as a raw-pointer op argument."""
    __slots__ = ("cw", "kind")

    def __init__(self, cw, kind):
        self.cw, self.kind = cw, kind

    def data_ptr(self):
        return getattr(self.cw, self.kind).data_ptr()


class _BufPtr:
    """A plan-owned scratch buffer that may still be re-allocated (grown) while the plan is built, as a raw-pointer op argument."""
    __slots__ = ("plan", "attr")

    def __init__(self, plan, attr):
        self.plan, self.attr = plan, attr

    def data_ptr(self):
        return getattr(self.plan, self.attr).data_ptr()


class _Lazy:
    """Placeholder for a slice of a zero-arena, materialised in Plan._finalise."""
    __slots__ = ("shape", "numel", "t")

    def __init__(self, shape):
        self.shape = tuple(shape)
        n = 1
        for s in shape:
            n *= s
        self.numel, self.t = n, None

    def data_ptr(self):
        return self.t.data_ptr()
