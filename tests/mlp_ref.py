"""float64 reference of the fused Mlp of an encoder Block (crd_mlp_fwd + crd_mlp_reduce, camradepth_amd/csrc/mlp_fused.hip), one function
per stage, written from the operation the header of that file defines:

    x2 = x1 + dp * bf16( fc2( GELU( norm2( dwconv3x3( norm1( fc1( Block.norm2(x1) ) ) ) ) ) ) + b2 )

Tensors are channel-last ([B][N][C], N = H * W), as the device stores them.  A stage function takes what the DEVICE stored for the
previous stage (exact bf16 / fp32 values, as float64) and the fixed-point sums the device reports (int64, value * 2^20), so an error
of one stage is never carried into the bound of the next.  It returns

    v   the un-rounded float64 value of the stage's output,
    A   the same expression with every term replaced by its magnitude (it scales the fp32 evaluation slack),
    and for h2 a third tensor (below).

BOUNDS.  bf16 keeps 8 significant bits: round-to-nearest moves a value by at most 2^-8 |v|.  The kernel rounds an fp32 value, not v:

    bf16 output:   |got - v| <= 2^-8 |v| + c 2^-23 A + TINY            (bound_bf16)
    fp32 output:   |got - v| <=           c 2^-23 A + TINY            (bound_f32)

c counts the fp32 operations on the longest path of the stage.  Every IEEE operation errs by at most 2^-24 of its result (half an
ulp), so counting a whole 2^-23 per operation leaves a factor two for second-order terms; TINY = 2^-126.

    stage  c    derivation
    xn     7    mean -> fp32, rstd -> fp32, gamma * rstd, mean * ga, beta - ., x * ga, + shift                           (C_AFFINE)
    h1     C+1  an MFMA sum over K = C products of two bf16 values (each exact in fp32) onto the bias
    h2     10   nine tap products added onto the bias one after the other, as the issue counts them               (C_STENCIL)
                + sum_taps |w| * amb: norm1(h1) is rounded to bf16 INSIDE the stage and is not stored.  Its fp32 value lies within
                e = C_AFFINE 2^-23 A_norm1 of the float64 one; where bf16(n - e) != bf16(n + e) the device may hold either
                neighbour, and amb is their distance (zero for all but a few elements in 10^4).
    h3     14   8 = ceil(1.13 * C_AFFINE): the affine's slack through GELU, whose slope is at most 1.13;
                4 = the erf allowance below, halved by Phi = (1 + erf) / 2; 2 = that sum and the product x * Phi           (C_H3)
    part   64   an MFMA sum over the K = 64 channels of the slab, onto zero
    x2     slabs + 1 for o = sum_s part[s] + b2 (rounded to bf16: the first term too, both times |dp|), and 2 for the fp32
           product and sum of x1 + dp * o_r, on |x1| + |dp o|

ALLOWANCES MEASURED ON THE CPU AGAINST float64 (tests/test_mlp_ref_cpu.py measures them again and asserts them), in units of 2^-23:
    * torch.erf in fp32 against fp64 on [-12, 12] / sqrt 2: 0.52.
    * the kernel does not call erff: gelu_exact (common.h) is Abramowitz-Stegun 7.1.26.  That formula in fp64 against erf: 1.17 (its
      published bound 1.5e-7 is 1.26); evaluated in fp32 with separate multiplies and adds, a correctly rounded division and exp: 4.55,
      the most where the rounding of -z^2 is multiplied by z^2 in the exponential.  The device takes 1 / . from v_rcp_f32 (1 ulp, not
      1/2: + 1 on t, whose polynomial has |t poly'(t)| <= 1) and the exponential from v_exp_f32 (1 ulp after an fp32 product with
      log2 e: + 2 on E <= 1).  ERF_UNITS = 8 covers 4.55 + 1 + 2.
    * rsqrt: gn_moments evaluates the mean and 1 / sqrt(var + eps) in fp64 and rounds each ONCE to fp32: 0.50 of 2^-23 relative (a
      half ulp).  These are the first two operations of C_AFFINE; no further allowance.

SUMS keep the project's bound: assert_close(rel=1e-5, elem=1e-5) against the float64 sums of the stored tensor (sums_close here).

MUTANTS (tests/test_mlp_ref_cpu.py shows each rejected): the stage functions take `mutant`, one of MUTANTS, and then compute what a
subtly wrong kernel would.  The tanh form of GELU ("gelu_tanh", not one the issue lists) is rejected as well: it differs from the erf
form by a few 1e-4, an even function of x, which is far inside 2^-8 |v| for positive x but many times the bound in the negative
tail, where |v| is small.  Not covered: a kernel that took the tanh form only for x > 0, or only for |x| < 0.3, where the two forms
agree to within the bf16 rounding.
"""
import math

import torch

U = 2.0 ** -23
HALF_BF16 = 2.0 ** -8
TINY = 2.0 ** -126
STAT_ONE = 2.0 ** 20
EPS = 1e-5
SLAB = 64
C_AFFINE, C_STENCIL, ERF_UNITS = 7, 10, 8
C_H3 = math.ceil(1.13 * C_AFFINE) + ERF_UNITS // 2 + 2
C_PART = SLAB
MUTANTS = ("mirror_x", "pad_before_norm1", "norm2_over_16", "count_np", "sums_with_pad_rows", "dp_on_residual", "prev_sample_sums",
           "gelu_tanh")


def bf16(v):
    """Nearest bf16 of float64 values, as float64."""
    return v.to(torch.bfloat16).double()


def bound_bf16(v, A, c, extra=0.0):
    return HALF_BF16 * v.abs() + c * U * A + extra + TINY


def bound_f32(A, c):
    return c * U * A + TINY


def slab_sums(x):
    """[B][N][C] -> float64 [B][C/16][2]: sum and sum of squares over pixels and 16 channels."""
    B, N, C = x.shape
    v = x.double().reshape(B, N, C // 16, 16)
    return torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1)


def to_stat(x):
    return (x.double() * STAT_ONE).round().to(torch.int64)


def sums_close(got_int, ref, rel=1e-5, elem=1e-5):
    """The project's bound for GroupNorm sums (assert_close of tests/test_gpu_igemm.py) -> (passes, max err / bound, rel-L2 / bound)."""
    got, ref = got_int.double() / STAT_ONE, ref.double()
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    rl2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    return err <= elem * scale and rl2 < rel, err / (elem * scale), rl2 / rel


def moments(st, count, gmul=1, mutant=None):
    """gn_moments (common.h) in float64 from int64 sums [B][G16][2]: -> mean, rstd [B][1][G16 * 16] (a group is gmul slabs)."""
    B, G16, _ = st.shape
    q = st.reshape(B, G16 // gmul, gmul, 2).sum(2)                    # integer addition, exact
    if mutant == "prev_sample_sums":
        q = q.roll(1, 0)
    inv = 1.0 / (float(count) * STAT_ONE)
    m = q[..., 0].double() * inv
    var = (q[..., 1].double() * inv - m * m).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    rep = 16 * gmul
    return m.repeat_interleave(rep, 1).unsqueeze(1), rstd.repeat_interleave(rep, 1).unsqueeze(1)


def affine(x, m, r, gamma, beta):
    g, b = gamma.double(), beta.double()
    return (x - m) * r * g + b, (x.abs() + m.abs()) * r * g.abs() + b.abs()


def np_of(N):
    return (N + 31) // 32 * 32


def stage_xn(x1, x1_stats, gamma, beta, mutant=None):
    N = x1.shape[1]
    count = (np_of(N) if mutant == "count_np" else N) * 16
    m, r = moments(x1_stats, count, 1, mutant)
    return affine(x1.double(), m, r, gamma, beta)


def stage_h1(xn_dev, w1, b1):
    x, w, b = xn_dev.double(), w1.double(), b1.double()
    return x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()


def h1_sums(h1_dev, b1=None, mutant=None):
    s = slab_sums(h1_dev)
    if mutant == "sums_with_pad_rows":        # the NP - N padding rows of the MFMA tile hold bf16(fc1 bias)
        N = h1_dev.shape[1]
        pad = bf16(b1.double()).reshape(1, 1, -1).expand(h1_dev.shape[0], np_of(N) - N, -1)
        s = s + slab_sums(pad)
    return s


def stage_h2(h1_dev, h1_stats, gamma, beta, w9, bd, H, W, mutant=None):
    """-> v, A, extra (the bf16 ambiguity of the unstored norm1(h1), see the module docstring).  w9 is [9][hid], tap ky * 3 + kx
    multiplies pixel (y + ky - 1, x + kx - 1)."""
    B, N, hid = h1_dev.shape
    count = (np_of(N) if mutant == "count_np" else N) * 16
    m, r = moments(h1_stats, count, 1, mutant)
    n, An = affine(h1_dev.double(), m, r, gamma, beta)
    e = C_AFFINE * U * An
    nr = bf16(n)
    amb = (bf16(n + e) - bf16(n - e)).abs()

    def padded(t, fill=None):
        t = t.reshape(B, H, W, hid)
        p = torch.zeros(B, H + 2, W + 2, hid, dtype=torch.float64)
        if fill is not None:
            p[:] = fill
        p[:, 1:H + 1, 1:W + 1] = t
        return p

    fill = None
    if mutant == "pad_before_norm1":          # a zero h1 outside the image, normalised like every other pixel
        fill = bf16(affine(torch.zeros(B, 1, hid, dtype=torch.float64), m, r, gamma, beta)[0]).reshape(B, 1, 1, hid)
    pn, pa = padded(nr, fill), padded(amb)
    v = bd.double().reshape(1, 1, 1, hid).expand(B, H, W, hid).clone()
    A = v.abs()
    extra = torch.zeros_like(v)
    for ky in range(3):
        for kx in range(3):
            w = w9[ky * 3 + ((2 - kx) if mutant == "mirror_x" else kx)].double()
            win = pn[:, ky:ky + H, kx:kx + W]
            v = v + win * w
            A = A + win.abs() * w.abs()
            extra = extra + pa[:, ky:ky + H, kx:kx + W] * w.abs()
    return v.reshape(B, N, hid), A.reshape(B, N, hid), extra.reshape(B, N, hid)


def stage_h3(h2_dev, h2_stats, gamma, beta, mutant=None):
    N = h2_dev.shape[1]
    gmul = 1 if mutant == "norm2_over_16" else 4
    count = (np_of(N) if mutant == "count_np" else N) * 16 * gmul
    m, r = moments(h2_stats, count, gmul, mutant)
    x, Ax = affine(h2_dev.double(), m, r, gamma, beta)
    if mutant == "gelu_tanh":
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))), Ax
    return x * 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))), Ax


def stage_part(h3_dev, w2):
    """-> v, A [hid / 64][B][N][C]: the slabs' contributions to fc2."""
    B, N, hid = h3_dev.shape
    h = h3_dev.double().reshape(B, N, hid // SLAB, SLAB).permute(2, 0, 1, 3)            # [S][B][N][64]
    w = w2.double().reshape(-1, hid // SLAB, SLAB).permute(1, 2, 0)                       # [S][64][C]
    return torch.einsum("sbnk,skc->sbnc", h, w), torch.einsum("sbnk,skc->sbnc", h.abs(), w.abs())


def stage_x2(part_dev, x1, b2, dp, mutant=None):
    """-> v, bound: x2 has a rounded portion (o) and an fp32 one, so the bound is assembled here."""
    slabs, B = part_dev.shape[0], part_dev.shape[1]
    d = (torch.ones(B, dtype=torch.float64) if dp is None else dp.double()).reshape(B, 1, 1)
    o = part_dev.double().sum(0) + b2.double()
    Ao = part_dev.double().abs().sum(0) + b2.double().abs()
    x = x1.double()
    v = d * (x + o) if mutant == "dp_on_residual" else x + d * o
    bound = d.abs() * (HALF_BF16 * o.abs() + (slabs + 1) * U * Ao) + 2 * U * (x.abs() + d.abs() * o.abs() * (1 + 2 * HALF_BF16)) + TINY
    return v, bound


def make_inputs(B, H, W, C, seed=0):
    """The inputs of tests/test_gpu_mlp_paths.py and tests/test_mlp_ref_cpu.py (hid = 4 C): x1 with an offset and a scale per sample and
    16-channel group, non-zero biases, an affine that differs per channel, asymmetric taps, fc weights exact in bf16."""
    hid, N = 4 * C, H * W
    g = torch.Generator().manual_seed(seed * 7919 + 1000 * B + 10 * C + N)

    def rn(*s):
        return torch.randn(*s, generator=g)

    off = (torch.rand(B, 1, C // 16, 1, generator=g) * 4 - 2)
    scl = (torch.rand(B, 1, C // 16, 1, generator=g) * 1.5 + 0.5)
    x1 = (rn(B, N, C // 16, 16) * scl + off + 0.3 * rn(1, 1, C // 16, 16)).reshape(B, N, C).contiguous()
    inp = dict(
        B=B, H=H, W=W, C=C, hid=hid, N=N, x1=x1, x1_stats=to_stat(slab_sums(x1)),
        w1=bf16((rn(hid, C) / C ** 0.5).double()).float(), b1=0.3 * rn(hid) + 0.2,
        w2=bf16((rn(C, hid) / hid ** 0.5).double()).float(), b2=0.2 * rn(C) + 0.1,
        w9=(rn(9, hid) / 3).contiguous(), bd=0.2 * rn(hid) + 0.1,
        g0=1 + 0.2 * rn(C), b0=0.2 * rn(C), g1=1 + 0.2 * rn(hid), b1n=0.3 * rn(hid), g2=1 + 0.2 * rn(hid), b2n=0.2 * rn(hid),
        dp=torch.tensor([1.0 / 0.9, 0.0, 1.0]).repeat(-(-B // 3))[:B])
    return inp


def fake_device(inp, mutant=None):
    """What a kernel that rounds exactly where the definition does would store: every stage's reference value rounded to its storage
    type, fed to the next stage.  With `mutant` the kernel is wrong in that one way."""
    H, W = inp["H"], inp["W"]
    d = {}
    d["xn"] = bf16(stage_xn(inp["x1"], inp["x1_stats"], inp["g0"], inp["b0"], mutant)[0])
    d["h1"] = bf16(stage_h1(d["xn"], inp["w1"], inp["b1"])[0])
    d["h1_stats"] = to_stat(h1_sums(d["h1"], inp["b1"], mutant))
    # (wrong sums are reported AND used by the kernel's own norm1: only the sums check can see them)
    d["h2"] = bf16(stage_h2(d["h1"], d["h1_stats"], inp["g1"], inp["b1n"], inp["w9"], inp["bd"], H, W, mutant)[0])
    d["h2_stats"] = to_stat(slab_sums(d["h2"]))
    d["h3"] = bf16(stage_h3(d["h2"], d["h2_stats"], inp["g2"], inp["b2n"], mutant)[0])
    d["part"] = stage_part(d["h3"], inp["w2"])[0].float().double()
    dpv = inp["dp"].double().reshape(-1, 1, 1)
    o = bf16(d["part"].sum(0) + inp["b2"].double())
    x = inp["x1"].double()
    d["x2"] = (dpv * (x + o) if mutant == "dp_on_residual" else x + dpv * o).float().double()
    return d


STAGES = ("xn", "h1", "h2", "h3", "part", "x2")


def stage_report(inp, dev, dp="inp"):
    """Every stage fed with the device's tensors of the one before -> dict stage -> (max |got - v| / bound, slack used).  The first
    figure of a bf16 output approaches 1 for a correct kernel (the rounding itself reaches 2^-8 |v|), so the second says how much
    room is left.  Where got is not the nearest bf16 of v, the device's unrounded value lay beyond the midpoint of the two
    neighbours, at least (|got - v| - |bf16(v) - v|) / 2 from v; the figure is the largest such distance as a fraction of the
    fp32 slack c 2^-23 A (0: every value is the nearest bf16 of v).  For h2 it is taken over the elements whose nine norm1(h1)
    inputs were all unambiguous (extra == 0); elsewhere the device may hold the other neighbour and `extra` is used in full.  For
    the fp32 outputs (and x2, most of whose bound is the rounding of o) the two figures are the same."""
    H, W = inp["H"], inp["W"]
    out = {}

    def bf(name, v, A, c, extra=0.0):
        err = (dev[name].double() - v).abs()
        best = (bf16(v) - v).abs()
        used = 0.5 * (err - best) / (c * U * A + TINY)
        if torch.is_tensor(extra):            # h2: where norm1(h1) was ambiguous the other neighbour is legitimate, not slack used
            used = used[extra == 0]
        out[name] = ((err / bound_bf16(v, A, c, extra)).max().item(), used.max().item() if used.numel() else 0.0)

    bf("xn", *stage_xn(inp["x1"], inp["x1_stats"], inp["g0"], inp["b0"]), C_AFFINE)
    bf("h1", *stage_h1(dev["xn"], inp["w1"], inp["b1"]), inp["C"] + 1)
    v, A, extra = stage_h2(dev["h1"], dev["h1_stats"], inp["g1"], inp["b1n"], inp["w9"], inp["bd"], H, W)
    bf("h2", v, A, C_STENCIL, extra)
    bf("h3", *stage_h3(dev["h2"], dev["h2_stats"], inp["g2"], inp["b2n"]), C_H3)
    v, A = stage_part(dev["h3"], inp["w2"])
    r = ((dev["part"].double() - v).abs() / bound_f32(A, C_PART)).max().item()
    out["part"] = (r, r)
    v, bound = stage_x2(dev["part"], inp["x1"], inp["b2"], inp["dp"] if isinstance(dp, str) else dp)
    r = ((dev["x2"].double() - v).abs() / bound).max().item()
    out["x2"] = (r, r)
    return out


def stage_ratios(inp, dev, dp="inp"):
    """max |got - v| / bound per stage -> dict stage -> float."""
    return {k: v[0] for k, v in stage_report(inp, dev, dp).items()}


def sums_ratios(dev):
    """The two reported sums against the float64 sums of the stored tensors -> dict name -> (passes, err ratio, rel-L2 ratio)."""
    return {"h1 sums": sums_close(dev["h1_stats"], slab_sums(dev["h1"])), "h2 sums": sums_close(dev["h2_stats"], slab_sums(dev["h2"]))}


# ---- the facts of a launch, from the formulas of mlp_fused.hip (the tests assert them for every case) ----
def lds_bytes(N, C):
    return C * 8 + (192 + 640) * 4 + SLAB * (C + 8) * 2 + C * SLAB * 2 + 2 * np_of(N) * SLAB * 2


def fused_supported(H, W, C, hid):
    N, nch = H * W, C // 32
    if C % 32 or nch not in (1, 2, 4, 5, 8) or hid % SLAB or hid // (C // 16) != SLAB:
        return 0
    if N > 416 or (N > 128 and nch == 8) or lds_bytes(N, C) > 160 * 1024:
        return 0
    return hid // SLAB


def reduce_partition(B, N, C):
    """crd_mlp_reduce's launch: -> dict(PL pixel lanes, idle threads, uncapped workgroups, cap, nblk, chunk)."""
    CG = C // 8
    PL = max(1, 256 // CG)
    want = -(-N // (2 * PL))
    cap = max(1, 1024 // max(B, 1))
    nblk = min(want, cap)
    chunk = -(-N // nblk)
    return dict(PL=PL, idle=256 - PL * CG, want=want, cap=cap, nblk=-(-N // chunk), chunk=chunk)


# id: (C, H, W, B, instantiation <NCH, XIT>, NT = 32-pixel row tiles)  -- tests/test_gpu_mlp_paths.py; hid = 4 C
PATH_CASES = {
    "C32_1x1": (32, 1, 1, 1, (1, 1), 1),
    "C64_1x128": (64, 1, 128, 3, (2, 1), 4),
    "C128_127x1": (128, 127, 1, 3, (4, 1), 4),
    "C160_5x7": (160, 5, 7, 3, (5, 1), 2),
    "C256_8x16": (256, 8, 16, 3, (8, 1), 4),
    "C256_8x13": (256, 8, 13, 3, (8, 1), 4),
    "C32_3x43": (32, 3, 43, 3, (1, 4), 5),
    "C64_13x32": (64, 13, 32, 3, (2, 4), 13),
    "C128_1x415": (128, 1, 415, 3, (4, 4), 13),
    "C160_11x23": (160, 11, 23, 3, (5, 4), 8),
    "C160_257x1": (160, 257, 1, 3, (5, 4), 9),
    "C160_16x26": (160, 16, 26, 3, (5, 4), 13),
}
# id: (B, N, C, slabs) of crd_mlp_reduce alone
REDUCE_CASES = {
    "one_pixel_128_lanes": (2, 1, 16, 1),
    "two_workgroups_ragged": (3, 129, 32, 2),
    "idle_threads": (2, 37, 320, 3),
    "one_lane_two_passes": (2, 5, 2048, 5),
    "production": (3, 104, 256, 16),
    "capped": (128, 40, 1024, 2),
}


def path_facts(C, H, W):
    """-> (supported value, <NCH, XIT>, NT, LDS bytes, second row tiles: wave pairs w with (w + 8) < NT) of a fused launch."""
    N = H * W
    NT = np_of(N) // 32
    return fused_supported(H, W, C, 4 * C), (C // 32, 1 if N <= 128 else 4), NT, lds_bytes(N, C), max(0, NT - 8)
