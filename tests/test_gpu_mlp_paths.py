"""GPU: every instantiation and pixel edge of the fused Mlp (crd_mlp_fwd + crd_mlp_reduce, csrc/mlp_fused.hip) against the float64
stage reference of tests/mlp_ref.py, whose docstring derives the bounds.

(a) test_fused_mlp_paths: the twelve shapes of mlp_ref.PATH_CASES -- all nine instantiations of k_mlp_fwd, N = 1, H = 1, W = 1, the
    N = 128 / 129 switch, full and ragged row tiles, NT = 8 / 9, the largest LDS footprint.  Every stage is checked on its own, fed with
    what the device stored for the stage before, and the end-to-end assertions of tests/test_gpu_mlp.py run at their tolerances.  Every
    output buffer ends in a tail of sentinels that must survive.
(b) the same test launches the inference form (xn = h1 = h2 = h3 = NULL; the reduce without sums; dp = NULL) and a second training-form
    run: bit-identical.
(c) test_reduce_exact: crd_mlp_reduce alone on dyadic rationals chosen so that every fp32 operation is exact: x2 and the integer sums
    must EQUAL the float64 result, bf16 ties with and without the bias included.
(d) test_unsupported_shape_leaves_outputs_untouched; the predicate table itself is in tests/test_mlp_ref_cpu.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import mlp_ref as R
from tests.test_gpu_igemm import assert_close, bf
from tests.test_gpu_mlp import slab_sums
from tests.util import sval

pytestmark = pytest.mark.gpu

SENT, TAIL = -77.0, 4096


def L():
    from camradepth_amd import lib
    return lib, lib.load()


def tailed(numel, dtype, fill):
    """A flat buffer of numel values `fill` followed by TAIL sentinels."""
    buf = torch.full((numel + TAIL,), SENT, dtype=dtype, device="cuda")
    buf[:numel] = fill
    return buf


def tails_intact(bufs):
    for name, (buf, numel) in bufs.items():
        assert bool((buf[numel:] == SENT).all()), f"{name}: written past its end"


def ptr(t):
    return None if t is None else t.data_ptr()


def to_device(inp):
    t = {k: inp[k].cuda().contiguous() for k in ("x1", "x1_stats", "b1", "b2", "w9", "bd", "g0", "b0", "g1", "b1n", "g2", "b2n", "dp")}
    t["w1"], t["w2"] = inp["w1"].to(torch.bfloat16).cuda().contiguous(), inp["w2"].to(torch.bfloat16).cuda().contiguous()
    return t


def launch(inp, t, save=True, sums=True, dp="inp", part_in=None):
    """One crd_mlp_fwd (unless part_in is given) + crd_mlp_reduce into fresh NaN-filled buffers with sentinel tails -> dict of device tensors."""
    lib, lb = L()
    B, H, W, Cs, hid, N = (inp[k] for k in ("B", "H", "W", "C", "hid", "N"))
    slabs = hid // 64
    nan = float("nan")
    bufs, o = {}, {}

    def out(name, shape, dtype, fill):
        n = 1
        for s in shape:
            n *= s
        buf = tailed(n, dtype, fill)
        bufs[name] = (buf, n)
        o[name] = buf[:n].view(*shape)
        return buf

    if part_in is None:
        if save:
            out("xn", (B, N, Cs), torch.bfloat16, nan)
            for k in ("h1", "h2", "h3"):
                out(k, (B, N, hid), torch.bfloat16, nan)
        out("h1_stats", (B, hid // 16, 2), torch.int64, 0)
        out("h2_stats", (B, hid // 16, 2), torch.int64, 0)
        out("part", (slabs, B, N, Cs), torch.float32, nan)
        d = lib.MlpDesc()
        d.x1, d.x1_stats, d.norm_gamma, d.norm_beta = ptr(t["x1"]), ptr(t["x1_stats"]), ptr(t["g0"]), ptr(t["b0"])
        d.w_fc1, d.b_fc1, d.norm1_gamma, d.norm1_beta = ptr(t["w1"]), ptr(t["b1"]), ptr(t["g1"]), ptr(t["b1n"])
        d.w9, d.b_dw, d.norm2_gamma, d.norm2_beta = ptr(t["w9"]), ptr(t["bd"]), ptr(t["g2"]), ptr(t["b2n"])
        d.w_fc2 = ptr(t["w2"])
        d.xn, d.h1, d.h2, d.h3 = (ptr(o[k]) for k in ("xn", "h1", "h2", "h3")) if save else (None, None, None, None)
        d.h1_stats, d.h2_stats, d.fc2_partials = ptr(o["h1_stats"]), ptr(o["h2_stats"]), ptr(o["part"])
        d.B, d.H, d.W, d.C, d.hidden = B, H, W, Cs, hid
        lib.check(lb.crd_mlp_fwd(C.byref(d), lib.stream()), "crd_mlp_fwd")
    else:
        o["part"] = part_in
    out("x2", (B, N, Cs), torch.float32, nan)
    if sums:
        out("x2_stats", (B, Cs // 16, 2), torch.int64, 0)
        out("x2_chan", (B, Cs, 2), torch.int64, 0)
    dpt = t["dp"] if isinstance(dp, str) else dp
    lib.check(lb.crd_mlp_reduce(ptr(o["part"]), slabs, ptr(t["x1"]), ptr(t["b2"]), ptr(dpt), B, N, Cs, ptr(o["x2"]),
                                ptr(o.get("x2_stats")), ptr(o.get("x2_chan")), lib.stream()), "crd_mlp_reduce")
    torch.cuda.synchronize()
    tails_intact(bufs)
    return o


def end_to_end_fp32(inp):
    """The torch fp32 chain of tests/test_gpu_mlp.py with the reference's rounding points ([B][C][N] layout)."""
    B, H, W, Cs, hid, N = (inp[k] for k in ("B", "H", "W", "C", "hid", "N"))
    xc = inp["x1"].permute(0, 2, 1)
    wd = inp["w9"].t().reshape(hid, 1, 3, 3)
    xn = bf(F.group_norm(xc, Cs // 16, inp["g0"], inp["b0"], 1e-5))
    h1 = bf(F.conv1d(xn, inp["w1"].unsqueeze(-1), inp["b1"]))
    h1n = bf(F.group_norm(h1, hid // 16, inp["g1"], inp["b1n"], 1e-5))
    h2 = bf(F.conv2d(h1n.reshape(B, hid, H, W), wd, inp["bd"], padding=1, groups=hid)).reshape(B, hid, N)
    h3 = bf(F.gelu(F.group_norm(h2, hid // 64, inp["g2"], inp["b2n"], 1e-5)))
    o = bf(F.conv1d(h3, inp["w2"].unsqueeze(-1), inp["b2"]))
    x2 = xc + inp["dp"].view(B, 1, 1) * o
    return {k: v.permute(0, 2, 1) for k, v in dict(xn=xn, h1=h1, h2=h2, h3=h3, x2=x2).items()}


@pytest.mark.parametrize("case", list(R.PATH_CASES))
def test_fused_mlp_paths(case):
    lib, lb = L()
    Cs, H, W, B, inst, NT = R.PATH_CASES[case]
    hid, N = 4 * Cs, H * W
    # ---- the case is the edge it is here for
    sup, inst_f, NT_f, lds, second = R.path_facts(Cs, H, W)
    assert lb.crd_mlp_fused_supported(H, W, Cs, hid) == sup == hid // 64
    assert inst_f == inst and (N <= 128) == (inst[1] == 1) and NT_f == NT == (N + 31) // 32 and lds <= 160 * 1024
    if case == "C160_16x26":
        assert lds == 153088
    if case in ("C160_11x23", "C160_257x1"):
        assert second == (0 if case == "C160_11x23" else 1)
    inp = R.make_inputs(B, H, W, Cs)
    assert torch.equal(inp["dp"], torch.tensor([1.0 / 0.9, 0.0, 1.0])[:B])
    assert min(float(inp[k].abs().min()) for k in ("b1", "bd", "b2")) > 0
    t = to_device(inp)

    # ---- (a) the training form: every stage against float64 within its derived bound
    o = launch(inp, t)
    dev = {k: v.cpu() for k, v in o.items()}
    assert not bool(torch.isnan(dev["part"]).any()) and not bool(torch.isnan(dev["x2"]).any())
    report = R.stage_report(inp, dev)
    print(f"{case}: max |got - v| / bound (fp32 slack used) per stage: " + ", ".join(f"{k} {v:.4f} ({s:.3f})" for k, (v, s) in report.items()))
    for k, (v, s) in report.items():
        assert v <= 1.0, f"{case}: stage {k} is at {v:.4f} of its bound"
    assert_close(sval(o["h1_stats"]), slab_sums(dev["h1"].float()), "h1 sums", rel=1e-5, elem=1e-5)
    assert_close(sval(o["h2_stats"]), slab_sums(dev["h2"].float()), "h2 sums", rel=1e-5, elem=1e-5)
    assert_close(sval(o["x2_stats"]), slab_sums(dev["x2"]), "x2 g16 sums", rel=1e-5, elem=1e-5)
    xd = dev["x2"].double()
    assert_close(sval(o["x2_chan"]), torch.stack([xd.sum(1), (xd * xd).sum(1)], -1).float(), "x2 channel sums", rel=1e-5, elem=1e-5)
    # ---- the end-to-end assertions of tests/test_gpu_mlp.py, at their tolerances
    ref = end_to_end_fp32(inp)
    assert_close(dev["xn"].float(), ref["xn"], "Block.norm2(x1)")
    assert_close(dev["h1"].float(), ref["h1"], "h1 = fc1")
    assert_close(dev["h2"].float(), ref["h2"], "h2 = depthwise", rel=8e-3, elem=2e-2)
    assert_close(dev["h3"].float(), ref["h3"], "h3 = GELU(norm2)", rel=8e-3, elem=3e-2)
    assert_close(dev["x2"], ref["x2"], "x2", rel=4e-3, elem=2e-2)

    # ---- (b) a second training-form run and the inference form give the same bits
    again = launch(inp, t)
    for k in o:
        assert torch.equal(again[k], o[k]), f"second run: {k} differs"
    inf = launch(inp, t, save=False, sums=False)
    assert set(inf) == {"h1_stats", "h2_stats", "part", "x2"}
    for k in inf:
        assert torch.equal(inf[k], o[k]), f"inference form: {k} differs from the training form"
    ones = launch(inp, t, sums=False, dp=torch.ones(B, device="cuda"), part_in=o["part"])
    none = launch(inp, t, sums=False, dp=None, part_in=o["part"])
    assert torch.equal(ones["x2"], none["x2"]), "dp = NULL is not dp = 1"
    v, bound = R.stage_x2(dev["part"], inp["x1"], inp["b2"], None)
    assert bool(((none["x2"].cpu().double() - v).abs() <= bound).all())


def rne8(k):
    """Integers to 8 significant bits, ties to even, in integer arithmetic (|k| < 2048): bf16 rounding of k / 32."""
    a = k.abs()
    sp = 1 << ((a >= 256).long() + (a >= 512).long() + (a >= 1024).long())
    q, rem = a // sp, a % sp
    up = (2 * rem > sp) | ((2 * rem == sp) & (q % 2 == 1))
    return torch.sign(k) * (q + up.long()) * sp


def reduce_problem(B, N, Cc, slabs):
    """Synthetic partials, x1, bias and dp (host, float64 values that fp32 holds exactly) with the exact float64 result and its sums."""
    g = torch.Generator().manual_seed(1000 * Cc + N)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64)

    # ---- everything in units of 1/32.  T = slab sum + bias: exact bf16 values, ties (odd in 256..511; 2 mod 4 in 512..1023), neighbours
    kind = ri(0, 6, B, N, Cc)
    sign = 2 * ri(0, 2, B, N, Cc) - 1
    T = torch.where(kind == 0, ri(-255, 256, B, N, Cc),
                    torch.where(kind <= 2, sign * (2 * ri(128, 256, B, N, Cc) + 1),
                                torch.where(kind == 3, sign * 2 * ri(128, 256, B, N, Cc), sign * ri(512, 1024, B, N, Cc))))
    bias = torch.tensor([0, 1, 0, -3, 0, 2, 0, -1], dtype=torch.int64).repeat(Cc // 8)
    S = T - bias                                                     # the slab sum
    parts = ri(-64, 65, slabs, B, N, Cc)
    parts[slabs - 1] = S - parts[:slabs - 1].sum(0)
    dp = torch.tensor([1.25, 0.5, 0.0, 1.0], dtype=torch.float64).repeat(-(-B // 4))[:B]
    o_r = rne8(T)
    assert torch.equal(o_r.double() / 32, R.bf16(T.double() / 32))   # the integer rounding is torch's bf16 conversion

    def half(k):                                                     # exactly between two bf16 values
        sp = 1 << ((k.abs() >= 256).long() + (k.abs() >= 512).long())
        return (sp > 1) & (2 * (k.abs() % sp) == sp)

    if B * N * Cc >= 4096:
        nb, wb = bias.expand(B, N, Cc) == 0, bias.expand(B, N, Cc) % 2 != 0
        assert int((half(T) & nb).sum()) > 0                          # a tie without a bias
        assert int((half(T) & wb & ~half(S)).sum()) > 0               # a tie only with the bias: round(sum) + bias differs
        assert int((half(S) & wb & ~half(T)).sum()) > 0               # a tie only without it
        assert int(((rne8(T) != T) & ~half(T)).sum()) > 0             # plain inexact values: truncation differs
    target = ri(-16, 17, B, N, Cc)                                    # x2, so that its sums and squares stay small
    x1 = target.double() / 32 - dp.view(B, 1, 1) * o_r.double() / 32
    assert torch.equal(x1.float().double(), x1) and torch.equal((dp.view(B, 1, 1) * o_r.double() / 32).float().double(), dp.view(B, 1, 1) * o_r.double() / 32)
    # float64 result from the definition
    o64 = parts.double().sum(0) / 32 + bias.double() / 32
    x2_ref = x1 + dp.view(B, 1, 1) * R.bf16(o64)
    assert torch.equal(x2_ref * 32, target.double())
    # |x2| <= 16 / 32: every running fp32 sum of a workgroup (at most N pixels x 16 channels) stays an integer below 2^24 on its
    # grid, 1/32 for x2 and 1/1024 for its square, and the fixed-point totals (2^-20) hold both exactly
    assert N * 16 * 16 < 2 ** 24 and N * 16 * 16 * 16 < 2 ** 24
    st_ref = R.to_stat(R.slab_sums(x2_ref))
    ch_ref = R.to_stat(torch.stack([x2_ref.sum(1), (x2_ref * x2_ref).sum(1)], -1))
    return dict(part=parts.double() / 32, x1=x1, b2=bias.double() / 32, dp=dp, x2=x2_ref, stats=st_ref, chan=ch_ref)


@pytest.mark.parametrize("case", list(R.REDUCE_CASES))
def test_reduce_exact(case):
    lib, lb = L()
    B, N, Cc, slabs = R.REDUCE_CASES[case]
    P = R.reduce_partition(B, N, Cc)
    # ---- the case is the edge it is named for (the formulas of crd_mlp_reduce)
    want = {"one_pixel_128_lanes": P["PL"] == 128 and N == 1 and P["nblk"] == 1,
            "two_workgroups_ragged": P["nblk"] == 2 and N % P["chunk"] != 0 and P["chunk"] % P["PL"] != 0,
            "idle_threads": P["idle"] == 16,
            "one_lane_two_passes": P["PL"] == 1 and 4 < slabs <= 8 and P["chunk"] == 2,
            "production": P["PL"] == 8 and P["nblk"] == 7 and slabs == 16,
            "capped": P["want"] > P["cap"] and P["nblk"] == P["cap"] and P["chunk"] > 2 * P["PL"]}[case]
    assert want, (case, P)
    q = reduce_problem(B, N, Cc, slabs)
    x2_ref, st_ref, ch_ref = q["x2"], q["stats"], q["chan"]
    part_d, x1_d, b2_d, dp_d = (q[k].float().cuda() for k in ("part", "x1", "b2", "dp"))
    x2 = tailed(B * N * Cc, torch.float32, float("nan"))
    st, ch = tailed(B * (Cc // 16) * 2, torch.int64, 0), tailed(B * Cc * 2, torch.int64, 0)
    lib.check(lb.crd_mlp_reduce(ptr(part_d), slabs, ptr(x1_d), ptr(b2_d), ptr(dp_d), B, N, Cc, ptr(x2), ptr(st), ptr(ch), lib.stream()),
              "crd_mlp_reduce")
    torch.cuda.synchronize()
    tails_intact({"x2": (x2, B * N * Cc), "stats": (st, B * (Cc // 16) * 2), "chan": (ch, B * Cc * 2)})
    got = x2[:B * N * Cc].view(B, N, Cc).cpu().double()
    bad = int((got != x2_ref).sum())
    assert bad == 0, f"{case}: {bad} values of x2 differ from the exact result, the largest by {(got - x2_ref).abs().max().item():.3e}"
    assert torch.equal(st[:B * (Cc // 16) * 2].view(B, Cc // 16, 2).cpu(), st_ref), f"{case}: g16 sums"
    assert torch.equal(ch[:B * Cc * 2].view(B, Cc, 2).cpu(), ch_ref), f"{case}: channel sums"


def test_unsupported_shape_leaves_outputs_untouched():
    """C = 256 at N = 129: the library's unsupported status, nothing launched, the NaN-filled outputs and the zeroed sums as they were."""
    lib, lb = L()
    B, H, W, Cs = 2, 3, 43, 256
    hid, N = 4 * Cs, H * W
    assert lb.crd_mlp_fused_supported(H, W, Cs, hid) == 0 == R.fused_supported(H, W, Cs, hid)
    nan = float("nan")
    f32 = torch.full((max(hid // 64 * B * N * Cs, 9 * hid),), nan, device="cuda")
    b16 = torch.full((B * N * hid,), nan, dtype=torch.bfloat16, device="cuda")
    i64 = torch.zeros(B * hid // 16 * 2, dtype=torch.int64, device="cuda")
    d = lib.MlpDesc()
    for n in ("x1", "norm_gamma", "norm_beta", "b_fc1", "norm1_gamma", "norm1_beta", "w9", "b_dw", "norm2_gamma", "norm2_beta", "fc2_partials"):
        setattr(d, n, ptr(f32))
    for n in ("w_fc1", "w_fc2", "xn", "h1", "h2", "h3"):
        setattr(d, n, ptr(b16))
    for n in ("x1_stats", "h1_stats", "h2_stats"):
        setattr(d, n, ptr(i64))
    d.B, d.H, d.W, d.C, d.hidden = B, H, W, Cs, hid
    rc = lb.crd_mlp_fwd(C.byref(d), lib.stream())
    torch.cuda.synchronize()
    assert rc == -2 and b"crd_mlp_fwd" in lb.crd_last_error(), (rc, lb.crd_last_error())
    assert bool(torch.isnan(f32).all()) and bool(torch.isnan(b16).all()) and not bool(i64.any())
