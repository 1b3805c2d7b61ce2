"""Every launch path of the encoder attention kernels (camradepth_amd/csrc/attention.hip, crd_attn_out_residual_stats in norm.hip)
against float64 references on the CPU, through the C ABI.

The launchers pick a kernel's geometry from the problem size and the developer switches are read once, so a path is reached by
shape only: every case asserts its path class through the host queries before it launches (tests/test_attn_paths_cpu.py pins the
same table without a GPU).  References are float64 on the same bf16-rounded operands with the kernels' documented rounding points;
tolerances are those of tests/test_gpu_ops.py for the same quantities.  Buffers whose contents the contract calls don't-care are
pre-filled with NaN (integer ones with a sentinel)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_attn_paths_cpu import OUT_BWD_CASES, SCORE_BWD_CASES, cdiv, out_bwd_class, score_bwd_class
from tests.test_gpu_igemm import assert_close
from tests.test_gpu_ops import L, P, ok
from tests.util import gval, sval, to_grad, zsum

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF16, I16 = torch.bfloat16, torch.int16


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def bf64(t):
    """bf16 rounding of a float64 tensor, as float64."""
    return t.to(BF16).double()


def bits(t):
    return t.view(I16) if t.dtype == BF16 else t.view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def refused(rc, *words):
    """A call the library refused before any launch: a status and a message that names the reason."""
    _, lb = L()
    torch.cuda.synchronize()
    msg = lb.crd_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def f32(v):
    """The value a C float argument takes."""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------------------------
# scores: S[b][n] = sum_h max_m bf16(bf16(q_h . k_h) * scale), idx = arg max
# ---------------------------------------------------------------------------------------------------------------------------------
def score_problem(B, N, M, heads, d, seed):
    g = torch.Generator().manual_seed(seed)
    C_ = heads * d
    q = torch.randn(B, N, C_, generator=g).to(BF16)
    k = torch.randn(B, M, C_, generator=g).to(BF16)
    return g, q, k


def scores_ref(q, k, heads, d, scale):
    """Row maxima [B][heads][N] in float64 with the kernel's two bf16 roundings (a few samples at a time: [b][h][N][M] doubles)."""
    B, N, _ = q.shape
    M = k.shape[1]
    q4, k4 = q.double().view(B, N, heads, d), k.double().view(B, M, heads, d)
    out = []
    for b0 in range(0, B, 8):
        att = bf64(bf64(torch.einsum("bnhd,bmhd->bhnm", q4[b0:b0 + 8], k4[b0:b0 + 8])) * scale)
        out.append(att.max(-1).values)
    return torch.cat(out)


def gather_keys(k, ii, heads, d):
    """k rows chosen by idx: [B][heads][N][d] float64."""
    B, M, _ = k.shape
    k4 = k.double().view(B, M, heads, d).permute(0, 2, 1, 3)                      # [B,h,M,d]
    return torch.gather(k4, 2, ii.permute(0, 2, 1).unsqueeze(-1).expand(-1, -1, -1, d))


def run_scores(q, k, heads, d, scale):
    """crd_attn_scores into NaN / sentinel filled outputs, checked against float64; returns device q, k, S, idx and idx on the host."""
    lib, lb = L()
    B, N, _ = q.shape
    M = k.shape[1]
    qd, kd = q.cuda(), k.cuda()
    S = nans(B, N)
    idx = torch.full((B, N, heads), -1, dtype=I16, device="cuda")
    ok(lb.crd_attn_scores(P(qd), P(kd), B, N, M, heads, d, scale, P(S), P(idx), lib.stream()), "attn_scores")
    ii = idx.cpu().long()
    assert int(ii.min()) >= 0 and int(ii.max()) < M, "arg-max out of range"     # (the backward gathers k rows through it)
    smax = scores_ref(q, k, heads, d, scale)
    assert_close(S.cpu(), smax.sum(1), "S", rel=2e-3, elem=1e-2)
    # the arg-max may differ where two scores tie after the bf16 roundings: the chosen key's score is the row maximum
    q4 = q.double().view(B, N, heads, d).permute(0, 2, 1, 3)
    chosen = bf64(bf64((q4 * gather_keys(k, ii, heads, d)).sum(-1)) * scale)
    assert float((chosen - smax).abs().max()) <= 1e-2 * float(smax.abs().max())
    return qd, kd, S, idx, ii


def score_bwd_ref(q, k, ii, dS, heads, d, scale):
    """float64 scatter reference of the score backward from the kernel's own idx (ii, on the host): dq [B][N][C] and dk [B][M][C]."""
    B, N, C_ = q.shape
    M = k.shape[1]
    gq = (scale * dS.double()).view(B, 1, N, 1)
    dq_ref = (gq * gather_keys(k, ii, heads, d)).permute(0, 2, 1, 3).reshape(B, N, C_)
    src = gq * q.double().view(B, N, heads, d).permute(0, 2, 1, 3)                # [B,h,N,d]
    row = (torch.arange(B * heads).view(B, heads, 1) * M + ii.permute(0, 2, 1)).reshape(-1)
    dk_ref = torch.zeros(B * heads * M, d, dtype=torch.float64).index_add_(0, row, src.reshape(-1, d))
    return dq_ref, dk_ref.view(B, heads, M, d).permute(0, 2, 1, 3).reshape(B, M, C_)


@pytest.mark.parametrize("shape", list(SCORE_BWD_CASES), ids=lambda s: "x".join(map(str, s)))
def test_score_backward_paths(shape):
    lib, lb = L()
    B, N, M, heads, d = shape
    parts_n, chunk, words, _ = SCORE_BWD_CASES[shape]
    assert score_bwd_class(lb, *shape) == SCORE_BWD_CASES[shape], "the launch rule moved this shape to another path"
    C_, scale = heads * d, f32(d ** -0.5)
    g, q, k = score_problem(B, N, M, heads, d, seed=11)
    qd, kd, S, idx, ii = run_scores(q, k, heads, d, scale)
    dS = torch.randn(B, N, generator=g)
    dSc = dS.cuda()
    dq_ref, dk_ref = score_bwd_ref(q, k, ii, dS, heads, d, scale)
    # the rank-one vector path that crd_attn_bwd runs in extra workgroups of the same launch
    t = to_grad(torch.randn(B, C_, generator=g)).cuda()
    wd = torch.zeros(C_, C_ + 8, dtype=BF16, device="cuda")
    wd[:, :C_] = (0.2 * torch.randn(C_, C_, generator=g)).to(BF16)
    tb0, es0 = nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_vec_bwd(P(t), P(wd), B, C_, C_ + 8, 1.0 / N, P(tb0), P(es0), lib.stream()), "attn_vec_bwd")

    # dk accumulator form (on the LDS path: one fixed-point add per owned value and workgroup; fallback: one per product)
    dq, dk = nans(B, N, C_, dtype=BF16), zsum(B, M, C_)
    ok(lb.crd_attn_scores_bwd(P(qd), P(kd), P(dSc), P(idx), B, N, M, heads, d, scale, P(dq), P(dk), None, lib.stream()),
       "attn_scores_bwd")
    assert_close(dq.float().cpu(), dq_ref, "dq")
    assert_close(gval(dk), dk_ref, "dk", rel=1e-4, elem=1e-4)

    if parts_n == 0:
        # the fallback has no partial form: it says which argument it needs, and launches nothing
        dq_u, dummy = nans(B, N, C_, dtype=BF16), nans(8)
        refused(lb.crd_attn_scores_bwd(P(qd), P(kd), P(dSc), P(idx), B, N, M, heads, d, scale, P(dq_u), None, P(dummy), lib.stream()),
                "crd_attn_scores_bwd", "dk accumulator")
        assert bool(torch.isnan(dq_u.float()).all()) and bool(torch.isnan(dummy).all())
        # fixed-point sums: a second run into a fresh accumulator is the same integers, whatever order the atomics landed in
        dq2, dk2 = nans(B, N, C_, dtype=BF16), zsum(B, M, C_)
        ok(lb.crd_attn_scores_bwd(P(qd), P(kd), P(dSc), P(idx), B, N, M, heads, d, scale, P(dq2), P(dk2), None, lib.stream()),
           "attn_scores_bwd again")
        assert same_bits(dq2, dq) and torch.equal(dk2, dk)
        dq3, dk3, tb1, es1 = nans(B, N, C_, dtype=BF16), zsum(B, M, C_), nans(B, C_, dtype=BF16), nans(B, C_)
        ok(lb.crd_attn_bwd(P(qd), P(kd), P(dSc), P(idx), B, N, M, heads, d, scale, P(dq3), P(dk3), None, P(t), P(wd), C_ + 8,
                           1.0 / N, P(tb1), P(es1), lib.stream()), "attn_bwd (fused)")
        assert same_bits(dq3, dq) and torch.equal(dk3, dk) and same_bits(tb1, tb0) and same_bits(es1, es0)
        return

    # partial form: one copy per workgroup with plain stores, folded by crd_sum_partials_bf16
    parts = nans(parts_n, B, M, C_)
    dq2 = nans(B, N, C_, dtype=BF16)
    ok(lb.crd_attn_scores_bwd(P(qd), P(kd), P(dSc), P(idx), B, N, M, heads, d, scale, P(dq2), None, P(parts), lib.stream()),
       "attn_scores_bwd partials")
    assert same_bits(dq2, dq)
    pc = parts.cpu()
    assert bool(torch.isfinite(pc).all()), "a partial copy kept its NaN fill"
    # (head, key) pairs nobody in a chunk chose: their rows are zero in that chunk's copy
    flat = ((((torch.arange(N) // chunk).view(1, N, 1) * B + torch.arange(B).view(B, 1, 1)) * heads
             + torch.arange(heads).view(1, 1, heads)) * M + ii).reshape(-1)
    counts = torch.bincount(flat, minlength=parts_n * B * heads * M).view(parts_n, B, heads, M).permute(0, 1, 3, 2)
    empty = counts == 0
    if M == 104:
        assert float(empty.double().mean()) > 0.25, "the case should leave many keys of a chunk unchosen"
    if M == 5:          # few keys: every (head, key) mask of every chunk is populated in each of its words
        assert int(counts.min()) >= words
    p5 = pc.view(parts_n, B, M, heads, d)
    assert bool((p5[empty] == 0).all()), "rows of unchosen keys must be zero"
    assert_close(pc.double().sum(0), dk_ref, "dk = sum of the partial copies", rel=1e-4, elem=1e-4)
    dkb = nans(B, M, C_, dtype=BF16)
    ok(lb.crd_sum_partials_bf16(P(parts), parts_n, B * M * C_, P(dkb), B * M * C_, lib.stream()), "sum_partials")
    assert_close(dkb.float().cpu(), bf64(dk_ref), "dk from partials (bf16)", rel=4e-3, elem=1e-2)
    # fused launch: bit for bit the unfused pair (a key's pixels are added in ascending order)
    parts3 = nans(parts_n, B, M, C_)
    dq3, tb1, es1 = nans(B, N, C_, dtype=BF16), nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_bwd(P(qd), P(kd), P(dSc), P(idx), B, N, M, heads, d, scale, P(dq3), None, P(parts3), P(t), P(wd), C_ + 8,
                       1.0 / N, P(tb1), P(es1), lib.stream()), "attn_bwd (fused)")
    assert same_bits(dq3, dq) and same_bits(tb1, tb0) and same_bits(es1, es0)
    assert same_bits(parts3, parts), "dk partials (fused launch)"


# M < 32, M a multiple of 32 / of 128, N < 32, every head count that changes the workgroup shape, head dims below the MFMA's K
SCORE_FWD_CASES = [(33, 1, 1, 8), (1, 32, 3, 16), (95, 128, 16, 8), (64, 96, 6, 48), (40, 160, 7, 56), (31, 31, 2, 64), (40, 31, 16, 64)]


@pytest.mark.parametrize("N,M,heads,d", SCORE_FWD_CASES)
def test_score_forward_edges(N, M, heads, d):
    lib, lb = L()
    B, C_, scale = 2, heads * d, f32(d ** -0.5)
    g, q, k = score_problem(B, N, M, heads, d, seed=12)
    qd, kd, S, idx, _ = run_scores(q, k, heads, d, scale)
    if C_ % 16:
        return
    # fused launch: the scores plus crd_attn_xbar_proj in cdiv(C, 64) extra workgroups per sample, of the score kernel's shape
    x = torch.randn(B, N, C_, generator=g).cuda()
    st, chan = zsum(B, C_ // 16, 2), zsum(B, C_, 2)
    ok(lb.crd_gn_stats(P(x), 1, C_, 0, B, N, C_, P(st), P(chan), lib.stream()), "gn_stats")
    gam, bet = (1 + 0.1 * torch.randn(C_, generator=g)).cuda(), (0.1 * torch.randn(C_, generator=g)).cuda()
    wf = (0.2 * torch.randn(C_, C_, generator=g)).to(BF16).cuda()
    xb0, u0 = nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_xbar_proj(P(chan), P(st), P(gam), P(bet), P(wf), B, N, C_, P(xb0), P(u0), lib.stream()), "xbar_proj")
    S2, idx2, xb1, u1 = nans(B, N), torch.full_like(idx, -1), nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_fwd(P(qd), P(kd), B, N, M, heads, d, scale, P(S2), P(idx2), P(chan), P(st), P(gam), P(bet), P(wf),
                       P(xb1), P(u1), lib.stream()), "attn_fwd (fused)")
    assert same_bits(S2, S) and torch.equal(idx2, idx) and same_bits(xb1, xb0) and same_bits(u1, u0)
    assert bool(torch.isfinite(u0).all()) and bool(torch.isfinite(xb0.float()).all())


def test_score_forward_refusals():
    """Shapes outside the kernel's limits are refused with a message, and nothing is launched."""
    lib, lb = L()
    q = torch.zeros(2 * 1040, dtype=BF16, device="cuda")
    S, idx = nans(2), torch.full((2 * 65,), -1, dtype=I16, device="cuda")
    refused(lb.crd_attn_scores(P(q), P(q), 1, 2, 2, 1, 72, 0.1, P(S), P(idx), lib.stream()), "crd_attn_scores", "head dim", "72")
    refused(lb.crd_attn_scores(P(q), P(q), 1, 2, 2, 17, 8, 0.1, P(S), P(idx), lib.stream()), "crd_attn_scores", "heads", "17")
    w, sums, par = torch.zeros(8, dtype=BF16, device="cuda"), zsum(8), torch.zeros(8, device="cuda")
    xb, u = nans(8, dtype=BF16), nans(8)
    refused(lb.crd_attn_fwd(P(q), P(q), 1, 2, 2, 65, 16, 0.1, P(S), P(idx), P(sums), P(sums), P(par), P(par), P(w), P(xb), P(u),
                            lib.stream()), "crd_attn_fwd", "1024")
    assert bool(torch.isnan(S).all()) and bool((idx == -1).all()) and bool(torch.isnan(u).all()) and bool(torch.isnan(xb.float()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# rank-one value path: xbar = bf16(mean_n GroupNorm(x)), u = W xbar; tb = bf16(t), es = inv_n W^T tb
# ---------------------------------------------------------------------------------------------------------------------------------
# C < 64 (lanes without a column), one and two 64-row parts, a ragged last part, a second 512-column pass, the documented limit
@pytest.mark.parametrize("C_", [16, 48, 64, 80, 528, 1024])
def test_rank_one_value_path(C_):
    lib, lb = L()
    g = torch.Generator().manual_seed(13)
    B, N, Cpad = 3, 37, C_ + 8
    x = torch.randn(B, N, C_, generator=g) + 0.5 * torch.randn(1, 1, C_, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    xd, gac, bec = x.cuda(), gamma.cuda(), beta.cuda()
    stats, chan = zsum(B, C_ // 16, 2), zsum(B, C_, 2)
    ok(lb.crd_gn_stats(P(xd), 1, C_, 0, B, N, C_, P(stats), P(chan), lib.stream()), "gn_stats")
    wp = (0.2 * torch.randn(C_, C_, generator=g)).to(BF16)                        # [co][ci]
    wf = wp.cuda()
    wd = torch.zeros(C_, Cpad, dtype=BF16, device="cuda")                         # [ci][co_pad]
    wd[:, :C_] = wp.t()
    xbar, u = nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_xbar_proj(P(chan), P(stats), P(gac), P(bec), P(wf), B, N, C_, P(xbar), P(u), lib.stream()), "xbar_proj")
    xn = F.group_norm(x.double().permute(0, 2, 1), C_ // 16, gamma.double(), beta.double(), 1e-5)
    assert_close(xbar.float().cpu(), xn.mean(2), "xbar", rel=4e-3, elem=1e-2)
    xbar1 = nans(B, C_, dtype=BF16)
    ok(lb.crd_attn_xbar(P(chan), P(stats), P(gac), P(bec), B, N, C_, P(xbar1), lib.stream()), "xbar")
    assert same_bits(xbar1, xbar)
    # The kernel takes these sums in fp64 on purpose (comment above matvec_rows), so the bound is derived, not measured: the
    # products of two bf16 values are exact in fp64, a sum of C <= 1024 of them is off by at most (C - 1) * 2^-53 * sum|w x|
    # < 2^-40 * sum|w x| in any order, and the one rounding to fp32 adds 2^-24 |u| (2^-23 allowed).
    w64, xb64 = wp.double(), xbar.cpu().double()
    u_ref, u_abs = xb64 @ w64.t(), xb64.abs() @ w64.abs().t()
    err = (u.cpu().double() - u_ref).abs()
    assert bool((err <= 2.0 ** -23 * u_ref.abs() + 2.0 ** -40 * u_abs).all()), f"u = W xbar: max err {float(err.max()):.3e}"
    # backward
    inv_n = f32(1.0 / N)
    t = to_grad(torch.randn(B, C_, generator=g)).cuda()
    tb, es = nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_vec_bwd(P(t), P(wd), B, C_, Cpad, inv_n, P(tb), P(es), lib.stream()), "attn_vec_bwd")
    assert same_bits(tb.cpu(), gval(t).to(BF16)), "tb = bf16(t)"
    tb64 = tb.cpu().double()
    es_ref, es_abs = (tb64 @ w64) * inv_n, (tb64.abs() @ w64.abs()) * inv_n
    err = (es.cpu().double() - es_ref).abs()                                       # (one more fp32 rounding: the inv_n multiply)
    assert bool((err <= 2 * 2.0 ** -23 * es_ref.abs() + 2.0 ** -40 * es_abs).all()), f"es = W^T tb / N: max err {float(err.max()):.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# output path: x1 = x + dp[b] * bf16(u[b][c] * S[b][n] + bp[c]) and its backward
# ---------------------------------------------------------------------------------------------------------------------------------
def residual_ref(x, u, S, bp, dp, got):
    """float64 x + dp * bf16(u S + bp).  The kernel forms u S + bp in fp32, so where the exact value lies within that error
    (2^-23 (|u S| + |bp|): one rounding each for the product and the sum, or one for a fused multiply-add) of a bf16 rounding
    boundary, either neighbour is a correct rounding: the reference takes the one the kernel took there, and such elements stay rare."""
    B = x.shape[0]
    x, u, S, bp = x.double(), u.double().unsqueeze(1), S.double().unsqueeze(2), bp.double()
    z = u * S + bp
    slack = 2.0 ** -23 * ((u * S).abs() + bp.abs())
    dps = torch.ones(B, 1, 1, dtype=torch.float64) if dp is None else dp.double().view(B, 1, 1)
    lo, hi = x + dps * bf64(z - slack), x + dps * bf64(z + slack)
    assert float((lo != hi).double().mean()) < 1e-3
    return torch.where((got.double() - lo).abs() <= (got.double() - hi).abs(), lo, hi)


def drop_path_scales(B, N, C_):
    """dp: 1 / 0.9 (a kept sample), 0 (a dropped one), then arbitrary values; NULL for one single-sample case."""
    if (B, N, C_) == (1, 61, 320):
        return None
    return torch.tensor([1.0 / 0.9, 0.0, 1.0, 0.7])[torch.arange(B) % 4]


def out_problem(B, N, C_, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, C_, generator=g) + 0.3 * torch.randn(B, 1, C_, generator=g)
    u, S, bp = torch.randn(B, C_, generator=g), torch.randn(B, N, generator=g), torch.randn(C_, generator=g)
    return g, x, u, S, bp, drop_path_scales(B, N, C_)


# lane layouts of k_attn_out_bwd: C = 8 (one lane per pixel), 16, 64, 256, 320 (idle lanes), 512 (a wave per pixel); a single pixel;
# the 256-pixel branch and the 1024 / B workgroup cap
OUT_CASES = [(3, 70, 8), (2, 33, 16), (2, 150, 64), (2, 97, 256), (1, 61, 320), (2, 40, 512), (1, 1, 64), (16, 2050, 64), (128, 2304, 16)]


@pytest.mark.parametrize("B,N,C_", OUT_CASES)
def test_output_path(B, N, C_):
    lib, lb = L()
    blocks, chunk = out_bwd_class(lb, B, N, C_)
    if (B, N) in OUT_BWD_CASES:
        assert (blocks, chunk) == OUT_BWD_CASES[(B, N)], "the launch rule moved this shape to another path"
    else:
        assert chunk <= 32 and blocks == cdiv(N, chunk), "a small-grid shape"
    g, x, u, S, bp, dp = out_problem(B, N, C_, seed=14)
    xc, uc, Sc, bpc = x.cuda(), u.cuda(), S.cuda(), bp.cuda()
    dpc = None if dp is None else dp.cuda()
    dps = torch.ones(B, 1, 1, dtype=torch.float64) if dp is None else dp.double().view(B, 1, 1)
    # forward
    x1 = nans(B, N, C_)
    ok(lb.crd_attn_out_residual(P(xc), P(uc), P(Sc), P(bpc), P(dpc), B, N, C_, P(x1), lib.stream()), "attn_out_residual")
    assert_close(x1.cpu(), residual_ref(x, u, S, bp, dp, x1.cpu()), "x1", rel=1e-5, elem=1e-5)
    gn = C_ % 16 == 0
    if gn:      # the same x1 plus the g16 sums crd_gn_stats(x1) would add
        x1b, st = nans(B, N, C_), zsum(B, C_ // 16, 2)
        ok(lb.crd_attn_out_residual_stats(P(xc), P(uc), P(Sc), P(bpc), P(dpc), B, N, C_, P(x1b), P(st), lib.stream()),
           "attn_out_residual_stats")
        assert same_bits(x1b, x1)
        xg = x1.cpu().double().view(B, N, C_ // 16, 16)
        assert_close(sval(st), torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1), "norm2 sums", rel=1e-5, elem=1e-5)
    # backward: dy = dp dx1; t = sum_n dy S, dbp_rows = sum_n dy, dS = sum_c dy u
    dx1 = torch.randn(B, N, C_, generator=g)

    def bwd_ref(d):
        dy = dps * d.double()
        return (dy * S.double().unsqueeze(2)).sum(1), dy.sum(1), (dy * u.double().unsqueeze(1)).sum(2)

    dx1c = dx1.cuda()
    t, dbp, dS = zsum(B, C_), zsum(B, C_), nans(B, N)
    ok(lb.crd_attn_out_bwd(P(dx1c), P(uc), P(Sc), P(dpc), B, N, C_, P(t), P(dbp), P(dS), lib.stream()), "attn_out_bwd")
    assert torch.equal(dx1c.cpu(), dx1), "crd_attn_out_bwd must not write dx1"
    t_ref, dbp_ref, dS_ref = bwd_ref(dx1)
    assert_close(gval(t), t_ref, "t", rel=1e-4, elem=1e-4)
    assert_close(gval(dbp), dbp_ref, "dbp rows (one per sample)", rel=1e-4, elem=1e-4)
    assert_close(dS.cpu(), dS_ref, "dS", rel=1e-4, elem=1e-4)
    if not gn:
        return
    # crd_attn_out_bwd_gn: Block.norm2's backward apply (fp32 input, accumulating into dx1) in front, in the same threads
    gamma, beta = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    dxn = (torch.randn(B, N, C_, generator=g)).to(BF16)
    gc_, bc_, dxnc = gamma.cuda(), beta.cuda(), dxn.cuda()
    stats = zsum(B, C_ // 16, 2)
    ok(lb.crd_gn_stats(P(xc), 1, C_, 0, B, N, C_, P(stats), None, lib.stream()), "gn_stats")
    r = zsum(B * C_ * 2 + B * (C_ // 16) * 2)
    ok(lb.crd_gn_bwd_reduce(P(xc), 1, C_, 0, P(dxnc), 0, C_, 0, B, N, C_, P(stats), 1, P(gc_), P(bc_), 0, None, P(r), None, 0,
                            lib.stream()), "gn_bwd_reduce")
    dg0, db0 = torch.randn(C_, generator=g), torch.randn(C_, generator=g)          # the parameter gradients accumulate
    dxb, dgb, dbb = dx1.clone().cuda(), dg0.clone().cuda(), db0.clone().cuda()
    tb, dbpb, dSb = zsum(B, C_), zsum(B, C_), nans(B, N)
    ok(lb.crd_attn_out_bwd_gn(P(dxb), P(uc), P(Sc), P(dpc), B, N, C_, P(tb), P(dbpb), P(dSb), P(xc), P(dxnc), P(stats), P(gc_), P(r),
                              P(dgb), P(dbb), lib.stream()), "attn_out_bwd_gn")
    # independent reference: float64 autograd through GroupNorm
    x64 = x.double().requires_grad_(True)
    F.group_norm(x64.permute(0, 2, 1), C_ // 16, gamma.double(), beta.double(), 1e-5).backward(dxn.double().permute(0, 2, 1))
    dx_ref = dx1.double() + x64.grad
    assert_close(dxb.cpu(), dx_ref, "dx1 += GroupNorm backward", rel=1e-3, elem=2e-3)
    t_ref, dbp_ref, dS_ref = bwd_ref(dxb.cpu())                                     # the sums of the dx1 the kernel stored
    assert_close(gval(tb), t_ref, "t (gn)", rel=1e-4, elem=1e-4)
    assert_close(gval(dbpb), dbp_ref, "dbp rows (gn)", rel=1e-4, elem=1e-4)
    assert_close(dSb.cpu(), dS_ref, "dS (gn)", rel=1e-4, elem=1e-4)
    # and the two launches it replaces (to fp32 rounding: they contract a*b+c differently; the parameter gradients are the same
    # integer sums added to the same start)
    dxa, dga, dba = dx1.clone().cuda(), dg0.clone().cuda(), db0.clone().cuda()
    ok(lb.crd_gn_bwd_apply(P(xc), 1, C_, 0, P(dxnc), 0, C_, 0, B, N, C_, P(stats), 1, P(gc_), P(bc_), 0, None, P(r), P(dga), P(dba),
                           P(dxa), 1, C_, 0, 1, None, 0, None, lib.stream()), "gn_bwd_apply")
    ta, dbpa, dSa = zsum(B, C_), zsum(B, C_), nans(B, N)
    ok(lb.crd_attn_out_bwd(P(dxa), P(uc), P(Sc), P(dpc), B, N, C_, P(ta), P(dbpa), P(dSa), lib.stream()), "attn_out_bwd")
    assert_close(dxb.cpu(), dxa.cpu(), "fused dx1", rel=1e-6, elem=2e-6)
    assert_close(gval(tb), gval(ta), "fused t", rel=1e-5, elem=1e-5)
    assert_close(gval(dbpb), gval(dbpa), "fused dbp", rel=1e-5, elem=1e-5)
    assert_close(dSb.cpu(), dSa.cpu(), "fused dS", rel=1e-5, elem=1e-5)
    assert same_bits(dgb, dga) and same_bits(dbb, dba)
    assert not torch.equal(dga.cpu(), dg0) and not torch.equal(dba.cpu(), db0)


def test_output_residual_grid_stride():
    """N * C / 8 items above 2048 workgroups of 256: the workgroups of crd_attn_out_residual take a second, partial round."""
    lib, lb = L()
    B, N, C_ = 1, 8200, 512
    assert cdiv(N * (C_ // 8), 256) > 2048
    g, x, u, S, bp, dp = out_problem(B, N, C_, seed=15)
    x1 = nans(B, N, C_)
    xc, uc, Sc, bpc, dpc = x.cuda(), u.cuda(), S.cuda(), bp.cuda(), dp.cuda()
    ok(lb.crd_attn_out_residual(P(xc), P(uc), P(Sc), P(bpc), P(dpc), B, N, C_, P(x1), lib.stream()), "attn_out_residual")
    assert_close(x1.cpu(), residual_ref(x, u, S, bp, dp, x1.cpu()), "x1", rel=1e-5, elem=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# folding the partial copies / the fixed-point accumulator into the bf16 operand of the next layer
# ---------------------------------------------------------------------------------------------------------------------------------
BIG_N = 8 * (2048 * 256 + 3)          # 2048 workgroups of 256 threads, 8 elements each, and a tail: the grid-stride loop's second round
assert cdiv(BIG_N // 8, 256) > 2048


def fold_ref(part, replicas, stride, n):
    """The kernel adds the copies in index order starting from zero, in fp32: so does this loop."""
    acc = torch.zeros(n)
    for r in range(replicas):
        acc = acc + part[r * stride:r * stride + n]
    return acc.to(BF16)


@pytest.mark.parametrize("replicas,n,pad", [(1, 296, 0), (3, 296, 0), (4, 296, 24), (5, 2056, 8), (52, 2056, 0), (2, BIG_N, 0)])
def test_sum_partials_bf16(replicas, n, pad):
    lib, lb = L()
    g = torch.Generator().manual_seed(16)
    stride = n + pad
    part = torch.randn(replicas * stride, generator=g) * (1 + 10 * torch.rand(replicas * stride, generator=g))
    if pad:         # replica_stride > n: what lies between the copies is not read
        part.view(replicas, stride)[:, n:] = NAN
    dst, pd = nans(n + 8, dtype=BF16), part.cuda()
    ok(lb.crd_sum_partials_bf16(P(pd), replicas, stride, P(dst), n, lib.stream()), "sum_partials")
    assert same_bits(dst[:n].cpu(), fold_ref(part, replicas, stride, n)), "bf16(sum of the copies in index order)"
    assert bool(torch.isnan(dst[n:].float()).all()), "wrote past n"


def test_gsum_to_bf16_grid_stride():
    lib, lb = L()
    g = torch.Generator().manual_seed(17)
    src = to_grad(torch.randn(BIG_N, generator=g) * 3).cuda()
    dst = nans(BIG_N + 8, dtype=BF16)
    ok(lb.crd_gsum_to_bf16(P(src), P(dst), BIG_N, lib.stream()), "gsum_to_bf16")
    assert same_bits(dst[:BIG_N].cpu(), gval(src).to(BF16))
    assert bool(torch.isnan(dst[BIG_N:].float()).all()), "wrote past n"
