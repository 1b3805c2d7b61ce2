"""crd_attn_bwd_fused and crd_attn_dk_fold (camradepth_amd/csrc/attention.hip) against the launches they replace and against float64.

The fused launch runs crd_attn_out_bwd(_gn) and the partial form of crd_attn_scores_bwd as one workgroup-local pass: dx1, dS, dq and
the dK partials must be the SAME BITS as the pair's; t and dbp_rows are fixed-point sums of float partial sums over other pixel chunks
and are held to the float64 reference with the tolerance tests/test_gpu_attention.py uses for them (rel = elem = 1e-4), and to the
pair's values with the tolerance that file uses between two forms of one computation (rel = elem = 1e-5: tighter than either form's
bound against the reference).  Both forms run the same index / row / scatter functions and copies of one text otherwise, so equal bits alone would not
catch an error the two have in common: the fused form's dS, dq, the sum of its dK partials and the dK that crd_attn_dk_fold makes of them are held to float64 as
well, with the tolerances tests/test_gpu_attention.py puts on the pair's.  Problem builders and references come from
tests/test_gpu_attention.py; outputs are pre-filled with NaN."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from tests.test_attn_paths_cpu import score_bwd_class
from tests.test_gpu_attention import BF16, bf64, f32, nans, out_problem, refused, run_scores, same_bits, score_bwd_ref, score_problem
from tests.test_gpu_igemm import assert_close
from tests.test_gpu_ops import L, P, ok
from tests.util import gval, to_grad, zsum

pytestmark = pytest.mark.gpu

# (B, N, M, heads, d) -> (parts, chunk, mask words): what the shape reaches
CASES = {
    (2, 600, 104, 2, 32): (10, 60, 2),          # two mask words
    (2, 641, 104, 2, 32): (11, 59, 2),          # ragged last chunk
    (64, 130, 35, 2, 32): (2, 65, 3),           # third mask word, single bit
    (2, 416, 104, 4, 40): (13, 32, 1),          # C = 160: 20 granules on 32 lanes, a head boundary inside a granule row
    (2, 104, 104, 8, 32): (4, 26, 1),           # stage-4 geometry
    (1, 1, 4, 1, 8): (1, 1, 1),                 # one pixel, C = 8
    (2, 150, 104, 8, 64): (5, 30, 1),           # C = 512: 64 lanes per pixel
}


def attention_problem(shape, seed):
    """q, k, idx of the score backward and dx1, u, S, x, dxn, gamma of the output backward, on the device."""
    B, N, M, heads, d = shape
    C_, scale = heads * d, f32(d ** -0.5)
    _, q, k = score_problem(B, N, M, heads, d, seed=seed)
    qd, kd, _, idx, ii = run_scores(q, k, heads, d, scale)
    g, x, u, S, _, _ = out_problem(B, N, C_, seed=seed + 1)
    p = dict(B=B, N=N, M=M, heads=heads, d=d, C=C_, scale=scale, q=qd, k=kd, idx=idx, x=x, u=u, S=S, xc=x.cuda(), uc=u.cuda(), Sc=S.cuda())
    p["q_host"], p["k_host"], p["idx_host"] = q, k, ii
    p["dx1"] = torch.randn(B, N, C_, generator=g)
    p["dp"] = torch.tensor([1.0 / 0.9, 0.0, 1.0, 0.7])[torch.arange(B) % 4]
    p["gamma"], p["beta"] = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    p["dxn"] = torch.randn(B, N, C_, generator=g).to(BF16)
    p["dg0"], p["db0"] = torch.randn(C_, generator=g), torch.randn(C_, generator=g)        # the parameter gradients accumulate
    return p


def groupnorm_sums(p):
    """stats of x and the sums crd_gn_bwd_reduce leaves for Block.norm2's backward apply (as tests/test_gpu_attention.py sets them up)."""
    lib, lb = L()
    B, N, C_ = p["B"], p["N"], p["C"]
    gc_, bc_, dxnc = p["gamma"].cuda(), p["beta"].cuda(), p["dxn"].cuda()
    stats, r = zsum(B, C_ // 16, 2), zsum(B * C_ * 2 + B * (C_ // 16) * 2)
    ok(lb.crd_gn_stats(P(p["xc"]), 1, C_, 0, B, N, C_, P(stats), None, lib.stream()), "gn_stats")
    ok(lb.crd_gn_bwd_reduce(P(p["xc"]), 1, C_, 0, P(dxnc), 0, C_, 0, B, N, C_, P(stats), 1, P(gc_), P(bc_), 0, None, P(r), None, 0,
                            lib.stream()), "gn_bwd_reduce")
    return gc_, dxnc, stats, r


def run_forms(p, parts_n, pre, dp, dgam, want_ds):
    """The existing pair and the fused entry on copies of the same inputs; returns both sets of outputs."""
    lib, lb = L()
    B, N, M, heads, d, C_, scale = (p[k] for k in ("B", "N", "M", "heads", "d", "C", "scale"))
    dpc = p["dp"].cuda() if dp else None
    gn = p["gn"] if pre else (None, None, None, None)
    gc_, dxnc, stats, r = gn
    out = []
    for fused in (False, True):
        dx = p["dx1"].clone().cuda()
        t, dbp = zsum(B, C_), zsum(B, C_)
        dS = nans(B, N) if want_ds or not fused else None
        dq, parts = nans(B, N, C_, dtype=BF16), nans(parts_n, B, M, C_)
        dg, db = (p["dg0"].clone().cuda(), p["db0"].clone().cuda()) if pre and dgam else (None, None)
        if fused:
            ok(lb.crd_attn_bwd_fused(P(dx), P(p["uc"]), P(p["Sc"]), P(dpc), P(p["q"]), P(p["k"]), P(p["idx"]), B, N, M, heads, d, scale,
                                     P(t), P(dbp), P(dS), P(dq), P(parts), P(p["xc"]) if pre else None, P(dxnc), P(stats), P(gc_), P(r),
                                     P(dg), P(db), lib.stream()), "attn_bwd_fused")
        else:
            if pre:
                ok(lb.crd_attn_out_bwd_gn(P(dx), P(p["uc"]), P(p["Sc"]), P(dpc), B, N, C_, P(t), P(dbp), P(dS), P(p["xc"]), P(dxnc), P(stats),
                                          P(gc_), P(r), P(dg), P(db), lib.stream()), "attn_out_bwd_gn")
            else:
                ok(lb.crd_attn_out_bwd(P(dx), P(p["uc"]), P(p["Sc"]), P(dpc), B, N, C_, P(t), P(dbp), P(dS), lib.stream()), "attn_out_bwd")
            ok(lb.crd_attn_scores_bwd(P(p["q"]), P(p["k"]), P(dS), P(p["idx"]), B, N, M, heads, d, scale, P(dq), None, P(parts),
                                      lib.stream()), "attn_scores_bwd partials")
        dk = None
        if fused:       # the fold this form continues with (its vector-path riders: tests further down)
            dk, tb, es = nans(B, M, C_, dtype=BF16), nans(B, C_, dtype=BF16), nans(B, C_)
            ok(lb.crd_attn_dk_fold(P(parts), parts_n, B * M * C_, P(dk), B * M * C_, P(t), P(p["wd"]), B, C_, C_ + 8, f32(1.0 / N), P(tb), P(es),
                                   lib.stream()), "attn_dk_fold")
            dk = dk.float().cpu()
        out.append(dict(dx=dx.cpu(), t=gval(t), dbp=gval(dbp), dS=None if dS is None else dS.cpu(), dq=dq.cpu(), parts=parts.cpu(), dk=dk,
                        dg=None if dg is None else dg.cpu(), db=None if db is None else db.cpu()))
    return out


@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "x".join(map(str, s)))
def test_fused_launch_equals_the_pair(shape):
    lib, lb = L()
    B, N, M, heads, d = shape
    parts_n = CASES[shape][0]
    assert score_bwd_class(lb, *shape)[:3] == CASES[shape], "the launch rule moved this shape to another path"
    assert lb.crd_attn_bwd_fused_supported(*shape) == parts_n
    p = attention_problem(shape, seed=21)
    C_ = p["C"]
    p["wd"] = torch.zeros(C_, C_ + 8, dtype=BF16, device="cuda")          # (the riders of crd_attn_dk_fold need a weight)
    can_pre = C_ % 16 == 0
    if can_pre:
        p["gn"] = groupnorm_sums(p)
        # float64 autograd through GroupNorm: the parameter gradients
        x64, g64, b64 = p["x"].double().requires_grad_(True), p["gamma"].double().requires_grad_(True), p["beta"].double().requires_grad_(True)
        F.group_norm(x64.permute(0, 2, 1), C_ // 16, g64, b64, 1e-5).backward(p["dxn"].double().permute(0, 2, 1))
        dg_ref, db_ref = p["dg0"].double() + g64.grad, p["db0"].double() + b64.grad
    else:       # C = 8: the GroupNorm form needs 16-channel groups, and says so
        some = nans(8)
        refused(lb.crd_attn_bwd_fused(P(p["dx1"].cuda()), P(p["uc"]), P(p["Sc"]), None, P(p["q"]), P(p["k"]), P(p["idx"]), B, N, M, heads, d,
                                      p["scale"], P(zsum(B, C_)), P(zsum(B, C_)), None, P(nans(B, N, C_, dtype=BF16)),
                                      P(nans(parts_n, B, M, C_)), P(p["xc"]), P(some), P(zsum(8)), P(some), P(zsum(8)), None, None,
                                      lib.stream()), "crd_attn_bwd_fused", "16")
    for pre in ((False, True) if can_pre else (False,)):
        for dp in (True, False):
            dps = p["dp"].double().view(B, 1, 1) if dp else torch.ones(B, 1, 1, dtype=torch.float64)
            for dgam in ((True, False) if pre else (False,)):
                for want_ds in (True, False):
                    what = f"pre={pre} dp={dp} dgamma={dgam} dS={want_ds}"
                    a, b = run_forms(p, parts_n, pre, dp, dgam, want_ds)
                    assert same_bits(b["dx"], a["dx"]), f"dx1 ({what})"
                    if not pre:
                        assert torch.equal(b["dx"], p["dx1"]), "without the GroupNorm form dx1 is not written"
                    if want_ds:
                        assert same_bits(b["dS"], a["dS"]), f"dS ({what})"
                    assert same_bits(b["dq"], a["dq"]), f"dq ({what})"
                    assert bool(torch.isfinite(b["parts"]).all()), "a partial copy kept its NaN fill"
                    assert same_bits(b["parts"], a["parts"]), f"dk partials ({what})"
                    dy = dps * a["dx"].double()                               # the dx1 both forms continue with
                    t_ref, dbp_ref = (dy * p["S"].double().unsqueeze(2)).sum(1), dy.sum(1)
                    for form, o in (("pair", a), ("fused", b)):
                        assert_close(o["t"], t_ref, f"t ({form}, {what})", rel=1e-4, elem=1e-4)
                        assert_close(o["dbp"], dbp_ref, f"dbp rows ({form}, {what})", rel=1e-4, elem=1e-4)
                    assert_close(b["t"], a["t"], f"t, fused against the pair ({what})", rel=1e-5, elem=1e-5)
                    assert_close(b["dbp"], a["dbp"], f"dbp rows, fused against the pair ({what})", rel=1e-5, elem=1e-5)
                    # the fused form against float64: dS of the dx1 it stored, then the scatter of scale * dS through its idx
                    dS_ref = (dy * p["u"].double().unsqueeze(1)).sum(2)
                    dq_ref, dk_ref = score_bwd_ref(p["q_host"], p["k_host"], p["idx_host"], dS_ref, heads, d, p["scale"])
                    if want_ds:
                        assert_close(b["dS"], dS_ref, f"dS (fused, {what})", rel=1e-4, elem=1e-4)
                    assert_close(b["dq"].float(), dq_ref, f"dq (fused, {what})")
                    assert_close(b["parts"].double().sum(0), dk_ref, f"dk = sum of the partial copies (fused, {what})", rel=1e-4, elem=1e-4)
                    assert_close(b["dk"], bf64(dk_ref), f"dk from crd_attn_dk_fold (fused, {what})", rel=4e-3, elem=1e-2)
                    if dgam:        # the same integer sums added to the same start
                        assert same_bits(b["dg"], a["dg"]) and same_bits(b["db"], a["db"]), f"dgamma / dbeta ({what})"
                        assert_close(b["dg"], dg_ref, f"dgamma ({what})", rel=1e-3, elem=2e-3)
                        assert_close(b["db"], db_ref, f"dbeta ({what})", rel=1e-3, elem=2e-3)


def test_fused_launch_refusals():
    """Shapes outside the kernel's limits and null pointers are refused with a status and a message, and nothing is launched."""
    lib, lb = L()

    def call(B, N, M, heads, d, drop=None, batch=None):
        C_ = heads * d
        a = dict(dx1=nans(B, N, C_), u=nans(B, C_), S=nans(B, N), q=torch.zeros(B, N, C_, dtype=BF16, device="cuda"),
                 k=torch.zeros(B, M, C_, dtype=BF16, device="cuda"), idx=torch.zeros(B, N, heads, dtype=torch.int16, device="cuda"),
                 t=zsum(B, C_), dbp=zsum(B, C_), dq=nans(B, N, C_, dtype=BF16), parts=nans(1, B, M, C_))
        if drop:
            a[drop] = None
        rc = lb.crd_attn_bwd_fused(P(a["dx1"]), P(a["u"]), P(a["S"]), None, P(a["q"]), P(a["k"]), P(a["idx"]), B if batch is None else batch,
                                   N, M, heads, d, 0.1,
                                   P(a["t"]), P(a["dbp"]), None, P(a["dq"]), P(a["parts"]), None, None, None, None, None, None, None,
                                   lib.stream())
        return rc, a

    def untouched(a):
        return all(bool(torch.isnan(a[k].float()).all()) for k in ("dx1", "dq", "parts") if a[k] is not None) and not bool(a["t"].any())

    assert lb.crd_attn_scores_bwd_partials(1, 200, 4200, 8, 8) == 0
    rc, a = call(1, 200, 4200, 8, 8)                    # parts == 0: the masks do not fit in LDS
    refused(rc, "crd_attn_bwd_fused", "LDS")
    assert untouched(a)
    assert lb.crd_attn_scores_bwd_partials(1, 550, 1000, 8, 64) == 9 and lb.crd_attn_bwd_fused_supported(1, 550, 1000, 8, 64) == 0
    rc, a = call(1, 550, 1000, 8, 64)                   # the score backward's chunk fits in 128 KB, with the 2 * C channel sums it does not
    refused(rc, "crd_attn_bwd_fused", "LDS")
    assert untouched(a)
    rc, a = call(1, 8, 4, 1, 8, batch=0)
    refused(rc, "crd_attn_bwd_fused", "positive")
    assert untouched(a)
    rc, a = call(1, 8, 4, 5, 104)                       # C = 520
    refused(rc, "crd_attn_bwd_fused", "520", "512")
    assert untouched(a)
    for drop in ("dq", "parts", "idx", "t"):
        rc, a = call(1, 8, 4, 1, 8, drop=drop)
        refused(rc, "crd_attn_bwd_fused", "null pointer")
        if drop != "t":
            assert untouched(a)
    some, wd = nans(8), torch.zeros(8, 16, dtype=BF16, device="cuda")
    dst, tb, es = nans(8, dtype=BF16), nans(8, dtype=BF16), nans(8)
    refused(lb.crd_attn_dk_fold(P(some), 1, 8, P(dst), 8, None, P(wd), 1, 8, 16, 1.0, P(tb), P(es), lib.stream()), "crd_attn_dk_fold", "null pointer")
    refused(lb.crd_attn_dk_fold(P(some), 0, 8, P(dst), 8, P(zsum(8)), P(wd), 1, 8, 16, 1.0, P(tb), P(es), lib.stream()), "crd_attn_dk_fold", "bad argument")
    assert bool(torch.isnan(dst.float()).all()) and bool(torch.isnan(tb.float()).all()) and bool(torch.isnan(es).all())


# replicas = 1, and a count that is no multiple of the four copies a pass of the fold loads
@pytest.mark.parametrize("shape", [(1, 1, 4, 1, 8), (2, 600, 104, 2, 32)], ids=lambda s: "x".join(map(str, s)))
def test_fold_entry_equals_the_fold_and_the_vector_path(shape):
    lib, lb = L()
    B, N, M, heads, d = shape
    parts_n = CASES[shape][0]
    assert parts_n == 1 or parts_n % 4
    p = attention_problem(shape, seed=22)
    C_, scale, n = p["C"], p["scale"], B * M * p["C"]
    g = torch.Generator().manual_seed(23)
    dS = torch.randn(B, N, generator=g).cuda()
    t = to_grad(torch.randn(B, C_, generator=g)).cuda()
    wd = torch.zeros(C_, C_ + 8, dtype=BF16, device="cuda")
    wd[:, :C_] = (0.2 * torch.randn(C_, C_, generator=g)).to(BF16)
    inv_n = f32(1.0 / N)
    # crd_attn_bwd: the partial copies and the vector outputs for this t; crd_sum_partials_bf16 folds the copies
    parts, dq, tb0, es0 = nans(parts_n, B, M, C_), nans(B, N, C_, dtype=BF16), nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_bwd(P(p["q"]), P(p["k"]), P(dS), P(p["idx"]), B, N, M, heads, d, scale, P(dq), None, P(parts), P(t), P(wd), C_ + 8,
                       inv_n, P(tb0), P(es0), lib.stream()), "attn_bwd")
    dst0 = nans(n + 8, dtype=BF16)
    ok(lb.crd_sum_partials_bf16(P(parts), parts_n, n, P(dst0), n, lib.stream()), "sum_partials")
    dst1, tb1, es1 = nans(n + 8, dtype=BF16), nans(B, C_, dtype=BF16), nans(B, C_)
    ok(lb.crd_attn_dk_fold(P(parts), parts_n, n, P(dst1), n, P(t), P(wd), B, C_, C_ + 8, inv_n, P(tb1), P(es1), lib.stream()), "attn_dk_fold")
    assert bool(torch.isfinite(dst0[:n].float()).all()) and bool(torch.isfinite(es0).all())
    assert same_bits(dst1[:n], dst0[:n]), "dst: the fold of the copies"
    assert bool(torch.isnan(dst1[n:].float()).all()), "wrote past n"
    assert same_bits(tb1, tb0) and same_bits(es1, es0), "tb / es: the vector path"


def test_train_step_with_and_without_the_fused_launches(monkeypatch):
    """One small full train step (depths 1-1-1-1, 2 x 64 x 96, eager: two runs of one plan give the same bits) with ATTN_BWD_FUSED forced
    to 0 and to 15.  The loss is equal (the forward is the same launches).  The q / k / sr gradients are the same bits: their dq and dK
    inputs are.  Every parameter gradient is within rel-L2 2e-2, the tighter of the two bounds tests/test_gpu_train.py puts on the gradient
    of a graph step against an eager one (2e-2 and 3e-2).  What really differs is far smaller, and is bounded from the number formats: the
    two plans differ in the last fp32 bits of t and dbp_rows only (bounded at 1e-5 by the op test above, and so is proj's bias gradient,
    their sum over the samples); everything behind them is stored in bf16 (Tb, the data gradients) or is a sum of such values, so an
    element moves by at most one bf16 rounding step, 2^-8 of its value, where a rounding flips, and proj's weight gradient (Tb x xbar)
    and the whole gradient vector stay within rel-L2 2^-8."""
    from camradepth_amd import plan_values, synth
    from camradepth_amd.config import ModelConfig
    from camradepth_amd.params import param_specs
    from camradepth_amd.trainer import TrainStep
    from tests.test_gpu_train import build, fix_masks, rel
    cfg = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    masks = synth.make_masks(cfg, 2, seed=99)
    batch = {k: v.cuda() for k, v in synth.make_batch(2, 64, 96, seed=70).items()}
    runs = {}
    for mask in (0, 15):
        monkeypatch.setattr(plan_values, "ATTN_BWD_FUSED", mask)
        m = build(cfg, sd)
        ts = TrainStep(m, 2, 64, 96, lr=1e-3, use_graph=False)
        names = [op.name for op in ts.plan.bwd]
        assert (names.count("crd_attn_bwd_fused"), names.count("crd_attn_dk_fold")) == ((4, 4) if mask else (0, 0))
        assert names.count("crd_attn_bwd") == (0 if mask else 4)
        fix_masks(ts, masks)
        ts.set_batch(batch)
        ts.step()
        torch.cuda.synchronize()
        runs[mask] = (ts.losses(), {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None}, m.flat_grad.clone())
    (l0, g0, f0), (l1, g1, f1) = runs[0], runs[15]
    assert l0 == l1, (l0, l1)
    assert g0.keys() == g1.keys()
    exact = 0
    worst = max((rel(g1[n], g0[n]), n) for n in g0)
    print(f"mask 15 against mask 0: whole gradient rel-L2 {rel(f1, f0):.3e}, worst parameter {worst[1]} {worst[0]:.3e}")
    assert rel(f1, f0) < 2.0 ** -8, rel(f1, f0)
    for n in g0:
        assert rel(g1[n], g0[n]) < 2e-2, (n, rel(g1[n], g0[n]))
        if ".attn.proj.bias" in n:
            assert rel(g1[n], g0[n]) < 1e-5, (n, rel(g1[n], g0[n]))
        if ".attn.proj.weight" in n:
            assert rel(g1[n], g0[n]) < 2.0 ** -8, (n, rel(g1[n], g0[n]))
        if any(s in n for s in (".attn.q.", ".attn.k.", ".attn.sr.")):
            assert torch.equal(g1[n], g0[n]), f"{n}: dq / dK are the same bits, so is this gradient"
            exact += 1
    assert exact >= 4 * 4 + 3 * 2          # q and k (weight, bias) of four Blocks, sr of the three stages that have one
    assert float(sum(v.abs().sum() for v in g1.values())) > 0
