"""GPU tests of max_grad_norm: torch.nn.utils.clip_grad_norm_(params, c) fused into the diffGradNorm step of TrainStep,
runner.Trainer and diffGradNorm.  Monitoring (c = inf) gives the bits of the default step, clipping matches an eager loop with
torch's clip_grad_norm_, and the total is reproducible.  Tiny config (depths 1,1,1,1), 2 x 64 x 96, synth batches, fixed dropout
masks (as tests/test_gpu_skip_nonfinite.py)."""
import dataclasses
import math

import pytest
import torch

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.params import param_specs

pytestmark = pytest.mark.gpu

CFG = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1))
SCHED = [(1e-3 * (1 + 0.1 * i), 0.9 - 0.01 * i) for i in range(16)]        # distinct (lr, beta1) per scheduler step
LR, BETAS = 1e-3, (0.9, 0.999)
# exact in fp32: the eager optimizer takes lr / betas as floats, TrainStep forms its bias corrections from the Python doubles (with
# beta2 = 0.999 the two step sizes differ by 6e-6 relative, with or without clipping)
LR_X, BETAS_X = 2.0 ** -10, (0.875, 1.0 - 2.0 ** -10)
FROZEN = "from_encoder_3."


def build(sd, frozen=False):
    from camradepth_amd.model import CamRaDepth
    m = CamRaDepth(input_channels=CFG.input_channels, depths=CFG.depths)
    m.load_state_dict(sd)
    m = m.cuda().train()
    if frozen:
        names = [n for n, p in m.named_parameters() if n.startswith(FROZEN)]
        assert names
        for n, p in m.named_parameters():
            if n.startswith(FROZEN):
                p.requires_grad_(False)
    return m


def fix_masks(ts, masks):
    ts.plan.training_masks_fixed = True
    ts.plan.dp_masks.copy_(torch.stack([t.cuda() for t in masks["drop_path"]]))
    ts.plan.d2_masks.copy_(torch.stack([t.cuda() for t in masks["dropout2d"]]))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def setup():
    sd = synth.fill_state_dict({n: s for n, s in param_specs(CFG)}, 0)
    masks = synth.make_masks(CFG, 2, seed=4321)
    batches = [synth.make_batch(2, 64, 96, seed=50 + i) for i in range(8)]
    return sd, masks, batches


def make_step(sd, masks, use_graph, k=1, frozen=False, **kw):
    from camradepth_amd.trainer import TrainStep
    m = build(sd, frozen)
    ts = TrainStep(m, 2, 64, 96, update_interval=k, use_graph=use_graph, **kw)
    fix_masks(ts, masks)
    return m, ts


def snap(m, ts):
    torch.cuda.synchronize()
    return [t.clone() for t in (m.flat, ts.m, ts.v, ts.pg, ts.egn)]


def run(ts, b):
    ts.set_batch({k: v.cuda() for k, v in b.items()})
    r = ts.step()
    torch.cuda.synchronize()
    return r


def window_norm(m, ts):
    """fp64 ||g|| of the window's (unclipped, accumulated) gradients over the trainable tensors."""
    g = m.flat_grad.double()
    s = 0.0
    for name, (a, b) in zip(m._names, ts.state.seg_host):
        if m._param(name).requires_grad:
            s += float((g[a:b] ** 2).sum())
    return math.sqrt(s)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_monitoring_is_bit_identical_to_default(setup, use_graph, k, wd):
    sd, masks, batches = setup
    out = []
    for mgn in (None, float("inf")):
        m, ts = make_step(sd, masks, use_graph, k, schedule=SCHED, weight_decay=wd, max_grad_norm=mgn)
        assert (ts.grad_norm is None) == (mgn is None)
        for i in range(4 * k):
            run(ts, batches[i % len(batches)])
            if mgn is not None and (i + 1) % k == 0:           # a window closed: the norm of ITS gradients
                gn = ts.grad_norm
                assert gn.dtype == torch.float32 and gn.dim() == 0 and gn.is_cuda
                ref = window_norm(m, ts)
                assert abs(float(gn) - ref) <= 1e-6 * ref, (i, float(gn), ref)
        out.append(snap(m, ts))
    for name, a, b in zip(("flat", "m", "v", "pg", "egn"), *out):
        assert torch.equal(a, b), (name, use_graph, k, wd, rel(b, a))


def _eager_run(sd, masks, batches, c, wd, frozen):
    """The usual PyTorch loop: backward -> torch.nn.utils.clip_grad_norm_ -> diffGradNorm.step (unclipped)."""
    from camradepth_amd import losses as hl
    from camradepth_amd.optim import diffGradNorm
    m = build(sd, frozen)
    opt = diffGradNorm(m.parameters(), lr=LR, betas=BETAS, weight_decay=wd)
    norms = []
    for b in batches:
        opt.zero_grad()
        out = m(b["image"].cuda(), masks=masks)
        loss, _ = hl.total_loss(out, {k: v.cuda() for k, v in b.items()}, False)
        loss.backward()
        norms.append(torch.nn.utils.clip_grad_norm_(m.parameters(), c if c is not None else float("inf")))
        opt.step()
    torch.cuda.synchronize()
    return m.flat.clone(), [float(n) for n in norms]


def _fused_run(sd, masks, batches, c, wd, frozen, use_graph):
    m, ts = make_step(sd, masks, use_graph, 1, frozen, lr=LR, betas=BETAS, weight_decay=wd,
                      max_grad_norm=c if c is not None else float("inf"))
    norms = []
    for b in batches:
        run(ts, b)
        norms.append(float(ts.grad_norm))
    return m.flat.clone(), norms


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("frozen", [False, True])
def test_clipped_step_follows_the_eager_clip_grad_norm_loop(setup, use_graph, wd, frozen):
    """TrainStep(max_grad_norm=c) against the eager loop with torch's clip_grad_norm_ over 4 steps.  The eager module path and the
    captured step do not give the same bits even WITHOUT clipping (other kernel paths; diffGradNorm's sign-like steps spread the
    difference: rel-L2 2.5e-2 - 6.4e-2 of the 4-step deltas, measured), so the bound is that unclipped control; the first step
    starts from the same parameters, and its norm is torch's.  The exact check is the per-step test below."""
    sd, masks, batches = setup
    steps = batches[:4]
    p0 = build(sd).flat.detach().clone()
    pe, ne = _eager_run(sd, masks, steps, None, wd, frozen)
    pf, nf = _fused_run(sd, masks, steps, None, wd, frozen, use_graph)
    control = rel(pf - p0, pe - p0)
    c = 0.1 * min(ne)                                           # clipping active on every step
    pe, ne = _eager_run(sd, masks, steps, c, wd, frozen)
    pf, nf = _fused_run(sd, masks, steps, c, wd, frozen, use_graph)
    r = rel(pf - p0, pe - p0)
    print(f"4 clipped steps vs the eager loop: rel-L2 of the deltas {r:.3e} (unclipped control {control:.3e}); norms {nf} / {ne}")
    assert all(n > c for n in ne) and all(n > c for n in nf), (c, ne, nf)
    assert abs(nf[0] - ne[0]) <= 1e-6 * ne[0], (nf, ne)
    assert all(abs(a - b) <= 1e-2 * b for a, b in zip(nf, ne)), (nf, ne)
    assert r <= 2 * control, (r, control)                       # measured: r = 0.04 - 0.92 x control
    if frozen:
        m = build(sd, True)
        for n in m._names:
            if n.startswith(FROZEN):
                o, k = m._offsets[m._index[n]], m._param(n).numel()
                assert torch.equal(pf[o:o + k], p0[o:o + k]) and torch.equal(pe[o:o + k], p0[o:o + k]), n


def _torch_clip_then_step(m, ts, before, c, wd, step):
    """One step of torch.nn.utils.clip_grad_norm_ + the unclipped diffGradNorm on the window's gradients (the fused step leaves
    them unclipped in flat_grad), from the state `before` (flat, m, v, pg, egn) -> (new flat values per tensor, torch's norm)."""
    from camradepth_amd.optim import diffGradNorm
    flat, ea, eas, pg, egn = before
    ps, state = [], {}
    for t, (name, (a, b)) in enumerate(zip(m._names, ts.state.seg_host)):
        shape = m._param(name).shape
        p = flat[a:b].clone().view(shape).requires_grad_(True)
        p.grad = m.flat_grad[a:b].clone().view(shape) if m._param(name).requires_grad else None
        ps.append(p)
        state[t] = {"step": step - 1, "exp_avg": ea[a:b].view(shape), "exp_avg_sq": eas[a:b].view(shape),
                    "previous_grad": pg[a:b].view(shape), "exp_grad_norm": egn[t].clone()}
    norm = torch.nn.utils.clip_grad_norm_(ps, c)
    opt = diffGradNorm(ps, lr=LR_X, betas=BETAS_X, weight_decay=wd)
    sd = opt.state_dict()
    sd["state"] = state
    opt.load_state_dict(sd)
    opt.step()
    torch.cuda.synchronize()
    return [p.detach().reshape(-1) for p in ps], float(norm)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("frozen", [False, True])
def test_each_clipped_step_is_clip_grad_norm_then_diffgradnorm(setup, use_graph, wd, frozen):
    """Step by step, on the fused step's own gradients: torch's clip_grad_norm_ followed by the existing unclipped diffGradNorm
    gives the same parameters and the same norm.  Only the clipping arithmetic differs: the fp64 total (torch's coefficient can be
    one ulp off ours) and c^2 sum g^2 for the per-tensor norm, which moves diffGradNorm's factor e / n by about 1e-7 relative where
    e > n (measured rel-L2 of the deltas: 0 with wd = 1e-2, up to 4.3e-7 with wd = 0, where a few elements per million differ by
    more than an ulp because exp_avg nearly cancels)."""
    sd, masks, batches = setup
    m, ts = make_step(sd, masks, use_graph, 1, frozen, lr=LR_X, betas=BETAS_X, weight_decay=wd, max_grad_norm=0.05)
    worst = 0.0
    for i, b in enumerate(batches[:4]):
        before = snap(m, ts)
        run(ts, b)
        ref, norm = _torch_clip_then_step(m, ts, before, 0.05, wd, i + 1)
        gn = float(ts.grad_norm)
        assert gn > 0.05 and abs(gn - norm) <= 1e-6 * norm, (i, gn, norm)
        new = torch.cat([m.flat[a:b] for a, b in ts.state.seg_host])
        new_ref = torch.cat(ref)
        old = torch.cat([before[0][a:b] for a, b in ts.state.seg_host])
        worst = max(worst, rel(new - old, new_ref - old))
    print(f"per-step clipped update vs clip_grad_norm_ + diffGradNorm: rel-L2 {worst:.3e}")
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_standalone_optimizer_matches_torch(wd):
    """Loose tensors (not one flat buffer): sizes below, at and across the 4096-element chunk, one without a gradient."""
    from camradepth_amd.optim import diffGradNorm
    gen = torch.Generator().manual_seed(5)
    shapes = [(17,), (4096,), (4097,), (3, 5000), (64, 64, 3), (9,)]
    params0 = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) * (1 + i) for i, s in enumerate(shapes)] for _ in range(3)]

    def run_opt(clip):
        ps = [p.clone().cuda().requires_grad_(True) for p in params0]
        opt = diffGradNorm(ps, lr=1e-2, weight_decay=wd, max_grad_norm=clip)
        norms = []
        for gs in grads:
            for i, (p, g) in enumerate(zip(ps, gs)):
                p.grad = None if i == 4 else g.clone().cuda()
            if clip is None:
                norms.append(float(torch.nn.utils.clip_grad_norm_(ps, c)))
            opt.step()
            if clip is not None:
                norms.append(float(opt.grad_norm))
                assert torch.equal(ps[0].grad.cpu(), gs[0])      # the fused path scales on the fly: .grad is not written
        torch.cuda.synchronize()
        return [p.detach().cpu() for p in ps], norms, opt
    c = 0.05 * math.sqrt(sum(float((g ** 2).sum()) for i, g in enumerate(grads[0]) if i != 4))
    ref, nref, _ = run_opt(None)
    got, ngot, opt = run_opt(c)
    for a, b in zip(ngot, nref):
        assert abs(a - b) <= 1e-6 * b, (ngot, nref)
    for i, (a, b, p0) in enumerate(zip(got, ref, params0)):
        if i == 4:
            assert torch.equal(a, p0) and torch.equal(b, p0)
        else:
            assert rel(a - p0, b - p0) <= 1e-5, (i, rel(a - p0, b - p0))
    # the optimizer state keeps the reference's keys only
    assert set(opt.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay"}


def test_skip_nonfinite_with_clipping_skips_and_matches_a_run_without_the_batch(setup):
    sd, masks, batches = setup
    bad = {k: v.clone() for k, v in batches[1].items()}
    bad["image"][0, 0, 10, 20] = float("nan")
    c = 0.05
    m1, ts1 = make_step(sd, masks, True, lr=LR, betas=BETAS, skip_nonfinite=True, max_grad_norm=c)
    run(ts1, batches[0])
    g0 = float(ts1.grad_norm)
    assert g0 > c
    run(ts1, bad)
    assert ts1.found_inf and not math.isfinite(float(ts1.grad_norm))
    run(ts1, batches[2])
    run(ts1, batches[3])
    assert ts1.skipped_steps == 1 and ts1.committed_steps == 3
    m2, ts2 = make_step(sd, masks, True, lr=LR, betas=BETAS, max_grad_norm=c)
    for b in (batches[0], batches[2], batches[3]):
        run(ts2, b)
    for name, a, b in zip(("flat", "m", "v", "pg", "egn"), snap(m1, ts1), snap(m2, ts2)):
        assert torch.equal(a, b), (name, rel(a, b))
    assert torch.equal(ts1.grad_norm, ts2.grad_norm)


@pytest.mark.parametrize("use_graph", [False, True])
def test_clipped_runs_are_bit_reproducible(setup, use_graph):
    sd, masks, batches = setup
    out = []
    for _ in range(2):
        m, ts = make_step(sd, masks, use_graph, 3, schedule=SCHED, weight_decay=1e-2, max_grad_norm=0.05)
        norms = []
        for i in range(9):
            run(ts, batches[i % len(batches)])
            norms.append(ts.grad_norm)
        out.append(snap(m, ts) + [torch.stack(norms)])
    for name, a, b in zip(("flat", "m", "v", "pg", "egn", "grad_norm"), *out):
        assert torch.equal(a, b), name


def test_refusals_before_any_launch(setup):
    from camradepth_amd import lib as L
    from camradepth_amd.optim import diffGradNorm
    from camradepth_amd.trainer import TrainStep
    sd, _, _ = setup
    m = build(sd)
    flat0 = m.flat.clone()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(L.CrdError, match="max_grad_norm"):
            TrainStep(m, 2, 64, 96, max_grad_norm=bad)
        with pytest.raises(L.CrdError, match="max_grad_norm"):
            diffGradNorm(m.parameters(), max_grad_norm=bad)
    ps = list(m.parameters())
    with pytest.raises(L.CrdError, match="one param group"):
        diffGradNorm([{"params": ps[:3]}, {"params": ps[3:]}], max_grad_norm=1.0)
    opt = diffGradNorm(ps[:3], lr=1e-3, max_grad_norm=1.0)
    opt.add_param_group({"params": ps[3:]})
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(L.CrdError, match="one param group"):
        opt.step()
    torch.cuda.synchronize()
    assert opt._groups is None and opt.grad_norm is None and torch.equal(m.flat, flat0)


def test_runner_trains_an_epoch_through_the_clipped_step():
    from camradepth_amd.model import CamRaDepth
    from camradepth_amd.runner import Trainer
    sd = synth.fill_state_dict({n: s for n, s in param_specs(CFG)}, 0)
    train = [synth.make_batch(2, 64, 96, seed=10 + i) for i in range(4)] + [synth.make_batch(1, 64, 96, seed=14)]
    res = {}
    for mgn in (None, 0.05):
        m = CamRaDepth(input_channels=7, depths=CFG.depths)
        m.load_state_dict(sd)
        m = m.cuda().train()
        tr = Trainer(m, train, None, None, learning_rate=1e-3, num_epochs=1, update_interval=2, max_grad_norm=mgn)
        p0 = m.flat.clone()
        r = tr.train_one_epoch(0)
        torch.cuda.synchronize()
        assert tr.training_steps == 3 and all(math.isfinite(v) for v in r.values())
        assert not torch.equal(m.flat, p0)
        res[mgn] = (m.flat - p0, tr)
    d, tr = res[0.05]
    assert len(tr._steps) == 2                                 # the ragged last batch: a second TrainStep on the same TrainState
    for ts in tr._steps.values():
        assert ts.max_grad_norm == 0.05 and ts.state is tr._train_state
    assert float(tr.step.grad_norm) > 0.05                    # the flush window was clipped
    assert not torch.equal(d, res[None][0])
