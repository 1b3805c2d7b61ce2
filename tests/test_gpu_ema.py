"""GPU tests of ema_decay: the exponential moving average of the weights kept by diffGradNorm's update kernel, in TrainStep,
runner.Trainer, the eager optimizer and the checkpoint, and the in-place weight swap.  Tiny config (depths 1,1,1,1), 2 x 64 x 96,
synth batches, fixed dropout masks (as tests/test_gpu_clip_grad_norm.py).

The oracle is the recurrence itself in fp64 on the host side: after every committed step n the parameters are read back bit-exactly
and e <- e + w_n (p - e) with the SAME fp32 w_n (optim.ema_weight).  Tolerance (derived, not measured): one device update is two
fp32 roundings, p - e and the fma, each at most u M-sized with u = 2^-24 and M = max(|p|, |e|) over the tensor (3 u M with the
fp64 oracle's own product); older error shrinks by d_n = 1 - w_n.  So after N updates |e_dev - e_fp64| <= 3 u M min(N, 1 / min w_n)
per element (tests/test_ema_cpu.py runs the numbers: the worst emulated error is 0.12 of it).  Every recurrence check also asserts
that the oracle moved by more than 100 bounds, so a missing update cannot pass."""
import dataclasses
import math

import pytest
import torch

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.params import param_specs

pytestmark = pytest.mark.gpu

CFG = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1))
SCHED = [(1e-3 * (1 + 0.1 * i), 0.9 - 0.01 * i) for i in range(16)]
LR, BETAS = 1e-3, (0.9, 0.999)
FROZEN = "from_encoder_3."
U = 2.0 ** -24


def build(sd, frozen=False):
    from camradepth_amd.model import CamRaDepth
    m = CamRaDepth(input_channels=CFG.input_channels, depths=CFG.depths)
    m.load_state_dict(sd)
    m = m.cuda().train()
    if frozen:
        assert [n for n, p in m.named_parameters() if n.startswith(FROZEN)]
        for n, p in m.named_parameters():
            if n.startswith(FROZEN):
                p.requires_grad_(False)
    return m


def fix_masks(ts, masks):
    ts.plan.training_masks_fixed = True
    ts.plan.dp_masks.copy_(torch.stack([t.cuda() for t in masks["drop_path"]]))
    ts.plan.d2_masks.copy_(torch.stack([t.cuda() for t in masks["dropout2d"]]))


@pytest.fixture(scope="module")
def setup():
    sd = synth.fill_state_dict({n: s for n, s in param_specs(CFG)}, 0)
    masks = synth.make_masks(CFG, 2, seed=4321)
    batches = [synth.make_batch(2, 64, 96, seed=50 + i) for i in range(8)]
    return sd, masks, batches


def make_step(sd, masks, use_graph=True, k=1, frozen=False, hw=(64, 96), **kw):
    from camradepth_amd.trainer import TrainStep
    m = build(sd, frozen)
    ts = TrainStep(m, 2, hw[0], hw[1], update_interval=k, use_graph=use_graph, **kw)
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


def poisoned(b):
    bad = {k: v.clone() for k, v in b.items()}
    bad["image"][0, 0, 10, 20] = float("nan")
    return bad


class Oracle:
    """The fp64 recurrence over flat buffers: segs = [(begin, end, trainable)] per tensor."""

    def __init__(self, ema0, segs, decay, warmup):
        from camradepth_amd.optim import ema_weight
        self.weight = lambda n: ema_weight(decay, warmup, n)[1]
        self.e = ema0.detach().double().clone()
        self.e0 = self.e.clone()
        self.segs, self.ws = segs, []
        n = self.e.numel()
        self.tid = torch.full((n,), len(segs), dtype=torch.int64, device=self.e.device)      # element -> tensor (gaps: one more id)
        self.train = torch.zeros(n, dtype=torch.bool, device=self.e.device)
        for t, (a, b, tr) in enumerate(segs):
            self.tid[a:b] = t
            self.train[a:b] = bool(tr)
        self.M = torch.zeros(len(segs) + 1, dtype=torch.float64, device=self.e.device)

    def update(self, p):
        """p: the parameters right after committed step n = len(ws) + 1."""
        w = self.weight(len(self.ws) + 1)
        self.ws.append(w)
        p = p.detach().double()
        self.e = torch.where(self.train, self.e + w * (p - self.e), self.e)
        self.M.scatter_reduce_(0, self.tid, torch.maximum(p.abs(), self.e.abs()), "amax")

    def bound(self):
        """per tensor: 3 u M min(N, 1 / min w_n)"""
        return 3 * U * self.M * min(len(self.ws), 1.0 / min(self.ws))

    def check(self, ema, p, what=""):
        torch.cuda.synchronize()
        err = (ema.detach().double() - self.e).abs()
        worst = torch.zeros_like(self.M).scatter_reduce_(0, self.tid, err, "amax")
        bound = self.bound()
        ok = worst[:-1] <= bound[:-1]
        assert bool(ok.all()), (what, len(self.ws), [(t, float(worst[t]), float(bound[t])) for t in torch.nonzero(~ok).flatten().tolist()[:5]])
        for a, b, tr in self.segs:                       # frozen tensors: the EMA never left the parameter
            if not tr:
                assert torch.equal(ema[a:b], p[a:b]) and torch.equal(ema[a:b].double(), self.e0[a:b]), (what, a, b)
        return float((worst[:-1] / bound[:-1].clamp_min(1e-300)).max())

    def assert_moved(self):
        """A missing (or a single dropped) update cannot pass: the oracle itself moved by more than 100 bounds."""
        moved = float((self.e - self.e0).abs().max())
        assert moved > 100 * float(self.bound()[:-1].max()), (moved, float(self.bound()[:-1].max()))


def oracle_for(m, ts):
    segs = [(a, b, m._param(n).requires_grad) for n, (a, b) in zip(m._names, ts.state.seg_host)]
    return Oracle(ts.ema, segs, ts.ema_decay, ts.ema_warmup)


def follow(m, ts, batches, iters, what=""):
    """Runs `iters` iterations; the EMA obeys the recurrence after every optimizer step and keeps its bits on the others."""
    orc = oracle_for(m, ts)
    assert torch.equal(ts.ema, m.flat) and ts.ema_updates == 0
    worst = 0.0
    for i in range(iters):
        before = ts.ema.clone()
        if run(ts, batches[i % len(batches)]):
            orc.update(m.flat)
            worst = max(worst, orc.check(ts.ema, m.flat, what))
            assert not torch.equal(ts.ema, before)
        else:
            assert torch.equal(ts.ema, before), (what, i)
        assert ts.ema_updates == len(orc.ws)
    orc.assert_moved()
    print(f"{what}: {len(orc.ws)} EMA updates, worst error {worst:.3f} of the bound")
    return orc


# ---------------------------------------------------------------------------------------------- 1. the recurrence
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("wd,frozen,warmup", [(0.0, False, False), (1e-2, True, False), (1e-2, False, True), (0.0, True, True)])
def test_ema_follows_the_recurrence(setup, use_graph, k, wd, frozen, warmup):
    sd, masks, batches = setup
    m, ts = make_step(sd, masks, use_graph, k, frozen, schedule=SCHED, weight_decay=wd, ema_decay=0.9, ema_warmup=warmup)
    follow(m, ts, batches, 12 * k, f"graph={use_graph} k={k} wd={wd} frozen={frozen} warmup={warmup}")
    sdict = ts.ema_state_dict()
    assert list(sdict) == list(m.state_dict()) and all(sdict[n].shape == v.shape for n, v in m.state_dict().items())
    assert sdict[m._names[0]].data_ptr() == ts.ema.data_ptr()                 # views, not copies


# ---------------------------------------------------------------------------------------------- 2. training keeps its bits
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kw", [{}, {"skip_nonfinite": True}, {"max_grad_norm": 0.05}], ids=["default", "skip", "clip"])
def test_training_is_not_perturbed(setup, use_graph, kw):
    sd, masks, batches = setup
    out = []
    for ema in (None, 0.9):
        m, ts = make_step(sd, masks, use_graph, 2, schedule=SCHED, weight_decay=1e-2, ema_decay=ema, **kw)
        losses = []
        for i in range(8):
            run(ts, batches[i])
            losses.append(ts.losses())
        out.append((snap(m, ts), losses))
    for name, a, b in zip(("flat", "m", "v", "pg", "egn"), out[0][0], out[1][0]):
        assert torch.equal(a, b), (name, use_graph, kw)
    assert out[0][1] == out[1][1]


# ---------------------------------------------------------------------------------------------- 3. skip_nonfinite
def test_a_skipped_window_leaves_the_ema_alone(setup):
    sd, masks, batches = setup
    m1, ts1 = make_step(sd, masks, True, lr=LR, betas=BETAS, skip_nonfinite=True, ema_decay=0.9)
    run(ts1, batches[0])
    e1, n1 = ts1.ema.clone(), ts1.ema_updates
    assert n1 == 1 and not torch.equal(e1, m1.flat)
    run(ts1, poisoned(batches[1]))
    assert ts1.found_inf and torch.equal(ts1.ema, e1) and ts1.ema_updates == 1
    run(ts1, batches[2])
    run(ts1, batches[3])
    assert ts1.skipped_steps == 1 and ts1.committed_steps == 3 and ts1.ema_updates == 3
    m2, ts2 = make_step(sd, masks, True, lr=LR, betas=BETAS, skip_nonfinite=True, ema_decay=0.9)
    for b in (batches[0], batches[2], batches[3]):
        run(ts2, b)
    for name, a, b in zip(("flat", "m", "v", "pg", "egn"), snap(m1, ts1), snap(m2, ts2)):
        assert torch.equal(a, b), name
    assert torch.equal(ts1.ema, ts2.ema) and ts2.ema_updates == 3


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("warmup", [True, False])
def test_device_and_host_weights_agree(setup, use_graph, warmup):
    """Finite data: the gated commit forms w_n on the device from its own count, the ungated one reads the host's -- the same bits.
    Decay 0.9999 with the warm-up walks (1 + n) / (10 + n), a division per step."""
    sd, masks, batches = setup
    emas = []
    for skip in (False, True):
        m, ts = make_step(sd, masks, use_graph, 1, schedule=SCHED, skip_nonfinite=skip, ema_decay=0.9999 if warmup else 0.9,
                          ema_warmup=warmup)
        for i in range(8):
            run(ts, batches[i])
        assert ts.ema_updates == 8 and not torch.equal(ts.ema, m.flat)
        emas.append((ts.ema.clone(), m.flat.clone()))
    assert torch.equal(emas[0][1], emas[1][1]) and torch.equal(emas[0][0], emas[1][0])


# ---------------------------------------------------------------------------------------------- 4. with max_grad_norm
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("mgn,skip", [(0.05, False), (float("inf"), False), (0.05, True)], ids=["clip", "monitor", "clip+skip"])
def test_recurrence_with_max_grad_norm(setup, use_graph, mgn, skip):
    sd, masks, batches = setup
    m, ts = make_step(sd, masks, use_graph, 1, True, schedule=SCHED, weight_decay=1e-2, max_grad_norm=mgn, skip_nonfinite=skip,
                      ema_decay=0.9, ema_warmup=False)
    follow(m, ts, batches, 12, f"graph={use_graph} max_grad_norm={mgn} skip_nonfinite={skip}")


# ---------------------------------------------------------------------------------------------- 5. the weight swap
@pytest.mark.parametrize("n,oa,ob", [(0, 0, 0), (1, 0, 0), (3, 1, 1), (4, 0, 0), (4097, 0, 0), (4097, 3, 3), (4097, 1, 2), (3 * 2 ** 20 + 5, 2, 2),
                                     (3 * 2 ** 20 + 5, 0, 3)])
def test_swap_is_exact(n, oa, ob):
    from camradepth_amd import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(n + oa)
    A, B = torch.randn(n + 16, generator=g).cuda(), torch.randn(n + 16, generator=g).cuda()
    A0, B0 = A.clone(), B.clone()
    a, b = A[oa:oa + n], B[ob:ob + n]
    L.check(lib.crd_swap_f32(a.data_ptr() if n else None, b.data_ptr() if n else None, n, L.stream()), "crd_swap_f32")
    torch.cuda.synchronize()
    assert torch.equal(a, B0[ob:ob + n]) and torch.equal(b, A0[oa:oa + n])
    assert torch.equal(A[:oa], A0[:oa]) and torch.equal(A[oa + n:], A0[oa + n:])           # nothing outside the range
    assert torch.equal(B[:ob], B0[:ob]) and torch.equal(B[ob + n:], B0[ob + n:])
    if n >= 2:
        assert lib.crd_swap_f32(a.data_ptr(), a.data_ptr() + 4, n, L.stream()) != 0          # overlapping buffers are refused
        assert lib.crd_swap_f32(a.data_ptr() + 2, b.data_ptr(), n - 1, L.stream()) != 0      # ... and misaligned floats


@pytest.mark.parametrize("fp8", [False, True])
def test_ema_weights_context(setup, fp8):
    from camradepth_amd import lib as L
    from camradepth_amd.inference import InferenceGraph
    sd, masks, batches = setup
    hw = (64, 96)
    if fp8:                                               # the e4m3 route of the largest decoder stage needs >= 192 tiles of 16 x 32
        hw = (128, 384)
        batches = [synth.make_batch(2, hw[0], hw[1], seed=70 + i) for i in range(6)]
    x = batches[5]["image"].cuda()
    scales = None

    def prepare(model):
        if fp8:
            model.__dict__["fp8_scales"] = scales
        return model
    m, ts = make_step(sd, masks, True, hw=hw, lr=LR, betas=BETAS, ema_decay=0.9, ema_warmup=False)
    if fp8:
        scales = m.calibrate_fp8(x)
    ig = InferenceGraph(m, 2, *hw)                        # captured BEFORE the context
    if fp8:
        assert any(op.name == "crd_conv3x3_fp8" for op in ig.plan.fwd)
    for i in range(3):
        run(ts, batches[i])
    raw, ema = m.flat.clone(), ts.ema.clone()
    ema_sd = {k: v.detach().cpu().clone() for k, v in ts.ema_state_dict().items()}
    out_raw = ig.run(x)["depth"]["final_depth"]
    assert not torch.equal(raw, ema)
    with ts.ema_weights():
        torch.cuda.synchronize()
        assert torch.equal(m.flat, ema) and torch.equal(ts.ema, raw)
        for k, v in m.state_dict().items():
            assert torch.equal(v.cpu(), ema_sd[k]), k
        out_ema = ig.run(x)["depth"]["final_depth"]
        with pytest.raises(L.CrdError, match="ema_weights"):
            ts.step()
        with pytest.raises(L.CrdError, match="re-entrant"):
            with ts.ema_weights():
                pass
        assert torch.equal(m.flat, ema)                   # the refused inner context exchanged nothing
    torch.cuda.synchronize()
    assert torch.equal(m.flat, raw) and torch.equal(ts.ema, ema)          # bit-restored
    fresh = prepare(build(ema_sd))
    fresh_ig = InferenceGraph(fresh, 2, *hw)
    if fp8:
        assert any(op.name == "crd_conv3x3_fp8" for op in fresh_ig.plan.fwd)
    out_fresh = fresh_ig.run(x)["depth"]["final_depth"]
    assert torch.equal(out_ema, out_fresh) and not torch.equal(out_ema, out_raw)
    assert torch.equal(ig.run(x)["depth"]["final_depth"], out_raw)         # ... and the raw weights are packed again
    # the next training steps are those of a run that never swapped
    m2, ts2 = make_step(sd, masks, True, hw=hw, lr=LR, betas=BETAS, ema_decay=0.9, ema_warmup=False)
    if fp8:
        prepare(m2)
    for i in range(5):
        run(ts2, batches[i])
    for i in range(3, 5):
        run(ts, batches[i])
    for name, a, b in zip(("flat", "m", "v", "pg", "egn"), snap(m, ts), snap(m2, ts2)):
        assert torch.equal(a, b), name
    assert torch.equal(ts.ema, ts2.ema)
    # an exception inside the context still restores the weights
    with pytest.raises(ZeroDivisionError):
        with ts.ema_weights():
            1 / 0
    torch.cuda.synchronize()
    assert torch.equal(m.flat, ts2.model.flat) and not ts._ema_swapped


# ---------------------------------------------------------------------------------------------- 6. the runner
def test_runner_evaluates_on_the_averaged_weights():
    from camradepth_amd.model import CamRaDepth
    from camradepth_amd.runner import Trainer
    sd = synth.fill_state_dict({n: s for n, s in param_specs(CFG)}, 0)
    train = [synth.make_batch(2, 64, 96, seed=10 + i) for i in range(4)] + [synth.make_batch(1, 64, 96, seed=14)]
    val = [synth.make_batch(2, 64, 96, seed=30 + i) for i in range(2)]
    test = [synth.make_batch(1, 64, 96, seed=40 + i) for i in range(2)]

    def model_of(state):
        m = CamRaDepth(input_channels=7, depths=CFG.depths)
        m.load_state_dict(state)
        return m.cuda().train()
    res = {}
    for with_ema in (True, False):
        m = model_of(sd)
        tr = Trainer(m, train, val, test, learning_rate=1e-3, num_epochs=1, update_interval=2, ema_decay=0.9, ema_warmup=False,
                     eval_with_ema=with_ema)
        before = tr.eval(0)                               # no step yet: the EMA is the parameters
        r = tr.train_one_epoch(0)
        assert tr.training_steps == 3 and all(math.isfinite(v) for v in r.values())
        assert len(tr._steps) == 2 and tr.step.ema_updates == 3          # the ragged last batch continued ONE EMA
        assert all(ts.ema is tr._train_state.ema for ts in tr._steps.values())
        raw = m.flat.clone()
        res[with_ema] = (tr.eval(0), tr.test(), before)
        torch.cuda.synchronize()
        assert torch.equal(m.flat, raw) and m.training
        ema_sd = {k: v.detach().cpu().clone() for k, v in tr.step.ema_state_dict().items()}
        raw_sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ref = {}
    for name, state in (("ema", ema_sd), ("raw", raw_sd)):
        tr = Trainer(model_of(state), None, val, test)
        ref[name] = (tr.eval(0), tr.test())

    def same(a, b):
        a, b = dict(a), dict(b)
        a.pop("time"), b.pop("time")
        return a == b
    assert res[True][0] == ref["ema"][0] and same(res[True][1], ref["ema"][1])
    assert res[False][0] == ref["raw"][0] and same(res[False][1], ref["raw"][1])
    assert ref["ema"][0] != ref["raw"][0] and res[True][2] == res[False][2]


# ---------------------------------------------------------------------------------------------- 7. checkpoint
@pytest.mark.parametrize("skip", [False, True])
def test_checkpoint_round_trip(setup, tmp_path, skip):
    from camradepth_amd.checkpoint import load_checkpoint, save_checkpoint
    sd, masks, batches = setup
    kw = dict(schedule=SCHED, weight_decay=1e-2, skip_nonfinite=skip, ema_decay=0.9999)          # the warm-up needs the count back
    m1, ts1 = make_step(sd, masks, True, **kw)
    for i in range(3):
        run(ts1, batches[i])
    path = str(tmp_path / "ck.pt")
    state = save_checkpoint(path, m1, ts1, steps=(0, 3))
    position = (ts1.sched_steps, ts1.iter_count, ts1.epoch_iter)
    assert set(state) == {"state_dict", "steps", "optimizer", "lr", "ema_state_dict", "ema_decay", "ema_updates"}
    assert state["ema_updates"] == 3 and state["ema_decay"] == 0.9999
    for i in range(3, 6):
        run(ts1, batches[i])
    m2, ts2 = make_step(sd, masks, True, **kw)
    load_checkpoint(path, m2, ts2)
    assert ts2.ema_updates == 3 and not torch.equal(ts2.ema, m2.flat)
    ts2.sched_steps, ts2.iter_count, ts2.epoch_iter = position             # the loop position is the caller's to restore
    for i in range(3, 6):
        run(ts2, batches[i])
    for name, a, b in zip(("flat", "m", "v", "pg", "egn"), snap(m1, ts1), snap(m2, ts2)):
        assert torch.equal(a, b), name
    assert torch.equal(ts1.ema, ts2.ema) and ts1.ema_updates == ts2.ema_updates == 6
    # a checkpoint without an EMA: re-seeded from the loaded weights, the count starts again
    m3, ts3 = make_step(sd, masks, True, **kw)
    run(ts3, batches[0])
    plain = {k: v for k, v in state.items() if not k.startswith("ema_")}
    load_checkpoint(plain, m3, ts3)
    assert ts3.ema_updates == 0 and torch.equal(ts3.ema, m3.flat)
    # model.load_state_dict alone does not touch the EMA
    e = ts1.ema.clone()
    m1.load_state_dict(sd)
    assert torch.equal(ts1.ema, e)
    # EMA off: the reference's keys
    m4, ts4 = make_step(sd, masks, True, schedule=SCHED)
    run(ts4, batches[0])
    assert set(save_checkpoint(str(tmp_path / "off.pt"), m4, ts4)) == {"state_dict", "steps", "optimizer", "lr"}
    # inside the swap a checkpoint's state_dict IS the averaged weights
    with ts2.ema_weights():
        swapped = save_checkpoint(str(tmp_path / "sw.pt"), m2, ts2)
    n0 = m2._names[0]
    assert torch.equal(swapped["state_dict"][n0], ts2.ema_state_dict()[n0].cpu())


# ---------------------------------------------------------------------------------------------- 8. the eager optimizer
@pytest.mark.parametrize("kw", [{}, {"skip_nonfinite": True}], ids=["default", "skip"])
@pytest.mark.parametrize("warmup", [False, True])
def test_eager_optimizer_two_groups_adopted(kw, warmup):
    """Loose tensors (adopted into one flat buffer per group), two param groups with their own lr, one tensor without a gradient."""
    from camradepth_amd.optim import diffGradNorm
    gen = torch.Generator().manual_seed(5)
    shapes = [(17,), (4096,), (4097,), (3, 5000), (64, 64, 3), (9,)]
    ps = [(0.05 * torch.randn(s, generator=gen)).cuda().requires_grad_(True) for s in shapes]
    opt = diffGradNorm([{"params": ps[:2], "lr": 1e-3}, {"params": ps[2:], "lr": 2e-3, "weight_decay": 1e-2}], ema_decay=0.9,
                       ema_warmup=warmup, **kw)
    p0 = [p.detach().clone() for p in ps]
    orcs = None
    for n in range(1, 13):
        for i, p in enumerate(ps):
            p.grad = None if i == 4 else torch.randn(p.shape, generator=gen).cuda()
        opt.step()
        torch.cuda.synchronize()
        es = opt.ema_state()
        if orcs is None:                                   # (the groups are laid out by the first step: seeded with p0)
            orcs = [Oracle(p0_.reshape(-1), [(0, p0_.numel(), i != 4)], 0.9, warmup) for i, p0_ in enumerate(p0)]
        for i, (p, o) in enumerate(zip(ps, orcs)):
            assert es[p].shape == p.shape
            if i != 4:
                o.update(p.reshape(-1))
            else:
                o.ws.append(o.weight(n))
            o.check(es[p].reshape(-1), p.detach().reshape(-1), f"tensor {i} step {n}")
    for i, o in enumerate(orcs):
        if i != 4:
            o.assert_moved()
    assert torch.equal(es[ps[4]], p0[4]) and torch.equal(ps[4].detach(), p0[4])
    assert set(opt.state_dict()["param_groups"][0]) == {"params", "lr", "betas", "eps", "weight_decay"}


# ---------------------------------------------------------------------------------------------- 9. reproducibility
@pytest.mark.parametrize("use_graph", [False, True])
def test_two_runs_give_the_same_ema(setup, use_graph):
    sd, masks, batches = setup
    out = []
    for _ in range(2):
        m, ts = make_step(sd, masks, use_graph, 3, schedule=SCHED, weight_decay=1e-2, ema_decay=0.999)
        for i in range(9):
            run(ts, batches[i % len(batches)])
        out.append(snap(m, ts) + [ts.ema.clone()])
    for name, a, b in zip(("flat", "m", "v", "pg", "egn", "ema"), *out):
        assert torch.equal(a, b), name
    assert not torch.equal(out[0][0], out[0][5])
