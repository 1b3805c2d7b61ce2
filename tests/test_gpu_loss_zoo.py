"""The depth-criterion zoo on the GPU: MaskedL1Loss, MaskedHuberLoss, MaskedRMSELoss, MaskedBerHuLoss and SmoothnessLoss against
the reference-pinned fixture (tests/golden/loss_zoo.npz), their reproducibility, and the criterion of the captured training
step (TrainStep(criterion=...)) and of runner.Trainer."""
import dataclasses

import numpy as np
import pytest
import torch

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.params import param_specs
from tests.loss_zoo_cases import CASES, depth_pair, grad_view, smooth_pair
from tests.util import load_npz

pytestmark = pytest.mark.gpu


def _crit(name):
    from camradepth_amd import losses as HL
    return {"l1": HL.MaskedL1Loss(), "huber": HL.MaskedHuberLoss(), "rmse": HL.MaskedRMSELoss(), "berhu": HL.MaskedBerHuLoss(thresh=0.2),
            "smooth": HL.SmoothnessLoss()}[name]


def _run(case, name):
    """-> (loss, full gradient) of the HIP module on the case's inputs."""
    if name == "smooth":
        p, other = smooth_pair(case)
    else:
        p, other = depth_pair(case)
    x = torch.from_numpy(p).cuda().requires_grad_(True)
    loss = _crit(name)(x, torch.from_numpy(other).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.detach().cpu()


def _assert_grad(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=what)
    ok = ~np.isnan(ref)
    scale = float(np.abs(ref[ok]).max()) if ok.any() else 0.0
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-5, atol=1e-5 * scale, err_msg=what)
    np.testing.assert_array_equal(got[ok] == 0, ref[ok] == 0, err_msg=what + ": zero pattern")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ["l1", "huber", "rmse", "berhu", "smooth"])
def test_matches_reference_fixture(case, name):
    g = load_npz("loss_zoo.npz")
    loss, grad = _run(case, name)
    ref = float(g[f"{case}__{name}__loss"])
    if np.isnan(ref):
        assert torch.isnan(loss), (case, name, float(loss))
    else:
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref) + 1e-7, (case, name, float(loss), ref)
    _assert_grad(grad_view(case, grad.numpy()), g[f"{case}__{name}__grad"], f"{case}/{name}")


@pytest.mark.parametrize("name", ["l1", "huber", "rmse", "berhu", "smooth"])
def test_bit_reproducible(name):
    a, b = _run("odd", name), _run("odd", name)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_berhu_edge_at_fp32_c():
    """Elements at |d| == fp32(c) where fp32(c)^2 > fp32(c^2) (tests/loss_zoo_cases.py, "edge_f32"): the reference rounds |d|^2 before
    it subtracts c^2, so they are in neither part -- no loss and no gradient."""
    p, t = depth_pair("edge_f32")
    c = 0.2 * float(np.abs(p - t)[t > 0].max())
    at_c = torch.from_numpy((t > 0) & (np.abs(p - t) == np.float32(c)))
    loss, grad = _run("edge_f32", "berhu")
    assert int(at_c.sum()) == 16 and not grad[at_c].any()
    ref = float(load_npz("loss_zoo.npz")["edge_f32__berhu__loss"])
    assert abs(float(loss) - ref) <= 1e-5 * ref


def test_berhu_empty_mask_is_nan_with_zero_gradient():
    from camradepth_amd import losses as HL
    x = torch.rand(2, 1, 8, 8, device="cuda").requires_grad_(True)
    loss = HL.MaskedBerHuLoss()(x, torch.zeros(2, 1, 8, 8, device="cuda"))
    loss.backward()
    assert torch.isnan(loss) and torch.equal(x.grad, torch.zeros_like(x))


@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (8, 256, 416)])
def test_smoothness_against_fp64_autograd(B, H, W):
    from camradepth_amd import losses as HL
    gen = torch.Generator().manual_seed(B * H + W)
    p = torch.rand(B, 1, H, W, generator=gen) * 0.9 + 0.05
    im = torch.rand(B, 3, H, W, generator=gen)
    x = p.double().requires_grad_(True)
    n = x / (x.mean(dim=(2, 3), keepdim=True) + 1e-7)
    wx = torch.exp(-(im[..., :, 1:] - im[..., :, :-1]).abs().double().mean(1, keepdim=True))
    wy = torch.exp(-(im[..., 1:, :] - im[..., :-1, :]).abs().double().mean(1, keepdim=True))
    ref = ((n[..., :, 1:] - n[..., :, :-1]).abs() * wx).mean() + ((n[..., 1:, :] - n[..., :-1, :]).abs() * wy).mean()
    ref.backward()
    xc = p.cuda().requires_grad_(True)
    imc = im.cuda().requires_grad_(True)
    loss = HL.SmoothnessLoss()(xc, imc)
    loss.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    _assert_grad(xc.grad.cpu().numpy(), x.grad.numpy(), "smoothness")
    assert imc.grad is None                                          # the image gets no gradient
    with pytest.raises(Exception):
        HL.SmoothnessLoss()(torch.rand(B, 2, H, W, device="cuda"), imc)      # one channel only


# ---- the captured training step -----------------------------------------------------------------------------------------------
def _build(cfg, sd):
    from camradepth_amd.model import CamRaDepth
    m = CamRaDepth(input_channels=cfg.input_channels, depths=cfg.depths, supervised_seg=cfg.supervised_seg,
                   unsupervised_seg=cfg.unsupervised_seg)
    m.load_state_dict(sd)
    return m.cuda().train()


def _fix_masks(ts, masks):
    ts.plan.training_masks_fixed = True
    ts.plan.dp_masks.copy_(torch.stack([t.cuda() for t in masks["drop_path"]]))
    ts.plan.d2_masks.copy_(torch.stack([t.cuda() for t in masks["dropout2d"]]))


def _train(cfg, sd, masks, batches, B, H, W, use_graph, **kw):
    from camradepth_amd.trainer import TrainStep
    m = _build(cfg, sd)
    ts = TrainStep(m, B, H, W, lr=1e-3, use_graph=use_graph, **kw)
    _fix_masks(ts, masks)
    losses, grads = [], []
    for b in batches:
        ts.set_batch(b)
        assert ts.step() is True
        losses.append(ts.losses())
        grads.append(m.flat_grad.clone())
    torch.cuda.synchronize()
    return losses, m.flat.clone(), grads


@pytest.mark.parametrize("use_graph", [True, False])
def test_default_criterion_is_unchanged(use_graph):
    from camradepth_amd import losses as HL
    cfg = dataclasses.replace(ModelConfig.variant("supervised_seg"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    masks = synth.make_masks(cfg, 2, seed=8)
    batches = [{k: v.cuda() for k, v in synth.make_batch(2, 64, 96, seed=60 + i).items()} for i in range(3)]
    a = _train(cfg, sd, masks, batches, 2, 64, 96, use_graph)
    b = _train(cfg, sd, masks, batches, 2, 64, 96, use_graph, criterion={"depth": HL.MaskedSmoothL1Loss(), "seg": HL.MaskedFocalLoss()})
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("name", ["berhu", "l1", "rmse"])
def test_criterion_reaches_the_graph(name):
    """The small configuration of test_graph_step_at_ragged_sizes_matches_eager_step with another depth criterion: graph step and
    eager step agree, the first iteration's losses are the eager module's, and the gradients are not smooth-L1's."""
    from camradepth_amd import losses as HL
    B, H, W = 3, 96, 160
    cfg = dataclasses.replace(ModelConfig.variant("sup_unsup_seg"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    masks = synth.make_masks(cfg, B, seed=5)
    batches = [{k: v.cuda() for k, v in synth.make_batch(B, H, W, seed=40 + i).items()} for i in range(3)]
    crit = {"depth": _crit(name), "seg": HL.MaskedFocalLoss()}
    lg, pg, gg = _train(cfg, sd, masks, batches, B, H, W, True, criterion=crit)
    le, pe, ge = _train(cfg, sd, masks, batches, B, H, W, False, criterion=crit)
    assert lg[0] == le[0], (lg[0], le[0])
    for a, b in zip(lg[1:], le[1:]):
        assert abs(a["loss"] - b["loss"]) < 2e-3 * abs(b["loss"]), (a, b)
    assert _rel(gg[-1], ge[-1]) < 3e-2
    # the eager model + total_loss with the same weights, masks and criterion
    m = _build(cfg, sd)
    out = m(batches[0]["image"], masks=masks)
    loss, parts = HL.total_loss(out, batches[0], cfg.supervised_seg, criterion=crit)
    for key in ("full", "half", "quarter"):
        assert abs(lg[0][key] - float(parts[key])) <= 1e-5 * abs(float(parts[key])), (key, lg[0][key], float(parts[key]))
    assert abs(lg[0]["loss"] - float(loss)) <= 1e-5 * abs(float(loss))
    # the choice is not ignored: smooth-L1's first-iteration gradients differ
    ls, _, gs = _train(cfg, sd, masks, batches[:1], B, H, W, True)
    assert not torch.equal(gs[0], gg[0]) and _rel(gs[0], gg[0]) > 1e-3
    assert ls[0]["full"] != lg[0]["full"] and ls[0]["rmse"] == lg[0]["rmse"]      # "rmse" is the full level's, whatever the criterion


def test_runner_trainer_with_berhu():
    from camradepth_amd import losses as HL
    from camradepth_amd.runner import Trainer
    cfg = dataclasses.replace(ModelConfig.variant("supervised_seg"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    m = _build(cfg, sd)
    train = [synth.make_batch(2, 64, 96, seed=10 + i) for i in range(3)]
    val = [synth.make_batch(2, 64, 96, seed=30 + i) for i in range(2)]
    crit = {"depth": HL.MaskedBerHuLoss(), "seg": HL.MaskedFocalLoss()}
    tr = Trainer(m, train, val, None, learning_rate=1e-3, num_epochs=1, criterion=crit)
    assert tr.criterion is crit
    r = tr.train_one_epoch(0)
    assert tr.step._depth_mode == "berhu"
    assert all(np.isfinite(v) for v in r.values()), r
    val_loss, rmse = tr.eval(0)
    assert np.isfinite(val_loss) and np.isfinite(rmse)
    m.eval()
    with torch.no_grad():
        eager = [float(HL.MaskedBerHuLoss()(m(b["image"].cuda())["depth"]["final_depth"], b["gt_full"].cuda())) for b in val]
    m.train()
    assert abs(val_loss - sum(eager) / len(eager)) <= 1e-5 * abs(val_loss), (val_loss, eager)
