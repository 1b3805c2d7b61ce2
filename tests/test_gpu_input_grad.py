"""GPU tests of the gradient with respect to the model input (x.grad; reference: CamRaDepth.forward under autograd,
src/models/CamRaDepth.py:173-176): the crd_input_grad kernel against an fp64 transposed convolution, the model's x.grad against
the oracle's autograd (with and without the oracle's attention arg-max injected), frozen-model saliency, the default path left
bit-identical, reproducibility, composition with an upstream module, and the fp8 plans."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.params import param_specs
from tests.test_gpu_train import build, inject_argmax, rel

pytestmark = pytest.mark.gpu

WGRAD_OPS = ("crd_conv_wgrad", "crd_conv_wgrad_grouped", "crd_dwconv3x3_wgrad", "crd_head_conv2_wgrad")


def _rel_rgb_radar(g, go):
    """rel-L2 of the RGB channels and of the radar channels separately (a channel-mapping error cannot hide)."""
    return rel(g[:, :3], go[:, :3]), rel(g[:, 3:], go[:, 3:])


# ---------------------------------------------------------------------------------------------------- 1. the kernel
KERNEL_CASES = [(B, H, W, cin, seg) for B in (1, 3) for (H, W) in ((64, 96), (96, 160), (160, 96), (96, 224))
                for cin in (3, 7) for seg in (False, True)]


@pytest.mark.parametrize("B,H,W,cin,seg", KERNEL_CASES)
def test_kernel_matches_fp64_transposed_convolution(B, H, W, cin, seg):
    from camradepth_amd import lib
    L = lib.load()
    g = torch.Generator().manual_seed(B * 1000 + H + W + cin + 7 * seg)
    Hs, Ws, ld, col0 = H // 4, W // 4, 304, 136
    draw = torch.randn(B, Hs * Ws, 64, generator=g).to(torch.bfloat16)
    w = (torch.randn(64, cin, 7, 7, generator=g) / 20).to(torch.bfloat16)
    wpe = torch.randn(64, 49, 8, generator=g).to(torch.bfloat16)            # channels >= cin: garbage the kernel must ignore
    wpe[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(64, 49, cin)
    dcbs = [torch.randn(B, H * W, ld, generator=g).to(torch.bfloat16) for _ in range(2 if seg else 1)]
    ref = F.conv_transpose2d(draw.double().view(B, Hs, Ws, 64).permute(0, 3, 1, 2), w.double(), stride=4, padding=3, output_padding=3)
    for d in dcbs:
        ref = ref + d[:, :, col0:col0 + cin].double().view(B, H, W, cin).permute(0, 3, 1, 2)
    dx = torch.full((B, cin, H, W), float("nan"), device="cuda")                 # every element must be written
    dd, wd = draw.cuda(), wpe.cuda()
    dc = [d.cuda() for d in dcbs]
    lib.check(L.crd_input_grad(dd.data_ptr(), wd.data_ptr(), dc[0].data_ptr(), dc[1].data_ptr() if seg else None, ld, col0, B, H, W,
                               cin, dx.data_ptr(), lib.stream()), "crd_input_grad")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all())
    e = rel(dx, ref)
    print(f"MEASURED kernel B{B} {H}x{W} Cin{cin} seg{int(seg)}: rel-L2 {e:.2e}")
    assert e <= 1e-5, e
    for c in range(cin):
        assert rel(dx[:, c], ref[:, c]) <= 1e-5, c


# ---------------------------------------------------------------------------------------------------- 2-4. the model vs the oracle
def _oracle(cfg, sd, x, masks, batch, frozen=False):
    from oracle import losses as ol
    from oracle import model as om
    sdo = {k: v.clone().requires_grad_(not frozen) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    taps = {}
    o = om.forward(sdo, xo, cfg, quant="bf16", masks=masks, taps=taps)
    lo, _ = ol.total_loss(o, batch, cfg.supervised_seg)
    lo.backward()
    return xo.grad, taps, sdo


def _model_x_grad(cfg, sd, batch, masks, train, taps=None, frozen=False):
    from camradepth_amd import losses as hl
    model = build(cfg, sd, train=train)
    if frozen:
        model.requires_grad_(False)
    x = batch["image"][:, :cfg.input_channels].cuda().requires_grad_(True)
    out = model(x, masks=masks)
    loss, _ = hl.total_loss(out, {k: v.cuda() for k, v in batch.items()}, cfg.supervised_seg)
    plan = model._plans[model._plan_key(x)]
    if taps is not None:
        assert inject_argmax(plan, taps) == 4
    loss.backward()
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    return x.grad, model, plan


# rgb / radar rel-L2 against the oracle with its arg-max injected: measured 0.018-0.027 over the four variants x two modes
# (0.021 frozen; the upstream conv's weight / bias gradients 0.021 / 0.010); bound 2x the worst
ARGMAX_BOUND = 0.055


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("variant", ["base", "supervised_seg", "unsupervised_seg", "sup_unsup_seg"])
def test_model_input_grad_vs_oracle_with_injected_argmax(variant, mode):
    cfg = dataclasses.replace(ModelConfig.variant(variant), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batch = synth.make_batch(2, 64, 96, seed=77)
    masks = synth.make_masks(cfg, 2, seed=4321) if mode == "train" else None
    go, taps, _ = _oracle(cfg, sd, batch["image"], masks, batch)
    g, _, _ = _model_x_grad(cfg, sd, batch, masks, mode == "train", taps)
    e_rgb, e_radar = _rel_rgb_radar(g, go)
    print(f"MEASURED x.grad {variant} {mode} injected arg-max: rgb {e_rgb:.4f} radar {e_radar:.4f}")
    assert e_rgb < ARGMAX_BOUND and e_radar < ARGMAX_BOUND, (e_rgb, e_radar)


RAGGED_BOUND = 0.21          # measured 0.063 / 0.105 / 0.086 (ragged sizes), 0.095 (input_channels=3): 2x the worst


@pytest.mark.parametrize("B,H,W", [(1, 96, 160), (3, 160, 96), (2, 96, 224)])
def test_model_input_grad_ragged_sizes_vs_oracle(B, H, W):
    cfg = dataclasses.replace(ModelConfig.variant("sup_unsup_seg"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batch = synth.make_batch(B, H, W, seed=77)
    masks = synth.make_masks(cfg, B, seed=4321)
    go, _, _ = _oracle(cfg, sd, batch["image"], masks, batch)
    g, _, _ = _model_x_grad(cfg, sd, batch, masks, True)
    e_rgb, e_radar = _rel_rgb_radar(g, go)
    print(f"MEASURED x.grad ragged B{B} {H}x{W}: rgb {e_rgb:.4f} radar {e_radar:.4f}")
    assert e_rgb < RAGGED_BOUND and e_radar < RAGGED_BOUND, (e_rgb, e_radar)


def test_model_input_grad_three_channel_input_vs_oracle():
    cfg = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1), input_channels=3)
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batch = synth.make_batch(2, 64, 96, seed=77)
    masks = synth.make_masks(cfg, 2, seed=4321)
    go, _, _ = _oracle(cfg, sd, batch["image"][:, :3], masks, batch)
    g, _, _ = _model_x_grad(cfg, sd, batch, masks, True)
    e = rel(g, go)
    print(f"MEASURED x.grad input_channels=3: rel {e:.4f}")
    assert g.shape == (2, 3, 64, 96) and e < RAGGED_BOUND, e


def test_frozen_model_saliency():
    """model.requires_grad_(False): x.grad still correct, no parameter gradient, no weight-gradient launch."""
    cfg = dataclasses.replace(ModelConfig.variant("supervised_seg"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batch = synth.make_batch(2, 64, 96, seed=77)
    masks = synth.make_masks(cfg, 2, seed=4321)
    go, taps, sdo = _oracle(cfg, sd, batch["image"], masks, batch, frozen=True)
    g, model, plan = _model_x_grad(cfg, sd, batch, masks, True, taps, frozen=True)
    e_rgb, e_radar = _rel_rgb_radar(g, go)
    print(f"MEASURED x.grad frozen model: rgb {e_rgb:.4f} radar {e_radar:.4f}")
    assert e_rgb < ARGMAX_BOUND and e_radar < ARGMAX_BOUND, (e_rgb, e_radar)
    assert all(p.grad is None for p in model.parameters())
    live = [op.name for op in plan.bwd if plan.live(op)]
    assert not [n for n in live if n in WGRAD_OPS], sorted(set(live))
    plan.want_x_grad = True
    assert "crd_input_grad" in [op.name for op in plan.bwd if plan.live(op)]
    plan.want_x_grad = False


# ---------------------------------------------------------------------------------------------------- 5-7
def _step(model, x, batch, masks, cfg):
    from camradepth_amd import losses as hl
    model.zero_grad()
    out = model(x, masks=masks)
    loss, _ = hl.total_loss(out, {k: v.cuda() for k, v in batch.items()}, cfg.supervised_seg)
    loss.backward()
    torch.cuda.synchronize()
    return out, loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("variant", ["base", "supervised_seg"])
def test_default_path_unchanged_by_input_grad(variant):
    """Outputs and every parameter gradient are bit-identical with and without x.requires_grad."""
    cfg = dataclasses.replace(ModelConfig.variant(variant), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batch = synth.make_batch(2, 64, 96, seed=77)
    masks = synth.make_masks(cfg, 2, seed=4321)
    model = build(cfg, sd)
    x = batch["image"].cuda()
    out0, l0, g0 = _step(model, x, batch, masks, cfg)
    xr = x.clone().requires_grad_(True)
    out1, l1, g1 = _step(model, xr, batch, masks, cfg)
    assert xr.grad is not None
    assert torch.equal(l0, l1)
    assert torch.equal(out0["depth"]["final_depth"], out1["depth"]["final_depth"])
    if cfg.supervised_seg:
        assert torch.equal(out0["seg"]["final_seg"], out1["seg"]["final_seg"])
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_input_grad_reproducible_and_fresh():
    cfg = dataclasses.replace(ModelConfig.variant("supervised_seg"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batch = synth.make_batch(2, 64, 96, seed=77)
    masks = synth.make_masks(cfg, 2, seed=4321)
    model = build(cfg, sd)
    grads = []
    for _ in range(2):
        x = batch["image"].cuda().requires_grad_(True)
        _step(model, x, batch, masks, cfg)
        grads.append(x.grad)
    assert grads[0] is not grads[1] and grads[0].data_ptr() != grads[1].data_ptr()
    assert torch.equal(grads[0], grads[1])
    # a later forward does not touch an earlier x.grad (a fresh tensor, not a view of a plan buffer)
    keep = grads[0].clone()
    other = synth.make_batch(2, 64, 96, seed=78)
    x = other["image"].cuda().requires_grad_(True)
    _step(model, x, other, masks, cfg)
    assert torch.equal(grads[0], keep) and not torch.equal(x.grad, keep)


def test_composition_with_upstream_module():
    """model(pre(x)) with a learnable 1x1 pre-processing conv: pre.weight.grad matches the oracle chain."""
    from camradepth_amd import losses as hl
    from oracle import losses as ol
    from oracle import model as om
    cfg = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batch = synth.make_batch(2, 64, 96, seed=77)
    masks = synth.make_masks(cfg, 2, seed=4321)
    torch.manual_seed(5)
    pre = torch.nn.Conv2d(7, 7, 1)
    with torch.no_grad():
        pre.weight.copy_(torch.eye(7).view(7, 7, 1, 1) + 0.1 * pre.weight)
    pre_o = torch.nn.Conv2d(7, 7, 1)
    pre_o.load_state_dict(pre.state_dict())
    sdo = {k: v.clone() for k, v in sd.items()}
    taps = {}
    o = om.forward(sdo, pre_o(batch["image"]), cfg, quant="bf16", masks=masks, taps=taps)
    lo, _ = ol.total_loss(o, batch, False)
    lo.backward()
    model = build(cfg, sd)
    pre = pre.cuda()
    out = model(pre(batch["image"].cuda()), masks=masks)
    assert inject_argmax(model._plans[next(iter(model._plans))], taps) == 4
    loss, _ = hl.total_loss(out, {k: v.cuda() for k, v in batch.items()}, False)
    loss.backward()
    ew, eb = rel(pre.weight.grad, pre_o.weight.grad), rel(pre.bias.grad, pre_o.bias.grad)
    print(f"MEASURED pre.weight.grad rel {ew:.4f}, pre.bias.grad rel {eb:.4f}")
    assert ew < ARGMAX_BOUND and eb < ARGMAX_BOUND, (ew, eb)


# ---------------------------------------------------------------------------------------------------- 8. fp8 plans
FP8_BOUND = 0.032            # measured 0.0157 (fp8-forward plan against the bf16 plan): 2x


def test_fp8_plans():
    from camradepth_amd import lib
    from camradepth_amd import losses as hl
    cfg = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    B, H, W = 8, 128, 192                      # large enough for the full-resolution stage to take the fp8 route
    batch = synth.make_batch(B, H, W, seed=77)
    masks = synth.make_masks(cfg, B, seed=4321)
    gb = {k: v.cuda() for k, v in batch.items()}

    def run(model):
        x = batch["image"].cuda().requires_grad_(True)
        model.zero_grad()
        out = model(x, masks=masks)
        loss, _ = hl.total_loss(out, gb, False)
        loss.backward()
        return x.grad, model._plans[model._plan_key(x)]

    g_bf16, _ = run(build(cfg, sd))
    m8 = build(cfg, sd)
    m8.calibrate_fp8(batch["image"][:2].cuda(), train=True, grads=True)
    x = batch["image"].cuda().requires_grad_(True)
    out = m8(x, masks=masks)
    plan = m8._plans[m8._plan_key(x)]
    assert plan.fp8_grad
    loss, _ = hl.total_loss(out, gb, False)
    with pytest.raises(lib.CrdError, match="e4m3"):
        loss.backward()
    assert plan.want_x_grad is False
    m8.calibrate_fp8(batch["image"][:2].cuda(), train=True, grads=False)      # fp8 forward, bf16 data gradients
    g8, plan = run(m8)
    assert plan.fp8 is not None and not plan.fp8_grad
    assert bool(torch.isfinite(g8).all())
    e = rel(g8, g_bf16)
    print(f"MEASURED fp8-forward x.grad vs bf16 plan: rel {e:.4f}")
    assert e < FP8_BOUND, e
