"""The two ways of executing a recorded plan that no other test runs: the CRD_DEBUG_SYNC loop (a synchronize behind every launch)
and the split_late mode (backward() leaves out the ops of stream LATE, run_late() runs them and the un-packing afterwards -- what
TrainStep does on its second stream).  Both must leave the flat gradient BIT-equal to the normal pass: every multi-workgroup sum
goes through the 64-bit fixed-point accumulators or index-ordered partial copies, the property
test_training_iteration_is_bit_reproducible rests on."""
import dataclasses

import pytest
import torch

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.engine import Plan
from camradepth_amd.model import CamRaDepth
from camradepth_amd.params import param_specs

pytestmark = pytest.mark.gpu

TAGS = ["dec", "enc3", "enc2", "enc1", "enc0"]


def _step(plan, masks, late=False):
    """One forward + backward on fixed inputs, masks and loss gradients; returns a copy of the flat gradient."""
    plan.model.flat_grad.zero_()
    plan.split_late = late
    try:
        plan.forward(masks=masks)
        plan.backward()
        if late:
            plan.run_late(TAGS)
    finally:
        plan.split_late = False
    torch.cuda.synchronize()
    return plan.model.flat_grad.clone()


@pytest.fixture(scope="module")
def ctx():
    cfg = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1))
    model = CamRaDepth(input_channels=7, depths=cfg.depths)
    model.load_state_dict(synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0))
    model = model.cuda().train()
    model._ensure_grad_views()
    B, H, W = 2, 64, 96
    plan = Plan(model, B, H, W, True)
    plan.x_in.copy_(synth.make_batch(B, H, W, seed=77)["image"])
    masks = synth.make_masks(cfg, B, seed=4321)
    g = torch.Generator().manual_seed(5)
    for j in (3, 4, 5):                      # a fixed loss gradient for the three depth outputs
        gd = plan.out_depth[("grad", j)].t
        gd.copy_(torch.randn(gd.shape, generator=g) * 1e-3)
    ref = _step(plan, masks)
    assert bool(torch.isfinite(ref).all()) and int((ref != 0).sum()) > ref.numel() // 2
    return plan, masks, ref


def test_debug_sync_loop_leaves_the_same_gradient(ctx, monkeypatch):
    plan, masks, ref = ctx
    monkeypatch.setenv("CRD_DEBUG_SYNC", "1")          # read per run_ops call
    got = _step(plan, masks)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} gradient elements differ"


def test_split_late_then_run_late_leaves_the_same_gradient(ctx):
    plan, masks, ref = ctx
    got = _step(plan, masks, late=True)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} gradient elements differ"
    assert torch.equal(_step(plan, masks), ref)        # and the plan is back on the one-stream pass
