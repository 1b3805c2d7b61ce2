"""CPU: the gradient with respect to the model input (x.grad).

* The oracle's autograd x.grad, in fp64, against the reference's fp64 run (tests/golden/make_input_grad_golden.py).
* The plan records ONE crd_input_grad launch at the end of the enc0 backward segment, live only while want_x_grad is set: with it
  off, the live op lists and bench.floor_budget are those of a plan built without the feature.
* The entry point refuses bad arguments before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

import bench
from camradepth_amd import lib as L
from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.engine import Plan
from camradepth_amd.model import CamRaDepth
from oracle import losses as ol
from oracle import model as om
from tests.golden.make_input_grad_golden import sample_positions
from tests.util import golden_state_dict, load_npz


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("variant", ["base", "supervised_seg"])
def test_oracle_input_grad_fp64_matches_reference(variant, mode):
    g = load_npz("input_grad_fp64.npz")
    key = f"{variant}_{mode}_"
    cfg = ModelConfig.variant(variant)
    sd = {k: v.double() for k, v in golden_state_dict(cfg).items()}
    batch = synth.make_batch(2, 64, 96, seed=77)
    batch = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    masks = synth.make_masks(cfg, 2, seed=4321) if mode == "train" else None
    if masks is not None:
        masks = {k: [t.double() for t in v] for k, v in masks.items()}
    x = batch["image"].clone().requires_grad_(True)
    out = om.forward(sd, x, cfg, masks=masks)
    loss, parts = ol.total_loss(out, batch, cfg.supervised_seg)
    loss.backward()
    terms = [float(loss.detach()), float(parts["full"]), float(parts["half"]), float(parts["quarter"]), float(parts["seg"]), float(parts["rmse"].detach())]
    np.testing.assert_allclose(terms, g[key + "loss"], rtol=1e-8, atol=1e-12)
    gx = x.grad.detach()
    bi, yi, xi = sample_positions(2, 64, 96)
    samp = gx[bi, :, yi, xi].numpy()
    ref = g[key + "xgrad_sample"]
    for c in range(7):               # per channel: an RGB / radar channel mix-up cannot hide behind the others' magnitude
        rel = np.linalg.norm(samp[:, c] - ref[:, c]) / np.linalg.norm(ref[:, c])
        assert rel <= 1e-8, (c, rel)
    # whole-tensor sums; a channel sum can cancel to far below its terms, so its bound scales with their L2 norm
    scale = np.sqrt(g[key + "xgrad_chan_sumsq"] * gx[:, 0].numel())
    np.testing.assert_array_less(np.abs(gx.sum(dim=(0, 2, 3)).numpy() - g[key + "xgrad_chan_sum"]), 1e-8 * scale)
    np.testing.assert_allclose((gx * gx).sum(dim=(0, 2, 3)).numpy(), g[key + "xgrad_chan_sumsq"], rtol=1e-8)


def _model(variant, cin=7):
    m = CamRaDepth(input_channels=cin, depths=(1, 1, 1, 1), **variant)
    m.train(True)
    m._ensure_grad_views()
    return m


def _without_feature(self, *a):
    self.want_x_grad, self.x_grad_op = False, None


VARIANTS = [{}, {"supervised_seg": True}, {"unsupervised_seg": True}, {"supervised_seg": True, "unsupervised_seg": True}]


@pytest.mark.parametrize("variant", VARIANTS)
def test_plan_records_one_conditional_input_grad_launch(variant, monkeypatch):
    p = Plan(_model(variant), 2, 64, 96, True)
    off = [(op.name, op.stream) for op in p.fwd + p.bwd if p.live(op)]
    fb_off = bench.floor_budget(p)
    with monkeypatch.context() as mp:
        mp.setattr(Plan, "_input_grad_op", _without_feature)
        p0 = Plan(_model(variant), 2, 64, 96, True)
    assert off == [(op.name, op.stream) for op in p0.fwd + p0.bwd if p0.live(op)]
    assert fb_off == bench.floor_budget(p0)
    assert "crd_input_grad" not in [n for n, _ in off]

    off_bwd = [op for op in p.bwd if p.live(op)]
    p.want_x_grad = True
    on = [op for op in p.bwd if p.live(op)]
    assert len(on) == len(off_bwd) + 1 and [op for op in on if op not in off_bwd] == [p.x_grad_op]
    assert p.x_grad_op.name == "crd_input_grad"
    # at the end of the enc0 segment, behind the stage-0 patch embed's GroupNorm backward (which writes `draw`, its first operand)
    tag, a, b = p.bwd_segments[-1]
    assert tag == "enc0" and p.bwd[b - 1] is p.x_grad_op
    writer = [i for i in range(a, b) if p.bwd[i].name == "crd_gn_bwd_apply" and p.x_grad_op.args[0] in p.bwd[i].args]
    assert len(writer) == 1 and writer[0] < b - 1
    op = p.x_grad_op
    seg = bool(variant.get("supervised_seg"))
    assert (op.args[3] is not None) == seg                     # the seg branch's x columns only where that branch has a loss
    B, H, W, C = 2, 64, 96, 7
    assert p.op_bytes(op) == B * 16 * 24 * 64 * 2 + B * H * W * C * 2 * (2 if seg else 1) + B * C * H * W * 4 + 64 * 49 * 8 * 2
    assert op.meta["flops"] == 2.0 * B * C * 64 * (7 * 16 - 3) * (7 * 24 - 3)
    fb_on = bench.floor_budget(p)
    assert fb_on["phases"]["bwd:enc0"]["launches"] == fb_off["phases"]["bwd:enc0"]["launches"] + 1
    p.want_x_grad = False


def test_fp8_gradient_plan_refuses_input_grad():
    m = _model({})
    m.__dict__["fp8_scales"] = {"depth_upsample.3": 0.01, "depth_upsample.4": 0.01}
    m.__dict__["fp8_train"] = True
    m.__dict__["fp8_grad"] = True
    p = Plan(m, 8, 128, 192, True)
    assert p.fp8_grad
    with pytest.raises(L.CrdError, match="e4m3"):
        p.set_x_grad(torch.empty((8, 7, 128, 192)))
    assert p.want_x_grad is False
    m.__dict__["fp8_grad"] = False                          # fp8 forward only: bf16 data gradients, x.grad available
    p = Plan(m, 8, 128, 192, True)
    assert not p.fp8_grad
    p.set_x_grad(torch.empty((8, 7, 128, 192)))
    assert p.want_x_grad is True


def test_entry_point_refuses_bad_arguments():
    lib = L.load()
    buf = (ctypes.c_uint8 * 256)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    ok = dict(draw=base, wpe=base, dcb=base, seg=None, ld=304, col0=136, B=2, H=64, W=96, Cin=7, dx=base)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.crd_input_grad(a["draw"], a["wpe"], a["dcb"], a["seg"], a["ld"], a["col0"], a["B"], a["H"], a["W"], a["Cin"], a["dx"], None)

    for bad in (dict(draw=None), dict(wpe=None), dict(dcb=None), dict(dx=None)):
        assert call(**bad) == -1, bad
        assert b"null" in lib.crd_last_error()
    assert call(dx=base + 4) == -1                            # float4 stores
    assert call(Cin=9) == -2 and b"Cin" in lib.crd_last_error()
    assert call(Cin=0) == -2
    assert call(H=66) == -2 and b"multiples of 4" in lib.crd_last_error()
    assert call(W=98) == -2
    assert call(col0=300) == -1                               # x columns past the row stride
    assert call(B=0) == -1
