"""Pins the CPU oracle (oracle/) against fixtures produced by the imported reference
(tests/golden/make_golden.py). CPU only."""
import numpy as np
import pytest
import torch

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.params import param_specs
from oracle import losses as olosses
from oracle import model as omodel
from oracle import optim as ooptim
from tests.util import golden_state_dict, load_npz, max_err, param_order, rel_err, subsample

VARIANTS = ["base", "supervised_seg", "unsupervised_seg", "sup_unsup_seg"]
TOL = 2e-5  # fp32 CPU vs fp32 CPU, different op grouping only


@pytest.mark.parametrize("variant", VARIANTS)
def test_param_inventory_matches_reference(variant):
    cfg = ModelConfig.variant(variant)
    ref = param_order(variant)
    mine = [[n, list(s)] for n, s in param_specs(cfg)]
    assert mine == ref["params"]
    assert [n for n, _ in mine] == ref["state_dict_keys"]
    assert sum(int(np.prod(s)) for _, s in mine) == ref["num_params"]
    if variant == "base":
        assert ref["num_params"] == 21966595 and len(mine) == 881


def fp32_close(o32, g32, g64, tol):
    """An fp32 oracle output against the reference's fp32 (g32) and fp64 (g64) runs of the same computation: within `tol` of g32,
    or -- where the reference's own fp32 rounding is larger than that -- no further from the fp64 result than 8 times the reference's
    fp32 output is.  How fp32 sums are grouped depends on the CPU's thread count and instruction set: the same oracle lies up to
    5 times the reference's fp32 error from the fp64 result on the CPUs this was measured on (encoder maps of magnitude ~40: 3e-4)."""
    return max_err(o32, g32) < tol or max_err(o32, g64) < 8 * max_err(g32, g64)


@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_eval_64x96(variant):
    """The eval forward in fp64 against the reference's own fp64 run (tests/golden/make_fp64_golden.py): the two agree to the last
    bits whatever CPU runs the test; and in fp32 against the reference's fp32 run (fp32_close)."""
    cfg = ModelConfig.variant(variant)
    g, g64 = load_npz(f"forward64x96_{variant}.npz"), load_npz(f"forward64x96_fp64_{variant}.npz")
    batch = synth.make_batch(1, 64, 96, seed=1234)
    taps, taps64 = {}, {}
    with torch.no_grad():
        out = omodel.forward(golden_state_dict(cfg), batch["image"], cfg, taps=taps)
        out64 = omodel.forward({k: v.double() for k, v in golden_state_dict(cfg).items()}, batch["image"].double(), cfg, taps=taps64)
    for i in range(4):
        k = f"eval_enc{i + 1}"
        assert max_err(taps64[f"enc{i + 1}"].numpy(), g64[k]) < 1e-8, k
        assert fp32_close(taps[f"enc{i + 1}"].numpy(), g[k], g64[k], 1e-4), k
    for k, j in (("eval_final_depth", None), ("eval_depth_half", 3), ("eval_depth_quarter", 2)):
        o64, o32 = ((o["depth"]["final_depth"] if j is None else o["depth"]["intermediate_depths"][j]).numpy() for o in (out64, out))
        assert max_err(o64, g64[k]) < 1e-8, k
        assert fp32_close(o32, g[k], g64[k], TOL), k
    if cfg.supervised_seg:
        s64 = out64["seg"]["final_seg"].numpy().reshape(-1)
        assert max_err(s64[::max(1, -(-s64.size // 32768))], g64["eval_final_seg"]) < 1e-7      # (subsample() rounds to fp32)
        assert fp32_close(subsample(out["seg"]["final_seg"], 32768), g["eval_final_seg"], g64["eval_final_seg"], 1e-4)
    if cfg.unsupervised_seg:
        assert np.array_equal(out64["seg"]["unsup_map"].numpy(), g64["eval_unsup_map"].astype(np.float32))
        assert np.array_equal(out["seg"]["unsup_map"].numpy(), g["eval_unsup_map"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", ["evalgrad", "train"])
def test_loss_and_grads_64x96(variant, mode):
    cfg = ModelConfig.variant(variant)
    sd = {k: v.clone().requires_grad_(True) for k, v in golden_state_dict(cfg).items()}
    g = load_npz(f"forward64x96_{variant}.npz")
    batch = synth.make_batch(2, 64, 96, seed=77)
    masks = synth.make_masks(cfg, 2, seed=4321) if mode == "train" else None
    x = batch["image"].clone().requires_grad_(True)
    out = omodel.forward(sd, x, cfg, masks=masks)
    loss, parts = olosses.total_loss(out, batch, cfg.supervised_seg)
    loss.backward()
    ref = g[mode + "_loss"]
    got = [float(loss.detach()), float(parts["full"]), float(parts["half"]), float(parts["quarter"]), float(parts["seg"]),
           float(parts["rmse"])]
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6)
    assert max_err(out["depth"]["final_depth"].detach().numpy(), g[mode + "_final_depth"]) < TOL
    assert rel_err(subsample(x.grad, 32768), g[mode + "_grad_input"]) < 1e-3
    for key in g:
        if key.startswith(mode + "_grad:"):
            name = key.split(":", 1)[1]
            if g[key].size == 0:  # the reference produces no gradient (argmax-only consumers, Q8)
                assert sd[name].grad is None, name
                continue
            assert rel_err(subsample(sd[name].grad), g[key]) < 1e-3, name
    norms = np.array([float(sd[n].grad.norm()) if sd[n].grad is not None else -1.0 for n, _ in param_specs(cfg)])
    np.testing.assert_allclose(norms, g[mode + "_gradnorms"], rtol=2e-3, atol=1e-7)


@pytest.mark.parametrize("variant", ["base", "supervised_seg"])
def test_forward_eval_256x416(variant):
    cfg = ModelConfig.variant(variant)
    sd = golden_state_dict(cfg)
    g = load_npz(f"forward256x416_{variant}.npz")
    batch = synth.make_batch(1, 256, 416, seed=1234)
    taps = {}
    with torch.no_grad():
        out = omodel.forward(sd, batch["image"], cfg, taps=taps)
        loss, parts = olosses.total_loss(out, batch, cfg.supervised_seg)
    assert max_err(out["depth"]["final_depth"].numpy(), g["final_depth"]) < 5e-5
    assert max_err(out["depth"]["intermediate_depths"][2].numpy(), g["depth_quarter"]) < 5e-5
    assert max_err(out["depth"]["intermediate_depths"][3].numpy(), g["depth_half"].astype(np.float32)) < 2e-3
    for i in range(4):
        e = taps[f"enc{i + 1}"]
        np.testing.assert_allclose([float(e.mean()), float(e.norm())], g[f"enc{i + 1}_stats"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(parts["rmse"]), g["loss"][5], rtol=1e-4)
    if cfg.supervised_seg:
        am = out["seg"]["final_seg"].argmax(1).numpy().astype(np.uint8)
        assert (am != g["seg_argmax"]).mean() < 1e-4


def test_leaf_modules():
    g = load_npz("leaf_modules.npz")

    def sd_for(shapes, seed, prefix="m."):
        return {prefix + k: v for k, v in synth.fill_state_dict(shapes, seed).items()}

    def blk_shapes(dim, ratio, sr):
        hid = dim * ratio
        s = {"norm1.weight": (dim,), "norm1.bias": (dim,), "norm2.weight": (dim,), "norm2.bias": (dim,),
             "attn.q.weight": (dim, dim, 1), "attn.q.bias": (dim,), "attn.k.weight": (dim, dim, 1), "attn.k.bias": (dim,),
             "attn.proj.weight": (dim, dim, 1), "attn.proj.bias": (dim,),
             "mlp1.fc1.weight": (hid, dim, 1), "mlp1.fc1.bias": (hid,), "mlp1.dwconv.dwconv.weight": (hid, 1, 3, 3),
             "mlp1.dwconv.dwconv.bias": (hid,), "mlp1.fc2.weight": (dim, hid, 1), "mlp1.fc2.bias": (dim,),
             "mlp1.norm1.weight": (hid,), "mlp1.norm1.bias": (hid,), "mlp1.norm2.weight": (hid,), "mlp1.norm2.bias": (hid,)}
        if sr > 1:
            s.update({"attn.sr.weight": (dim, dim, sr, sr), "attn.sr.bias": (dim,), "attn.norm.weight": (dim,),
                      "attn.norm.bias": (dim,)})
        return s

    with torch.no_grad():
        for tag, (dim, heads, ratio, sr, H, W) in {"blk_sr2": (32, 2, 4, 2, 8, 12), "blk_sr1": (48, 3, 2, 1, 4, 6),
                                                    "blk_sr4": (32, 1, 8, 4, 8, 8)}.items():
            sd = sd_for(blk_shapes(dim, ratio, sr), 11)
            x = torch.from_numpy(g[f"{tag}_x"])
            assert max_err(omodel.block(sd, "m", x, H, W, heads, sr).numpy(), g[f"{tag}_y"]) < TOL
            xn = torch.nn.functional.group_norm(x, dim // 16, sd["m.norm1.weight"], sd["m.norm1.bias"])
            assert max_err(omodel.attention_maxpool(sd, "m.attn", xn, H, W, heads, sr).numpy(), g[f"{tag}_attn_y"]) < TOL
            assert max_err(omodel.mlp(sd, "m.mlp1", xn, H, W, dim).numpy(), g[f"{tag}_mlp_y"]) < TOL
        sd = sd_for({"proj.weight": (32, 7, 7, 7), "proj.bias": (32,), "norm.weight": (32,), "norm.bias": (32,)}, 12)
        assert max_err(omodel.patch_embed(sd, "m", torch.from_numpy(g["pe7_x"]), 7, 4)[0].numpy(), g["pe7_y"]) < TOL
        sd = sd_for({"proj.weight": (32, 16, 3, 3), "proj.bias": (32,), "norm.weight": (32,), "norm.bias": (32,)}, 13)
        assert max_err(omodel.patch_embed(sd, "m", torch.from_numpy(g["pe3_x"]), 3, 2)[0].numpy(), g["pe3_y"]) < TOL
        x = torch.from_numpy(g["convlayer_x"])
        sd = sd_for({"model.0.weight": (32, 24, 3, 3), "model.1.weight": (32,), "model.1.bias": (32,)}, 14)
        assert max_err(omodel.conv_layer(sd, "m", x, 3).numpy(), g["convlayer_y"]) < TOL

        def srb_shapes(cin, pre=""):
            s = {}
            for li, (ci, co) in enumerate([(cin, 96), (cin + 96, 64), (cin + 160, 128)]):
                s[f"{pre}layers.{li}.model.0.weight"] = (co, ci, 3, 3)
                s[f"{pre}layers.{li}.model.1.weight"] = (co,)
                s[f"{pre}layers.{li}.model.1.bias"] = (co,)
            return s
        sd = sd_for(srb_shapes(24), 15)
        assert max_err(omodel.short_res_block(sd, "m", x).numpy(), g["srb_y"]) < TOL
        sd = sd_for(srb_shapes(24, "conv."), 16)
        xd, skip = torch.from_numpy(g["dec_x"]), torch.from_numpy(g["dec_skip"])
        assert max_err(omodel.decoder_stage(sd, "m", xd, skip).numpy(), g["dec_y"]) < TOL
        assert max_err(omodel.bicubic2x(xd).numpy(), g["bicubic_y"]) == 0.0
        sd = sd_for({"conv_1.weight": (32, 24, 3, 3), "conv_1.bias": (32,), "conv_2.weight": (1, 32, 3, 3),
                     "conv_2.bias": (1,)}, 17)
        x = torch.from_numpy(g["da_x"])
        assert max_err(omodel.depth_activation(sd, "m", x).numpy(), g["da_y"]) < TOL
        assert np.array_equal(omodel.seg_block(x[:, :21], 21).numpy(), g["segblock_y"])


def test_diffgradnorm_40_steps():
    g = load_npz("diffgradnorm_40steps.npz")
    ps = [torch.from_numpy(g[f"p{j}_init"]).clone() for j in range(3)]
    sts = [ooptim.new_state(p) for p in ps]
    branch_taken = 0
    for it in range(40):
        lr, b1, b2 = g["hp"][it]
        for j in range(3):
            grad = torch.from_numpy(g[f"p{j}_grads"][it])
            e_prev = float(sts[j]["exp_grad_norm"])
            branch_taken += int(0.95 * e_prev + 0.05 * float(grad.norm()) > float(grad.norm()))
            ooptim.step_tensor(ps[j], grad, sts[j], lr, b1, b2)
            np.testing.assert_allclose(ps[j].numpy(), g[f"p{j}_traj"][it], rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(float(sts[j]["exp_grad_norm"]), g["exp_grad_norm"][it][j], rtol=1e-6)
    assert branch_taken >= 6  # the norm-correction branch (diffGradNorm.py:84) is exercised
    for j in range(3):
        np.testing.assert_allclose(sts[j]["exp_avg"].numpy(), g[f"p{j}_exp_avg"], rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(sts[j]["exp_avg_sq"].numpy(), g[f"p{j}_exp_avg_sq"], rtol=1e-5, atol=1e-10)
    sched = ooptim.one_cycle_schedule(41, 6e-5)
    np.testing.assert_allclose([s[0] for s in sched[:40]], g["hp"][:, 0], rtol=1e-9)
    np.testing.assert_allclose([s[1] for s in sched[:40]], g["hp"][:, 1], rtol=1e-9)


def test_losses_and_metrics():
    g = load_npz("losses_metrics.npz")
    b = synth.make_batch(2, 24, 40, seed=3)
    pred, logits = torch.from_numpy(g["pred"]), torch.from_numpy(g["logits"])
    np.testing.assert_allclose(float(olosses.masked_smooth_l1(pred, b["gt_full"])), g["smooth_l1"], rtol=1e-6)
    np.testing.assert_allclose(float(olosses.masked_mse(pred, b["gt_full"])), g["mse"], rtol=1e-6)
    np.testing.assert_allclose(float(olosses.masked_focal(logits, b["seg"])), g["focal"], rtol=1e-6)
    m = olosses.test_metrics(pred[0], b["gt_full"][0])
    np.testing.assert_allclose([m["MAE"], m["RMSE"], m["REL"]], g["metrics"], rtol=1e-5)


def test_label_resize_oracle_matches_scipy_zoom():
    """oracle.data.resize_labels against scipy.ndimage.zoom(order=0, grid_mode=True), the routine scikit-image 0.19.3's
    resize(order=0, anti_aliasing=False) calls (dataloader.py:262-267)."""
    import scipy.ndimage as ndi
    from oracle import data as od
    rs = np.random.RandomState(0)
    for (SH, SW), (DH, DW) in [((450, 800), (416, 800)), ((450, 800), (208, 400)), ((37, 53), (16, 20)), ((20, 31), (33, 50)),
                              ((416, 800), (256, 416))]:
        m = rs.randint(0, 22, size=(SH, SW)).astype(np.uint8)
        rows = min(416, SH)
        src = m[:rows].astype(np.float64)
        ref = ndi.zoom(src, [DH / src.shape[0], DW / src.shape[1]], order=0, mode="reflect", grid_mode=True)
        assert ref.shape == (DH, DW)
        assert np.array_equal(od.resize_labels(m, (DH, DW), rows=416), ref.astype(np.int64))


def test_seg_iou_oracle_properties():
    from oracle import losses as ol
    rs = np.random.RandomState(1)
    t = torch.from_numpy(rs.randint(0, 21, size=(1, 12, 20)).astype(np.int64))
    perfect = torch.nn.functional.one_hot(t, 21).permute(0, 3, 1, 2).float()
    assert ol.seg_iou(perfect, t) == pytest.approx(len(torch.unique(t)) / 21.0)      # absent classes score 0
    t2 = t.clone()
    t2[0, 0, 0] = 255
    assert np.isnan(ol.seg_iou(perfect, t2))                                         # the reference's caught ValueError
    # two classes, hand-computed: target [0,0,1,1], pred [0,1,1,1] -> IoU0 = 1/2, IoU1 = 2/3
    lg = torch.tensor([[[[1.0, 0.0, 0.0, 0.0]], [[0.0, 1.0, 1.0, 1.0]]]])
    assert ol.seg_iou(lg, torch.tensor([[[0, 0, 1, 1]]]), num_classes=2) == pytest.approx((0.5 + 2 / 3) / 2)


def test_oracle_fp8_mode_semantics():
    """The oracle's fp8 ConvLayer mode (BASELINE config 5; nothing in the reference corresponds, so this pins the DEFINITION the
    HIP path is tested against): operands are exactly e4m3-representable after scaling, the result equals a plain fp32
    convolution of the de-quantised operands rounded to bf16, an all-zero weight row gets scale 1, and under autograd the value
    is the fp8 convolution's while the gradients are the bf16 convolution's (straight-through)."""
    import torch.nn.functional as F
    from oracle import model as om
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 24, 9, 11, generator=g) * 2
    w = torch.randn(16, 24, 3, 3, generator=g) * 0.2
    w[5] = 0
    s = float(x.abs().max()) / 448.0
    y = om._conv2d_fp8(x, w, s, padding=1)
    xb, wb = x.bfloat16().float(), w.bfloat16().float()
    xq = (xb * (1.0 / torch.tensor(s))).clamp(-448, 448).to(torch.float8_e4m3fn).float()
    am = wb.abs().amax(dim=(1, 2, 3))
    ws = torch.where(am > 0, am / 448.0, torch.ones_like(am))
    assert float(ws[5]) == 1.0
    wq = (wb * (1.0 / ws).view(-1, 1, 1, 1)).to(torch.float8_e4m3fn).float()
    ref = (F.conv2d(xq, wq, None, padding=1) * (torch.tensor(s) * ws).view(1, -1, 1, 1)).bfloat16().float()
    assert torch.equal(y, ref)
    assert float(y[:, 5].abs().max()) == 0.0
    # quantisation error of e4m3 operands: a few percent of the bf16 convolution
    y16 = om._conv2d(x, w, None, "bf16", padding=1)
    assert 1e-3 < float((y - y16).norm() / y16.norm()) < 0.08
    # straight-through: forward value of the fp8 path, gradients of the bf16 path
    sd = {"l.model.0.weight": w.clone().requires_grad_(True), "l.model.1.weight": torch.ones(16), "l.model.1.bias": torch.zeros(16)}
    xr = x.clone().requires_grad_(True)
    out8 = om.conv_layer(sd, "l", xr, 3, "bf16", fp8_scale=s)
    with torch.no_grad():
        out8_ng = om.conv_layer(sd, "l", x, 3, "bf16", fp8_scale=s)
    assert torch.allclose(out8, out8_ng, atol=1e-6)
    out8.square().sum().backward()
    gx8, gw8 = xr.grad.clone(), sd["l.model.0.weight"].grad.clone()
    # the same thing spelled out: bf16 convolution for the gradient, its value replaced by the fp8 convolution's
    x2, w2 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y16b = om._conv2d(x2, w2, None, "bf16", padding=1)
    yv = y16b + (y - y16b).detach()
    out = F.gelu(om._gn(yv, sd, "l.model.1", 1))
    out.square().sum().backward()
    assert torch.allclose(gx8, x2.grad, rtol=1e-5, atol=1e-7) and torch.allclose(gw8, w2.grad, rtol=1e-5, atol=1e-7)
    assert float(gw8[5].abs().max()) > 0.0      # the zero weight row still receives its (bf16-path) gradient


@pytest.mark.parametrize("tag,B,H,W,seed", [("64", 2, 64, 96, 77), ("256", 1, 256, 416, 1234)])
def test_oracle_bf16_mode_lies_inside_the_references_own_bf16_spread(tag, B, H, W, seed):
    """The yardstick most GPU tests compare against is oracle.forward(quant="bf16"), whose rounding points this build chose (CUDA
    autocast's policy: bf16 conv / matmul operands and results, fp32 GroupNorm).  tests/golden/ref_autocast_bf16.npz holds the REAL
    reference run under torch.autocast("cpu", bfloat16) -- the one autocast the build container can execute; it also runs GroupNorm
    in bf16, so it is the noisier of the two -- next to its own fp32 run, on the golden weights (tests/golden/make_autocast_fixture.py).
    The oracle's bf16 mode has to (a) move away from fp32 at all, (b) stay inside the reference's own bf16 distance, (c) sit no further
    from the reference's bf16 run than the two distances add up to -- for the final depth, the loss and the per-parameter gradient norms."""
    cfg = ModelConfig.variant("base")
    g = load_npz("ref_autocast_bf16.npz")
    batch = synth.make_batch(B, H, W, seed=seed)
    sd = {k: v.clone().requires_grad_(True) for k, v in golden_state_dict(cfg).items()}
    out = omodel.forward(sd, batch["image"], cfg, quant="bf16")
    loss, _ = olosses.total_loss(out, batch, False)
    loss.backward()
    ob = out["depth"]["final_depth"].detach().numpy()
    rf, ra = g[f"fp32_final_depth_{tag}"], g[f"autocast_final_depth_{tag}"]
    d_ob, d_ra, d_x = rel_err(ob, rf), rel_err(ra, rf), rel_err(ob, ra)
    assert 1e-3 < d_ob <= d_ra, (d_ob, d_ra)                    # measured 64x96: 0.010 / 0.025; 256x416: 0.0187 / 0.0438
    assert d_x <= 1.1 * (d_ob + d_ra), (d_x, d_ob, d_ra)        # measured 256x416: 0.028
    lf, la = g[f"fp32_loss_{tag}"], g[f"autocast_loss_{tag}"]
    assert abs(float(loss) - lf[0]) <= 2.0 * abs(la[0] - lf[0]) + 2e-3 * abs(lf[0]), (float(loss), lf[0], la[0])
    # per-parameter gradient norms: the spread of log(norm / fp32 norm) over the 881 tensors, oracle bf16 vs reference autocast
    gn = np.array([float(sd[n].grad.norm()) if sd[n].grad is not None else -1.0 for n, _ in param_specs(cfg)])
    nf, na = g[f"fp32_gradnorms_{tag}"], g[f"autocast_gradnorms_{tag}"]
    ok = (nf > 1e-12) & (na > 0) & (gn > 0)
    assert ok.sum() > 800
    s_o = np.median(np.abs(np.log(gn[ok] / nf[ok])))
    s_a = np.median(np.abs(np.log(na[ok] / nf[ok])))
    assert s_o <= 1.5 * s_a + 1e-3, (s_o, s_a)
    # with the golden weights bf16 INFLATES the encoder's gradient norms (the arg-max routing amplifies rounding noise): the reference's
    # own autocast run shows the bias (median log ratio 64x96: -0.06, 256x416: +0.33), the oracle's bf16 mode the same direction, smaller
    # (-0.08 / +0.19); the two agree with each other better than either does with fp32 (median |log ratio| 0.02 / 0.17)
    m_o, m_a = np.median(np.log(gn[ok] / nf[ok])), np.median(np.log(na[ok] / nf[ok]))
    assert abs(m_o) <= 1.5 * abs(m_a) + 0.05, (m_o, m_a)
    assert np.median(np.abs(np.log(gn[ok] / na[ok]))) <= max(s_o, s_a), "oracle bf16 is closer to the reference's bf16 run than to fp32"
