"""HIP implementations of the CamRaDepth loss callables (same class names and call signature as
src/utils/loss_funcs.py:14-91,118-180).  Each loss is one masked-reduction kernel plus an analytic
backward kernel (BerHu and the smoothness loss: two of each); no boolean-mask gather.

Under data parallelism the reference computes every masked mean over the GATHERED global batch
(nn.DataParallel gathers outputs on device 0, src/main/runner.py:136,197-203).  To reproduce that
exactly with one process per GPU the (sum, count) partials are all-reduced before they are used,
so the value is the global loss and the local gradient is already divided by the global count
(gradients are then SUM-reduced across ranks, see parallel.GradSync).
"""
import math

import torch
import torch.distributed as dist
import torch.nn as nn

from . import lib as L


def _allreduce_acc(acc):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(acc)


class _MaskedL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mode):
        lb = L.load()
        pred_c, target_c = pred.contiguous().float(), target.contiguous().float()
        acc = torch.zeros(4, dtype=L.SUM_DTYPE, device=pred.device)     # crd_sum_t: order-independent, exact under all-reduce
        L.check(lb.crd_masked_l1_fwd(pred_c.data_ptr(), target_c.data_ptr(), pred_c.numel(), acc.data_ptr(), L.stream()),
                "crd_masked_l1_fwd")
        _allreduce_acc(acc)
        ctx.save_for_backward(pred_c, target_c, acc)
        ctx.mode = mode
        a = L.stat_checked(acc)              # NaN when a non-finite partial was dropped (the reference's float sums report it)
        return ((a[0] if mode == "smooth_l1" else a[2]) / a[1]).float()

    @staticmethod
    def backward(ctx, gout):
        pred, target, acc = ctx.saved_tensors
        if ctx.mode != "smooth_l1":
            raise NotImplementedError("MaskedMSELoss is a metric in the reference (runner.py:208); no backward")
        lb = L.load()
        d = torch.empty_like(pred)
        g = gout.contiguous().float()
        L.check(lb.crd_masked_l1_bwd(pred.data_ptr(), target.data_ptr(), pred.numel(), acc.data_ptr(), g.data_ptr(), 1.0,
                                     d.data_ptr(), L.stream()), "crd_masked_l1_bwd")
        return d, None, None


class MaskedSmoothL1Loss(nn.Module):
    """SmoothL1(beta=1) mean over target > 0 (reference: src/utils/loss_funcs.py:77-91)."""

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        return _MaskedL1.apply(pred, target, "smooth_l1")


class MaskedMSELoss(nn.Module):
    """mean((target-pred)^2) over target > 0 (reference: src/utils/loss_funcs.py:36-46)."""

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        self.loss = _MaskedL1.apply(pred.detach(), target, "mse")
        return self.loss


def _allreduce_max(t):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)


class _MaskedDist(torch.autograd.Function):
    """MaskedL1Loss (mode 0) / MaskedRMSELoss (mode 1): one pass for sum |d|, count and sum d^2 (crd_masked_dist_fwd)."""

    @staticmethod
    def forward(ctx, pred, target, mode):
        lb = L.load()
        pred_c, target_c = pred.contiguous().float(), target.contiguous().float()
        acc = torch.zeros(4, dtype=L.SUM_DTYPE, device=pred.device)
        L.check(lb.crd_masked_dist_fwd(pred_c.data_ptr(), target_c.data_ptr(), pred_c.numel(), acc.data_ptr(), L.stream()),
                "crd_masked_dist_fwd")
        _allreduce_acc(acc)
        ctx.save_for_backward(pred_c, target_c, acc)
        ctx.mode = mode
        a = L.stat_checked(acc)
        return (a[0] / a[1] if mode == 0 else torch.sqrt(a[2] / a[1])).float()

    @staticmethod
    def backward(ctx, gout):
        pred, target, acc = ctx.saved_tensors
        d = torch.empty_like(pred)
        g = gout.contiguous().float()
        L.check(L.load().crd_masked_dist_bwd(pred.data_ptr(), target.data_ptr(), pred.numel(), acc.data_ptr(), g.data_ptr(), 1.0,
                                             ctx.mode, d.data_ptr(), L.stream()), "crd_masked_dist_bwd")
        return d, None, None


def berhu_value(s1, s2, count, max_abs, thresh):
    """MaskedBerHuLoss from crd_masked_berhu's sums: (sum part1 + sum part2-numerators / (2c)) / count, c = thresh * max |d|
    (the reference's delta, a float64 constant taken with .item()).  NaN when c = 0 or the mask is empty, as the reference's
    division by 2c is (its torch.max raises on an empty mask instead)."""
    c = thresh * max_abs
    return (s1 + s2 / (2.0 * c)) / count


class _BerHu(torch.autograd.Function):
    """Phase (a) max |d|, count, sum d^2; the ranks' partials are reduced (SUM, max: MAX); phase (b) the loss sums with the
    global c; the backward re-runs phase (b) for the gradient only."""

    @staticmethod
    def forward(ctx, pred, target, thresh):
        lb = L.load()
        pred_c, target_c = pred.contiguous().float(), target.contiguous().float()
        acc = torch.zeros(4, dtype=L.SUM_DTYPE, device=pred.device)
        mx = torch.zeros(1, dtype=torch.int32, device=pred.device)      # fp32 bit pattern of max |d| (non-negative: orders as an int)
        L.check(lb.crd_masked_berhu_max(pred_c.data_ptr(), target_c.data_ptr(), pred_c.numel(), acc.data_ptr(), mx.data_ptr(),
                                        L.stream()), "crd_masked_berhu_max")
        _allreduce_acc(acc)
        _allreduce_max(mx)
        ls = torch.zeros(2, dtype=L.SUM_DTYPE, device=pred.device)
        L.check(lb.crd_masked_berhu(pred_c.data_ptr(), target_c.data_ptr(), pred_c.numel(), acc.data_ptr(), mx.data_ptr(),
                                    L.f64_bits(thresh), ls.data_ptr(), None, 0.0, None, L.stream()), "crd_masked_berhu")
        _allreduce_acc(ls)
        ctx.save_for_backward(pred_c, target_c, acc, mx)
        ctx.thresh = thresh
        a, s = L.stat_checked(acc), L.stat_value(ls)
        return berhu_value(s[0], s[1], a[1], mx.view(torch.float32)[0].double(), thresh).float()

    @staticmethod
    def backward(ctx, gout):
        pred, target, acc, mx = ctx.saved_tensors
        d = torch.empty_like(pred)
        g = gout.contiguous().float()
        L.check(L.load().crd_masked_berhu(pred.data_ptr(), target.data_ptr(), pred.numel(), acc.data_ptr(), mx.data_ptr(),
                                          L.f64_bits(ctx.thresh), None, g.data_ptr(), 1.0, d.data_ptr(), L.stream()), "crd_masked_berhu")
        return d, None, None


class _Smoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, image):
        lb = L.load()
        p, im = pred.contiguous().float(), image.contiguous().float()
        B, C, H, W = im.shape
        acc = torch.zeros((B, 3), dtype=L.SUM_DTYPE, device=p.device)     # per sample: sum p, x-term sum, y-term sum
        L.check(lb.crd_smoothness_fwd(p.data_ptr(), im.data_ptr(), B, C, H, W, acc.data_ptr(), L.stream()), "crd_smoothness_fwd")
        # the gathered batch's means: sum the terms and the batch size (in the same fixed point) over the ranks; the per-sample
        # means stay local.  The backward's denominators become the gathered batch's through its gradient scale, local B / global B.
        tot = torch.cat([acc[:, 1:].sum(0), torch.full((1,), B << L.STAT_FRAC_BITS, dtype=L.SUM_DTYPE, device=p.device)])
        _allreduce_acc(tot)
        gscale = (B / L.stat_value(tot[2:])).float()
        ctx.save_for_backward(p, im, acc, gscale)
        t = L.stat_checked(tot)                  # (the one host wait, as in the other loss modules)
        return (t[0] / (t[2] * H * (W - 1)) + t[1] / (t[2] * (H - 1) * W)).float()

    @staticmethod
    def backward(ctx, gout):
        p, im, acc, gscale = ctx.saved_tensors
        B, C, H, W = im.shape
        d = torch.empty_like(p)
        g = (gout.float() * gscale).contiguous()
        L.check(L.load().crd_smoothness_bwd(p.data_ptr(), im.data_ptr(), B, C, H, W, acc.data_ptr(), g.data_ptr(), 1.0,
                                            d.data_ptr(), L.stream()), "crd_smoothness_bwd")
        return d, None


class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        lb = L.load()
        lg = logits.contiguous().float()
        tg = target.contiguous().to(torch.int64)
        B, Cc = lg.shape[0], lg.shape[1]
        HW = lg.numel() // (B * Cc)
        acc = torch.zeros(4, dtype=L.SUM_DTYPE, device=lg.device)
        L.check(lb.crd_ce_fwd(lg.data_ptr(), tg.data_ptr(), B, Cc, HW, acc.data_ptr(), L.stream()), "crd_ce_fwd")
        _allreduce_acc(acc)
        ctx.save_for_backward(lg, tg, acc)
        a = L.stat_checked(acc)
        n_bad = int(acc[2]) >> L.STAT_FRAC_BITS      # (the sums are on their way to the host already: no further wait)
        if n_bad:
            raise L.CrdError(f"MaskedFocalLoss: {n_bad} target label(s) are neither in [0, {Cc}) nor ignore_index 255 "
                             "(torch.nn.functional.cross_entropy raises on them)")
        ce = (a[0] / a[1]).float()
        pt = torch.exp(-ce)
        return (1 - pt) ** 2 * ce

    @staticmethod
    def backward(ctx, gout):
        lg, tg, acc = ctx.saved_tensors
        lb = L.load()
        B, Cc = lg.shape[0], lg.shape[1]
        HW = lg.numel() // (B * Cc)
        d = torch.empty_like(lg)
        g = gout.contiguous().float()
        L.check(lb.crd_ce_focal_bwd(lg.data_ptr(), tg.data_ptr(), B, Cc, HW, acc.data_ptr(), g.data_ptr(), 1.0, d.data_ptr(),
                                    L.stream()), "crd_ce_focal_bwd")
        return d, None


class MaskedL1Loss(nn.Module):
    """mean |target - pred| over target > 0 (reference: src/utils/loss_funcs.py:49-59)."""

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        self.loss = _MaskedDist.apply(pred, target, 0)
        return self.loss


class MaskedHuberLoss(nn.Module):
    """nn.HuberLoss() (delta = 1) mean over target > 0 (reference: src/utils/loss_funcs.py:61-75).  Huber with delta = 1 is
    smooth-L1 with beta = 1 term for term, so this runs the MaskedSmoothL1Loss kernels."""

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        return _MaskedL1.apply(pred, target, "smooth_l1")


class MaskedRMSELoss(nn.Module):
    """sqrt(mean (target - pred)^2) over target > 0 (reference: src/utils/loss_funcs.py:118-128)."""

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        self.loss = _MaskedDist.apply(pred, target, 1)
        return self.loss


class MaskedBerHuLoss(nn.Module):
    """Reverse Huber over target > 0 with c = thresh * max |target - pred| (reference: src/utils/loss_funcs.py:130-155): |d| below
    c, d^2 / (2c) above it, nothing at |d| == c; c is a constant of the backward.  An empty mask gives a NaN loss and a zero
    gradient (the reference's torch.max raises there)."""

    def __init__(self, thresh=0.2):
        super().__init__()
        self.thresh = thresh

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        if not (float(self.thresh) > 0.0 and math.isfinite(float(self.thresh))):
            raise L.CrdError(f"MaskedBerHuLoss: thresh must be a finite number > 0, got {self.thresh!r}")
        return _BerHu.apply(pred, target, float(self.thresh))


class SmoothnessLoss(nn.Module):
    """Edge-aware smoothness of pred_depth / (per-sample mean + 1e-7) weighted by exp(-mean_c |image gradient|)
    (reference: src/utils/loss_funcs.py:157-180).  pred_depth [B, 1, H, W], image [B, C, H, W]; the image gets no gradient."""

    def forward(self, pred_depth, image):
        if pred_depth.dim() != 4 or pred_depth.shape[1] != 1:
            raise L.CrdError(f"SmoothnessLoss: pred_depth must be [B, 1, H, W], got {tuple(pred_depth.shape)}")
        if image.dim() != 4 or image.shape[0] != pred_depth.shape[0] or image.shape[2:] != pred_depth.shape[2:]:
            raise L.CrdError(f"SmoothnessLoss: image {tuple(image.shape)} does not match pred_depth {tuple(pred_depth.shape)}")
        return _Smoothness.apply(pred_depth, image.detach())


class MaskedFocalLoss(nn.Module):
    """Focal transform (gamma=2) of the scalar mean cross entropy, ignore_index=255
    (reference: src/utils/loss_funcs.py:14-34).  A target label that is neither 255 nor a class raises CrdError naming how many
    there are (torch raises there too); the kernels never read through such a label."""

    def __init__(self, weight=None, gamma=2, reduction="mean"):
        super().__init__()
        assert gamma == 2 and weight is None, "only the reference's configuration (gamma=2, no class weights) is implemented"
        self.gamma, self.reduction = gamma, reduction

    def forward(self, inputs, target):
        return _Focal.apply(inputs, target)


def total_loss(out, batch, supervised_seg, update_interval=1, criterion=None):
    """Loss combination of Trainer.train_one_epoch (reference: src/main/runner.py:197-218)."""
    crit = criterion or {"depth": MaskedSmoothL1Loss(), "seg": MaskedFocalLoss()}
    final, inter, seg = out["depth"]["final_depth"], out["depth"]["intermediate_depths"], out["seg"]["final_seg"]
    l_seg = (crit["seg"](seg, batch["seg"]) if seg is not None else 0) * (1 if supervised_seg else 0)
    l_half = crit["depth"](inter[-1].squeeze(1), batch["gt_half"].squeeze(1))
    l_quarter = crit["depth"](inter[-2].squeeze(1), batch["gt_quarter"].squeeze(1))
    l_full = crit["depth"](final, batch["gt_full"])
    w = [1, 1, 1, 0.2, 0.2]
    loss = (w[0] * l_full + w[1] * l_half + w[2] * l_quarter + w[3] * l_seg + w[4] * 0) / sum(w)
    return loss / update_interval, {"full": l_full, "half": l_half, "quarter": l_quarter, "seg": l_seg}
