"""HIP implementations of the CamRaDepth loss callables (same class names and call signature as
src/utils/loss_funcs.py:14-91,118-180).  Each loss is one masked-reduction kernel plus an analytic
backward kernel (BerHu and the smoothness loss: two of each); no boolean-mask gather.

Under data parallelism the reference computes every masked mean over the GATHERED global batch
(nn.DataParallel gathers outputs on device 0, src/main/runner.py:136,197-203).  To reproduce that
exactly with one process per GPU the (sum, count) partials are all-reduced before they are used,
so the value is the global loss and the local gradient is already divided by the global count
(gradients are then SUM-reduced across ranks, see parallel.GradSync).
"""
import collections
import math

import torch
import torch.distributed as dist
import torch.nn as nn

from . import lib as L


def _allreduce_acc(acc):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(acc)


def _allreduce_max(t):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)


def berhu_value(s1, s2, count, max_abs, thresh):
    """MaskedBerHuLoss from crd_masked_berhu's sums: (sum part1 + sum part2-numerators / (2c)) / count, c = thresh * max |d|
    (the reference's delta, a float64 constant taken with .item()).  NaN when c = 0 or the mask is empty, as the reference's
    division by 2c is (its torch.max raises on an empty mask instead)."""
    c = thresh * max_abs
    return (s1 + s2 / (2.0 * c)) / count


def _launch(lb, entry, *args):
    L.check(getattr(lb, entry)(*args, L.stream()), entry)


def _addr(t):
    return None if t is None else t.data_ptr()


# The trainable depth criteria, one record per mode: what the loss modules below and the captured step (trainer.TrainStep) launch, and
# how the value comes from the sums.  pair = (pred, target, n); every pointer is an address or None.
#   partials(lb, pair, acc, maxbits)      the forward launch into the 4-slot crd_sum_t block acc = (sum, count, sum d^2, -);
#                                         two_phase: (-, count, sum d^2, -) and the fp32 bits of max |d| in maxbits
#   grad(lb, pair, acc, maxbits, thresh, loss, gout, gmul, d)
#                                         the backward launch: d = gmul * gout[0] (1 if None) * dvalue / dpred; two_phase: with it, or with
#                                         d = None instead of it, the two loss sums into `loss`
#   value(a, s, max_abs, thresh)          the criterion from the float64 values a of the block (two_phase: s of the loss sums, max |d|)
#   two_phase                             BerHu: c = thresh * max |d| over ALL ranks comes first; one entry (phase b) then computes the
#                                         loss sums and the gradient
Criterion = collections.namedtuple("Criterion", "partials grad value two_phase", defaults=(False,))


def _dist(mode, value):      # crd_masked_dist_*: mode 0 L1, mode 1 RMSE
    return Criterion(lambda lb, pair, acc, mx: _launch(lb, "crd_masked_dist_fwd", *pair, acc),
                     lambda lb, pair, acc, mx, thresh, loss, gout, gmul, d: _launch(lb, "crd_masked_dist_bwd", *pair, acc, gout, gmul, mode, d),
                     value)


CRITERIA = {
    "smooth_l1": Criterion(lambda lb, pair, acc, mx: _launch(lb, "crd_masked_l1_fwd", *pair, acc),
                           lambda lb, pair, acc, mx, thresh, loss, gout, gmul, d: _launch(lb, "crd_masked_l1_bwd", *pair, acc, gout, gmul, d),
                           lambda a, s, max_abs, thresh: a[0] / a[1]),
    "l1": _dist(0, lambda a, s, max_abs, thresh: a[0] / a[1]),
    "rmse": _dist(1, lambda a, s, max_abs, thresh: torch.sqrt(a[2] / a[1])),
    "berhu": Criterion(lambda lb, pair, acc, mx: _launch(lb, "crd_masked_berhu_max", *pair, acc, mx),
                       lambda lb, pair, acc, mx, thresh, loss, gout, gmul, d: _launch(lb, "crd_masked_berhu", *pair, acc, mx, L.f64_bits(thresh),
                                                                                      loss, gout, gmul, d),
                       lambda a, s, max_abs, thresh: berhu_value(s[0], s[1], a[1], max_abs, thresh), two_phase=True),
}


class _MaskedDepth(torch.autograd.Function):
    """One criterion of CRITERIA on a (pred, target) pair.  Two-phase (BerHu): phase (a) max |d|, count, sum d^2; the ranks' partials
    are reduced (SUM, max: MAX); phase (b) the loss sums with the global c; the backward re-runs phase (b) for the gradient only.
    metric: value(a) of a detached metric on the criterion's partials, which has no backward (MaskedMSELoss)."""

    @staticmethod
    def forward(ctx, pred, target, mode, thresh=None, metric=None):
        lb, crit, dev = L.load(), CRITERIA[mode], pred.device
        pred_c, target_c = pred.contiguous().float(), target.contiguous().float()
        pair = pred_c.data_ptr(), target_c.data_ptr(), pred_c.numel()
        acc = torch.zeros(4, dtype=L.SUM_DTYPE, device=dev)     # crd_sum_t: order-independent, exact under all-reduce
        mx = torch.zeros(1, dtype=torch.int32, device=dev) if crit.two_phase else None      # (non-negative floats order as ints)
        crit.partials(lb, pair, acc.data_ptr(), _addr(mx))
        _allreduce_acc(acc)
        s = max_abs = None
        if crit.two_phase:
            _allreduce_max(mx)
            ls = torch.zeros(2, dtype=L.SUM_DTYPE, device=dev)
            crit.grad(lb, pair, acc.data_ptr(), mx.data_ptr(), thresh, ls.data_ptr(), None, 0.0, None)
            _allreduce_acc(ls)
            s, max_abs = L.stat_value(ls), mx.view(torch.float32)[0].double()
        ctx.save_for_backward(pred_c, target_c, acc, mx)
        ctx.mode, ctx.thresh, ctx.metric = mode, thresh, metric is not None
        a = L.stat_checked(acc)              # NaN when a non-finite partial was dropped (the reference's float sums report it)
        return (metric(a) if metric else crit.value(a, s, max_abs, thresh)).float()

    @staticmethod
    def backward(ctx, gout):
        pred, target, acc, mx = ctx.saved_tensors
        if ctx.metric:
            raise NotImplementedError("MaskedMSELoss is a metric in the reference (runner.py:208); no backward")
        d = torch.empty_like(pred)
        g = gout.contiguous().float()
        CRITERIA[ctx.mode].grad(L.load(), (pred.data_ptr(), target.data_ptr(), pred.numel()), acc.data_ptr(), _addr(mx), ctx.thresh, None,
                                g.data_ptr(), 1.0, d.data_ptr())
        return d, None, None, None, None


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


class DepthCriterion(nn.Module):
    """A depth criterion that trains: `mode` names its record in CRITERIA.  trainer.depth_criterion_mode accepts exactly the
    subclasses of this class."""
    mode = None

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        return _MaskedDepth.apply(pred, target, self.mode)


class MaskedSmoothL1Loss(DepthCriterion):
    """SmoothL1(beta=1) mean over target > 0 (reference: src/utils/loss_funcs.py:77-91)."""
    mode = "smooth_l1"


class MaskedMSELoss(nn.Module):
    """mean((target-pred)^2) over target > 0 (reference: src/utils/loss_funcs.py:36-46): a detached metric on smooth-L1's partials."""

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        self.loss = _MaskedDepth.apply(pred.detach(), target, "smooth_l1", None, lambda a: a[2] / a[1])
        return self.loss


class MaskedL1Loss(DepthCriterion):
    """mean |target - pred| over target > 0 (reference: src/utils/loss_funcs.py:49-59)."""
    mode = "l1"

    def forward(self, pred, target):
        self.loss = super().forward(pred, target)
        return self.loss


class MaskedHuberLoss(DepthCriterion):
    """nn.HuberLoss() (delta = 1) mean over target > 0 (reference: src/utils/loss_funcs.py:61-75).  Huber with delta = 1 is
    smooth-L1 with beta = 1 term for term, so this runs the MaskedSmoothL1Loss kernels."""
    mode = "smooth_l1"


class MaskedRMSELoss(DepthCriterion):
    """sqrt(mean (target - pred)^2) over target > 0 (reference: src/utils/loss_funcs.py:118-128)."""
    mode = "rmse"

    def forward(self, pred, target):
        self.loss = super().forward(pred, target)
        return self.loss


class MaskedBerHuLoss(DepthCriterion):
    """Reverse Huber over target > 0 with c = thresh * max |target - pred| (reference: src/utils/loss_funcs.py:130-155): |d| below
    c, d^2 / (2c) above it, nothing at |d| == c; c is a constant of the backward.  An empty mask gives a NaN loss and a zero
    gradient (the reference's torch.max raises there)."""
    mode = "berhu"

    def __init__(self, thresh=0.2):
        super().__init__()
        self.thresh = thresh

    def forward(self, pred, target):
        assert pred.dim() == target.dim(), "inconsistent dimensions"
        if not (float(self.thresh) > 0.0 and math.isfinite(float(self.thresh))):
            raise L.CrdError(f"MaskedBerHuLoss: thresh must be a finite number > 0, got {self.thresh!r}")
        return _MaskedDepth.apply(pred, target, self.mode, float(self.thresh))


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
