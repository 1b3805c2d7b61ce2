"""Device-side evaluation metrics: the counterpart of the per-frame loop in `Trainer.test`
(reference: src/main/runner.py:443-465).  The reference pulls every frame to the host and calls `.item()` three times
per frame; here one kernel reduces all frames of a batch and the host reads B x 4 floats once."""
import math
import struct

import torch

from . import lib as L


class DepthMetrics:
    """Accumulates MAE / RMSE / REL over frames exactly like Trainer.test: per-frame metrics, averaged over the frames
    that have at least one valid ground-truth pixel (frames without are skipped, runner.py:449-451)."""

    def __init__(self, max_depth=100.0, max_distance=100.0):
        self.max_depth, self.max_distance = float(max_depth), float(max_distance)
        self.rows = []          # device tensors [frames, 4], read on result()

    def update(self, pred, gt):
        """pred, gt: fp32 cuda tensors [B,1,H,W] (or [B,H,W]); normalised inverse... as produced by the model / dataloader."""
        if not pred.is_cuda:
            raise L.CrdError("DepthMetrics runs on the GPU (no CPU fallback; see oracle.losses.test_metrics for the CPU check)")
        pred = pred.detach().contiguous().float()
        gt = gt.detach().contiguous().float()
        frames = pred.shape[0]
        n = pred.numel() // frames
        acc = torch.zeros(frames, 4, dtype=L.SUM_DTYPE, device=pred.device)      # crd_sum_t (reproducible sums)
        L.check(L.load().crd_test_metrics(pred.data_ptr(), gt.data_ptr(), frames, n, self.max_depth, self.max_distance,
                                          acc.data_ptr(), L.stream()), "crd_test_metrics")
        self.rows.append(acc)

    def per_frame(self):
        a = L.stat_value(torch.cat(self.rows).cpu())
        out = []
        for sa, sq, sr, cnt in a.tolist():
            out.append(None if cnt == 0 else {"MAE": sa / cnt, "RMSE": math.sqrt(sq / cnt), "REL": sr / cnt})
        return out

    def result(self):
        ms = [m for m in self.per_frame() if m is not None]
        if not ms:
            return None
        return {k: sum(m[k] for m in ms) / len(ms) for k in ("MAE", "RMSE", "REL")}


class SegIoU:
    """The segmentation metric of Trainer.test (runner.py:432-436,508): per frame
    `JaccardIndex(num_classes, ignore_index=255)(pred_seg, gt_seg)` of torchmetrics 0.10.2 -- macro average over all
    num_classes classes of intersection / union from the confusion matrix of arg-max predictions, a class absent from both
    scoring 0 -- averaged over frames with np.nanmean.  Label 255 is NOT ignored by that call: ignore_index >= num_classes
    removes no class and torchmetrics raises ValueError on a target label >= num_classes, which the reference catches
    (runner.py:437-438), leaving that frame's IoU NaN.  One kernel builds the per-frame confusion matrices."""

    def __init__(self, num_classes=21):
        self.C = int(num_classes)
        self.mats, self.oor = [], []

    def update(self, logits, labels):
        """logits fp32 cuda [B,C,H,W], labels int64 cuda [B,H,W]."""
        if not logits.is_cuda:
            raise L.CrdError("SegIoU runs on the GPU (no CPU fallback; see oracle.losses.seg_iou for the CPU check)")
        logits = logits.detach().contiguous().float()
        labels = labels.detach().contiguous().to(torch.int64)
        B, C = logits.shape[0], logits.shape[1]
        assert C == self.C
        hw = logits.numel() // (B * C)
        mat = torch.zeros(B, C, C, dtype=torch.int64, device=logits.device)
        oor = torch.zeros(B, dtype=torch.int64, device=logits.device)
        L.check(L.load().crd_seg_confusion(logits.data_ptr(), labels.data_ptr(), B, C, hw, mat.data_ptr(), oor.data_ptr(), L.stream()),
                "crd_seg_confusion")
        self.mats.append(mat)
        self.oor.append(oor)

    def per_frame(self):
        mats, oor = torch.cat(self.mats).cpu().double(), torch.cat(self.oor).cpu()
        out = []
        for m, bad in zip(mats, oor.tolist()):
            if bad:
                out.append(float("nan"))
                continue
            inter = torch.diag(m)
            union = m.sum(0) + m.sum(1) - inter
            scores = torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(inter))
            out.append(float(scores.mean()))
        return out

    def result(self):
        """np.nanmean over the frames (NaN when every frame is NaN)."""
        vals = [v for v in self.per_frame() if not math.isnan(v)]
        return sum(vals) / len(vals) if vals else float("nan")


# ---------------------------------------------------------------------------------------------------------------------------
# The standard depth-evaluation suite (include/camradepth_hip.h: crd_depth_eval)
# ---------------------------------------------------------------------------------------------------------------------------
EVAL_COLUMNS = ("count", "sum_abs_e", "sum_e2", "sum_abs_e_over_dg", "sum_e2_over_dg", "sum_r", "sum_r2", "sum_abs_q", "sum_q2",
                "n_delta1", "n_delta2", "n_delta3")
EVAL_METRICS = ("MAE", "RMSE", "AbsRel", "SqRel", "RMSElog", "SILog", "iMAE", "iRMSE", "delta1", "delta2", "delta3")


def metrics_from_sums(sums12):
    """The metrics of one set of the twelve sums of crd_depth_eval, in float64 (no GPU needed).

    With dg the true distance and dp the predicted one in metres, e = dp - dg, r = log dp - log dg, q = 1/dp - 1/dg and
    m = max(dp/dg, dg/dp), sums12 = (n, S|e|, Se^2, S|e|/dg, Se^2/dg, Sr, Sr^2, S|q|, Sq^2, #(m < 1.25), #(m < 1.25^2), #(m < 1.25^3)):
        MAE = s1/n   RMSE = sqrt(s2/n)   AbsRel = s3/n   SqRel = s4/n   RMSElog = sqrt(s6/n)
        SILog = 100 sqrt(max(0, s6/n - (s5/n)^2))   iMAE = 1000 s7/n   iRMSE = 1000 sqrt(s8/n)  (1/km)   delta_k = s(8+k)/n
    Returns None when n == 0 (no valid pixel); NaN sums give NaN metrics."""
    s = [float(v) for v in sums12]
    if len(s) != 12:
        raise ValueError(f"metrics_from_sums: twelve sums expected, got {len(s)}")
    n = s[0]
    if n == 0:
        return None
    if math.isnan(n):
        return {k: float("nan") for k in EVAL_METRICS}
    mean_r = s[5] / n
    return {"MAE": s[1] / n, "RMSE": math.sqrt(s[2] / n), "AbsRel": s[3] / n, "SqRel": s[4] / n, "RMSElog": math.sqrt(s[6] / n),
            "SILog": 100.0 * math.sqrt(max(0.0, s[6] / n - mean_r * mean_r)), "iMAE": 1000.0 * s[7] / n,
            "iRMSE": 1000.0 * math.sqrt(s[8] / n), "delta1": s[9] / n, "delta2": s[10] / n, "delta3": s[11] / n}


def _f32(v):
    return struct.unpack("<f", struct.pack("<f", float(v)))[0]


def eval_bins(max_depth, bin_width):
    """ceil(max_depth / bin_width) with the fp32 division crd_depth_eval checks its n_bins against."""
    return int(math.ceil(_f32(_f32(max_depth) / _f32(bin_width))))


class DepthEval:
    """Threshold accuracies, AbsRel, SqRel, RMSE(log), SILog, iRMSE / iMAE, MAE and RMSE in METRES OF TRUE DISTANCE, at any number
    of distance caps, from one kernel per batch and one host read at the end.

    pred is the model's final depth and gt the dataloader's ground truth: fp32 [B,1,H,W] or [B,H,W], normalised inverted depth
    (gt = (max_depth - d) / max_depth for a lidar hit, 0 = no hit).  Per pixel, in fp32:
        dg = max_depth * (1 - gt)                                   valid: gt > 0 and dg >= min_depth
        dp = min(max(max_depth * (1 - clamp(pred, 0, 1)), min_depth), max_depth)
        bin = min(NB - 1, floor(dg / bin_width)),  NB = ceil(max_depth / bin_width)
    and per (frame, bin) the twelve sums of `metrics_from_sums` are kept.  A cap c (a multiple of bin_width, at most
    NB * bin_width) keeps the ground truth WITHIN c metres: the bins below c / bin_width are added per frame.  Results are the
    mean over the frames that have a valid pixel under the cap (as DepthMetrics), or `pooled` (sums added over frames first).
    min_depth defaults to KITTI's evaluation clamp of 1e-3 m.

    These are not Trainer.test's numbers: its REL divides by the inverted distance and its 50 m set keeps what lies BEYOND 50 m
    (DepthMetrics, faithful to the reference); AbsRel here divides by the true distance and a cap keeps what lies within it.
    The sums are order-independent fixed-point integers: two runs give the same bits, and frames gathered from other ranks are
    concatenated, not re-summed.  A non-finite or out-of-range term raises the library's sticky flag; the frames of the update()
    calls during which it was raised read NaN."""

    def __init__(self, max_depth=100.0, min_depth=1e-3, bin_width=10.0):
        self.max_depth, self.min_depth, self.bin_width = float(max_depth), float(min_depth), float(bin_width)
        for name in ("max_depth", "min_depth", "bin_width"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v > 0):
                raise L.CrdError(f"camradepth_amd.metrics.DepthEval: {name} = {v} must be finite and > 0")
        if not self.min_depth < self.max_depth:
            raise L.CrdError(f"camradepth_amd.metrics.DepthEval: min_depth = {self.min_depth} must be below max_depth = {self.max_depth}")
        self.n_bins = eval_bins(self.max_depth, self.bin_width)
        if self.n_bins > L.EVAL_MAX_BINS:
            raise L.CrdError(f"camradepth_amd.metrics.DepthEval: {self.n_bins} bins of {self.bin_width} m exceed {L.EVAL_MAX_BINS}")
        self._parts = []       # per update(): (acc int64 [B][NB][12], flag int32 [1]) on the device; per merge: a packed int64 [F][NB*12+1]
        self._host = None      # the packed rows on the host, read once

    # ------------------------------------------------------------------ accumulation
    def update(self, pred, gt):
        """One crd_depth_eval launch over the batch (plus the 64-thread capture of the non-finite flag); nothing is read back."""
        if not pred.is_cuda:
            raise L.CrdError("DepthEval runs on the GPU (no CPU fallback; metrics_from_sums does the arithmetic on sums you bring)")
        pred = pred.detach().contiguous().float()
        gt = gt.detach().contiguous().float()
        if pred.numel() != gt.numel() or pred.shape[0] != gt.shape[0]:
            raise L.CrdError(f"DepthEval.update: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
        frames = pred.shape[0]
        n = pred.numel() // frames
        acc = torch.zeros(frames, self.n_bins, 12, dtype=L.SUM_DTYPE, device=pred.device)
        flag = torch.zeros(1, dtype=torch.int32, device=pred.device)
        lib = L.load()
        L.check(lib.crd_depth_eval(pred.data_ptr(), gt.data_ptr(), frames, n, self.max_depth, self.min_depth, self.bin_width,
                                   self.n_bins, acc.data_ptr(), L.stream()), "crd_depth_eval")
        # the flag's device-side capture: this call's frames read NaN if a partial was dropped since the flag was last taken;
        # crd_nonfinite_status still reports it (the capture carries it over)
        L.check(lib.crd_nonfinite_capture(flag.data_ptr(), L.stream()), "crd_nonfinite_capture")
        self._parts.append((acc, flag))
        self._host = None

    def _packed(self, device=None):
        """int64 [F][NB*12 + 1]: the raw sums of every frame and, last, whether its update() dropped a partial."""
        rows = []
        for part in self._parts:
            if isinstance(part, tuple):
                acc, flag = part
                part = torch.cat([acc.reshape(acc.shape[0], -1), flag.to(torch.int64).expand(acc.shape[0], 1)], dim=1)
            rows.append(part if device is None else part.to(device))
        if not rows:
            return torch.zeros(0, self.n_bins * 12 + 1, dtype=torch.int64, device=device or "cpu")
        dev = rows[0].device
        return torch.cat([r.to(dev) for r in rows])

    def _rows(self):
        if self._host is None:
            self._host = self._packed().cpu().tolist()      # Python integers: adding bins or frames cannot overflow
        return self._host

    def merge(self, other):
        """Append the frames of another DepthEval with the same settings (frames are concatenated, never summed)."""
        if (other.max_depth, other.min_depth, other.bin_width) != (self.max_depth, self.min_depth, self.bin_width):
            raise L.CrdError("DepthEval.merge: the two evaluations differ in max_depth, min_depth or bin_width")
        self._parts.extend(other._parts)
        self._host = None
        return self

    def all_gather(self, group=None):
        """Every rank of the process group ends with the frames of all ranks, in rank order (so all ranks report the same
        numbers).  Ranks may hold different numbers of frames.  A collective call."""
        import torch.distributed as dist
        dev = torch.device("cuda", torch.cuda.current_device())
        mine = self._packed(dev)
        world = dist.get_world_size(group)
        counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(counts, torch.tensor([mine.shape[0]], dtype=torch.int64, device=dev), group=group)
        counts = [int(c) for c in counts]
        width = self.n_bins * 12 + 1
        padded = torch.zeros(max(counts + [1]), width, dtype=torch.int64, device=dev)
        padded[:mine.shape[0]] = mine
        bufs = [torch.empty_like(padded) for _ in range(world)]
        dist.all_gather(bufs, padded, group=group)
        self._parts = [b[:c].clone() for b, c in zip(bufs, counts) if c]
        self._host = None
        return self

    # ------------------------------------------------------------------ results
    def _bins_of(self, cap):
        if cap is None:
            return self.n_bins
        k = float(cap) / self.bin_width
        if not (abs(k - round(k)) < 1e-9 and 1 <= round(k) <= self.n_bins):
            raise L.CrdError(f"DepthEval: cap = {cap} must be a positive multiple of bin_width = {self.bin_width}, at most "
                             f"{self.n_bins * self.bin_width}")
        return int(round(k))

    @staticmethod
    def _value(ints, flagged):
        if flagged:
            return [float("nan")] * 12
        return [float(v) * 2.0 ** -bits for v, bits in zip(ints, L.EVAL_FRAC_BITS)]      # float(int) rounds to nearest

    def _frame_sums(self, row, lo, hi):
        """The twelve integer sums of bins lo..hi-1 of one packed row, and its flag."""
        out = [0] * 12
        for b in range(lo, hi):
            for c in range(12):
                out[c] += row[b * 12 + c]
        return out, bool(row[-1])

    def frames(self):
        return len(self._rows())

    def sums(self):
        """The raw sums as a float64 numpy array [frames][NB][12] (NaN rows where the non-finite flag was raised)."""
        import numpy as np
        rows = self._rows()
        out = np.zeros((len(rows), self.n_bins, 12), dtype=np.float64)
        for f, row in enumerate(rows):
            for b in range(self.n_bins):
                out[f, b] = self._value(row[b * 12:(b + 1) * 12], bool(row[-1]))
        return out

    def per_frame(self, cap=None):
        """One metrics dict per frame (None for a frame without a valid pixel within `cap` metres)."""
        k = self._bins_of(cap)
        return [metrics_from_sums(self._value(*self._frame_sums(row, 0, k))) for row in self._rows()]

    def _reduce(self, lo, hi, pooled):
        if pooled:
            tot, bad = [0] * 12, False
            for row in self._rows():
                s, flagged = self._frame_sums(row, lo, hi)
                tot = [a + b for a, b in zip(tot, s)]
                bad = bad or flagged
            return metrics_from_sums(self._value(tot, bad))
        ms = [metrics_from_sums(self._value(*self._frame_sums(row, lo, hi))) for row in self._rows()]
        ms = [m for m in ms if m is not None]
        if not ms:
            return None
        return {k: sum(m[k] for m in ms) / len(ms) for k in EVAL_METRICS}

    def result(self, cap=None, pooled=False):
        """The mean over the frames that have a valid pixel within `cap` metres, or (pooled) the metrics of the sums added over
        all frames; None when no frame has one."""
        return self._reduce(0, self._bins_of(cap), pooled)

    def by_range(self, pooled=True):
        """One entry per distance bin: {"lo": metres, "hi": metres, "metrics": dict or None}."""
        return [{"lo": b * self.bin_width, "hi": min((b + 1) * self.bin_width, self.max_depth), "metrics": self._reduce(b, b + 1, pooled)}
                for b in range(self.n_bins)]
