"""float64 numpy restatement of the segmentation criterion and metrics (include/camradepth_hip.h: crd_ce_fwd, crd_ce_focal_bwd,
crd_seg_argmax, crd_seg_confusion), shared by test_seg_loss_ref_cpu.py and test_gpu_seg_loss.py.  The inputs are the float32
logits exactly as the kernels see them; everything computed from them is float64.

Labels: 255 is ignore_index (no loss, no gradient, not counted).  Any other label outside [0, C) is OUT OF RANGE: torch raises on
it; here it is skipped like an ignored pixel and counted, so that the caller can raise."""
import numpy as np

IGNORE = 255


def _f64(logits):
    return np.asarray(logits, dtype=np.float32).astype(np.float64)


def label_masks(labels, C):
    """-> (valid, out_of_range) boolean masks shaped as labels."""
    labels = np.asarray(labels, dtype=np.int64)
    ignored = labels == IGNORE
    oor = ~ignored & ((labels < 0) | (labels >= C))
    return ~ignored & ~oor, oor


def log_softmax(logits):
    """Over axis 1 of [B, C, HW], log-sum-exp with the maximum subtracted.  A -inf logit gives -inf (probability 0)."""
    x = _f64(logits)
    mx = x.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (x - mx) - np.log(np.exp(x - mx).sum(axis=1, keepdims=True))


def ce_terms(logits, labels, C):
    """-> (ce [B, HW] float64: -log softmax[label] on the valid pixels and 0 elsewhere, valid, out_of_range)."""
    labels = np.asarray(labels, dtype=np.int64)
    valid, oor = label_masks(labels, C)
    ls = log_softmax(logits)
    safe = np.where(valid, labels, 0)                       # never index with a label that is not a class
    picked = np.take_along_axis(ls, safe[:, None, :], axis=1)[:, 0, :]
    return np.where(valid, -picked, 0.0), valid, oor


def ce_sums(logits, labels, C):
    """-> (sum of the cross entropy over the valid pixels, their count, the number of out-of-range labels)."""
    ce, valid, oor = ce_terms(logits, labels, C)
    return float(ce.sum()), int(valid.sum()), int(oor.sum())


def focal(sum_ce, count):
    """(1 - exp(-ce))^2 ce of the scalar mean ce = sum / count; NaN when nothing is valid (0 / 0, as torch's mean)."""
    if count == 0:
        return float("nan")
    ce = float(sum_ce) / float(count)
    return (1.0 - np.exp(-ce)) ** 2 * ce


def focal_dce(ce):
    """dF/dce = 2 (1 - pt) pt ce + (1 - pt)^2 with pt = exp(-ce)."""
    pt = np.exp(-ce)
    return 2.0 * (1.0 - pt) * pt * ce + (1.0 - pt) ** 2


def focal_grad(logits, labels, C, g=1.0):
    """dlogits [B, C, HW] float64 of g * focal: g dF/dce / count (softmax - onehot) on the valid pixels, 0 on ignored and
    out-of-range ones (all zero when nothing is valid, as torch's backward of the NaN mean)."""
    labels = np.asarray(labels, dtype=np.int64)
    ce, valid, _ = ce_terms(logits, labels, C)
    count = int(valid.sum())
    out = np.zeros(np.shape(logits), dtype=np.float64)
    if count == 0:
        return out
    scale = float(g) * focal_dce(ce.sum() / count) / count
    d = np.exp(log_softmax(logits))
    onehot = (np.arange(C)[None, :, None] == np.where(valid, labels, -1)[:, None, :])
    d = scale * (d - onehot)
    return np.where(valid[:, None, :], d, 0.0)


def argmax_first(logits, axis):
    """Index of the FIRST maximal entry along axis (written out: not np.argmax)."""
    x = _f64(logits)
    n = x.shape[axis]
    shape = [1] * x.ndim
    shape[axis] = n
    idx = np.arange(n).reshape(shape)
    return np.where(x == x.max(axis=axis, keepdims=True), idx, n).min(axis=axis)


def confusion(logits, labels, C):
    """One frame: logits [C, HW], labels [HW] -> (mat int64 [C, C] with mat[target][prediction], number of labels outside [0, C)).
    Label 255 is NOT ignored here (torchmetrics' JaccardIndex raises on it as on any label >= C): it counts as out of range."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    pred = argmax_first(np.asarray(logits).reshape(C, -1), 0)
    ok = (labels >= 0) & (labels < C)
    mat = np.bincount(labels[ok] * C + pred[ok], minlength=C * C).reshape(C, C).astype(np.int64)
    return mat, int((~ok).sum())
