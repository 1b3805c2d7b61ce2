"""float64 numpy restatement of the definitions of crd_depth_eval (include/camradepth_hip.h), shared by test_depth_eval_cpu.py
and test_gpu_depth_eval.py.  What the definition fixes in fp32 stays fp32 here -- the distances dg and dp with their clamps, the
bin index and the threshold ratio m, so that counts and delta columns can be compared exactly -- and everything summed is float64
arithmetic on those fp32 distances."""
import numpy as np

F = np.float32


def distances(pred, gt, max_depth=100.0, min_depth=1e-3):
    """-> dg, dp (fp32, shaped as the inputs) and the valid mask."""
    pred, gt = np.asarray(pred, dtype=F), np.asarray(gt, dtype=F)
    md, lo = F(max_depth), F(min_depth)
    with np.errstate(invalid="ignore"):
        dg = md * (F(1.0) - gt)
        valid = (gt > 0) & (dg >= lo)
        pc = np.where(pred < 0, F(0), np.where(pred > 1, F(1), pred)).astype(F)         # NaN stays NaN
        dr = (md * (F(1.0) - pc)).astype(F)
        dp = np.where(dr < lo, lo, np.where(dr > md, md, dr)).astype(F)
    return dg.astype(F), dp, valid


def n_bins(max_depth, bin_width):
    return int(np.ceil(F(max_depth) / F(bin_width)))


def bin_index(dg, max_depth, bin_width):
    nb = n_bins(max_depth, bin_width)
    return np.minimum(nb - 1, np.floor(dg / F(bin_width)).astype(np.int64))


def frame_sums(pred, gt, max_depth=100.0, min_depth=1e-3, bin_width=10.0):
    """One frame -> float64 [NB][12]."""
    nb = n_bins(max_depth, bin_width)
    dg, dp, valid = distances(np.ravel(pred), np.ravel(gt), max_depth, min_depth)
    dg, dp = dg[valid], dp[valid]
    b = bin_index(dg, max_depth, bin_width)
    m = np.maximum(dp / dg, dg / dp)                            # fp32, as defined
    g, p = dg.astype(np.float64), dp.astype(np.float64)
    e, r, q = p - g, np.log(p) - np.log(g), 1.0 / p - 1.0 / g
    terms = [np.ones_like(g), np.abs(e), e * e, np.abs(e) / g, e * e / g, r, r * r, np.abs(q), q * q,
             (m < F(1.25)).astype(np.float64), (m < F(1.5625)).astype(np.float64), (m < F(1.953125)).astype(np.float64)]
    out = np.zeros((nb, 12), dtype=np.float64)
    for c, t in enumerate(terms):
        out[:, c] = np.bincount(b, weights=t, minlength=nb)
    return out


def batch_sums(pred, gt, max_depth=100.0, min_depth=1e-3, bin_width=10.0):
    """-> float64 [frames][NB][12]."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    return np.stack([frame_sums(pred[f], gt[f], max_depth, min_depth, bin_width) for f in range(pred.shape[0])])


def metrics(s):
    """The metrics of twelve float64 sums, written out independently of camradepth_amd.metrics.metrics_from_sums."""
    s = np.asarray(s, dtype=np.float64)
    n = s[0]
    if n == 0:
        return None
    return {"MAE": s[1] / n, "RMSE": np.sqrt(s[2] / n), "AbsRel": s[3] / n, "SqRel": s[4] / n, "RMSElog": np.sqrt(s[6] / n),
            "SILog": 100.0 * np.sqrt(max(0.0, s[6] / n - (s[5] / n) ** 2)), "iMAE": 1000.0 * s[7] / n,
            "iRMSE": 1000.0 * np.sqrt(s[8] / n), "delta1": s[9] / n, "delta2": s[10] / n, "delta3": s[11] / n}


def cap_sums(sums_f, cap, bin_width=10.0):
    """Twelve sums of one frame [NB][12] over the bins below cap / bin_width."""
    return sums_f[:int(round(cap / bin_width))].sum(axis=0)
