"""CPU: the surface of the standard depth-evaluation suite -- crd_depth_eval in the header and the binding, its argument checks
(refused before any launch, so no GPU is needed), metrics_from_sums against a float64 numpy restatement, Trainer.test's keywords."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import depth_eval_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def _header():
    return open(os.path.join(REPO, "include", "camradepth_hip.h")).read()


def test_header_declares_crd_depth_eval_and_the_binding_knows_it(built):
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+crd_depth_eval\s*\((.*?)\)\s*;", h, flags=re.S)
    assert m, "crd_depth_eval is not declared in include/camradepth_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0] == "const float* pred" and args[1] == "const float* gt" and "crd_sum_t* acc" in args[8]
    assert built._SIGS["crd_depth_eval"] == "ppilfffipp"
    assert hasattr(built.load(), "crd_depth_eval")
    assert built.ABI_VERSION == int(re.search(r"#define\s+CRD_ABI_VERSION\s+(\d+)", h).group(1)) >= 11


def test_fraction_bit_table_of_the_header_equals_the_binding(built):
    h = _header()
    m = re.search(r"CRD_EVAL_FRAC_BITS\[CRD_EVAL_COLUMNS\]\s*=\s*\{([^}]*)\}", h)
    assert m, "CRD_EVAL_FRAC_BITS table not found in the header"
    bits = tuple(int(v) for v in m.group(1).split(","))
    assert int(re.search(r"#define\s+CRD_EVAL_COLUMNS\s+(\d+)", h).group(1)) == 12 == len(bits)
    assert bits == tuple(built.EVAL_FRAC_BITS)
    assert [bits[c] for c in (0, 9, 10, 11)] == [0, 0, 0, 0]                      # the counts are integers
    assert all(0 < b < 62 for c, b in enumerate(bits) if c not in (0, 9, 10, 11))
    assert int(re.search(r"#define\s+CRD_EVAL_MAX_BINS\s+(\d+)", h).group(1)) == built.EVAL_MAX_BINS
    # the ranges stated next to the table: 928 x 1600 all-valid pixels of the largest per-pixel term at the default min_depth
    # (dg, dp in [1e-3, 100]) fit below 2^63 in columns 0-3, 5-7 and 9-11
    npix, ln = 928 * 1600, float(np.log(1e5))
    worst = {0: 1, 1: 100.0, 2: 1e4, 3: 1e5, 5: ln, 6: ln * ln, 7: 1e3, 9: 1, 10: 1, 11: 1}
    for c, w in worst.items():
        assert npix * w * 2.0 ** bits[c] < 2.0 ** 63, c
        assert w * 2.0 ** bits[c] < 2.0 ** 62, c                                  # and no single term is refused


def test_invalid_arguments_are_refused_before_any_launch(built):
    L = built.load()
    buf = ctypes.create_string_buffer(64)          # any non-NULL host address: a refused call launches nothing and reads none of it
    a = ctypes.addressof(buf)
    good = dict(pred=a, gt=a, frames=1, n=16, max_depth=100.0, min_depth=1e-3, bin_width=10.0, n_bins=10, acc=a)

    def refused(word, **kw):
        k = dict(good, **kw)
        rc = L.crd_depth_eval(k["pred"], k["gt"], k["frames"], k["n"], k["max_depth"], k["min_depth"], k["bin_width"], k["n_bins"],
                              k["acc"], None)
        msg = L.crd_last_error()
        assert rc == -1 and b"crd_depth_eval" in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, "crd_depth_eval")

    refused(b"pred", pred=None)
    refused(b"gt", gt=None)
    refused(b"acc", acc=None)
    refused(b"frames", frames=0)
    refused(b"frames", frames=-2)
    refused(b": n =", n=0)
    refused(b": n =", n=-5)
    for name in ("max_depth", "min_depth", "bin_width"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(name.encode(), **{name: bad})
    refused(b"min_depth", min_depth=100.0)                      # min_depth >= max_depth
    refused(b"min_depth", min_depth=250.0)
    refused(b"n_bins", n_bins=9)                                # not ceil(max_depth / bin_width)
    refused(b"n_bins", n_bins=11)
    refused(b"n_bins", n_bins=0)
    refused(b"n_bins", max_depth=95.0, n_bins=9)                # a partial last bin still counts: ceil(9.5) = 10
    refused(b"n_bins", max_depth=1000.0, n_bins=100)            # more than CRD_EVAL_MAX_BINS
    assert built.EVAL_MAX_BINS < 100


def _synthetic_frame(seed=0, n=5000):
    rs = np.random.RandomState(seed)
    d = rs.uniform(0.5, 99.5, size=n)
    gt = (1.0 - d / 100.0).astype(np.float32)
    gt[rs.uniform(size=n) < 0.5] = 0.0
    dp = d * (1.0 + 0.3 * rs.uniform(-1, 1, size=n))
    pred = (1.0 - dp / 100.0).astype(np.float32)
    return pred, gt


def test_metrics_from_sums_against_numpy():
    from camradepth_amd.metrics import EVAL_METRICS, metrics_from_sums
    pred, gt = _synthetic_frame()
    sums = ref.frame_sums(pred, gt)                             # [10][12] float64
    assert sums[:, 0].sum() > 1000
    # written out once more from the per-pixel quantities, for the whole frame: the restatement of the metric formulas
    dg, dp, valid = ref.distances(pred, gt)
    g, p = dg[valid].astype(np.float64), dp[valid].astype(np.float64)
    e, r, q = p - g, np.log(p) - np.log(g), 1 / p - 1 / g
    m = np.maximum(dp[valid] / dg[valid], dg[valid] / dp[valid])
    direct = {"MAE": np.mean(np.abs(e)), "RMSE": np.sqrt(np.mean(e * e)), "AbsRel": np.mean(np.abs(e) / g), "SqRel": np.mean(e * e / g),
              "RMSElog": np.sqrt(np.mean(r * r)), "SILog": 100 * np.sqrt(np.mean(r * r) - np.mean(r) ** 2),
              "iMAE": 1000 * np.mean(np.abs(q)), "iRMSE": 1000 * np.sqrt(np.mean(q * q)),
              "delta1": np.mean(m < 1.25), "delta2": np.mean(m < 1.25 ** 2), "delta3": np.mean(m < 1.25 ** 3)}
    got = metrics_from_sums(sums.sum(axis=0))
    assert set(got) == set(EVAL_METRICS) == set(direct)
    for k in EVAL_METRICS:
        np.testing.assert_allclose(got[k], direct[k], rtol=1e-9, err_msg=k)       # (a mean of sums against a mean of terms)
    # cap handling: the bins below cap / bin_width, against the formulas on those sums -- rtol 1e-12
    for cap in (10.0, 30.0, 50.0, 80.0, 100.0):
        s = ref.cap_sums(sums, cap)
        got, exp = metrics_from_sums(s), ref.metrics(s)
        sel = valid & (dg < cap)
        assert s[0] == sel.sum() > 0
        for k in EVAL_METRICS:
            np.testing.assert_allclose(got[k], exp[k], rtol=1e-12, err_msg=f"{k} at cap {cap}")
    for b in range(10):                                         # and bin by bin, lists and tuples accepted
        for k, v in metrics_from_sums(list(sums[b])).items():
            np.testing.assert_allclose(v, ref.metrics(sums[b])[k], rtol=1e-12)
    # an empty frame is None; NaN sums give NaN metrics; a wrong length is refused
    assert metrics_from_sums(np.zeros(12)) is None
    assert metrics_from_sums(ref.frame_sums(pred, np.zeros_like(gt)).sum(axis=0)) is None
    assert all(np.isnan(v) for v in metrics_from_sums([float("nan")] * 12).values())
    with pytest.raises(ValueError):
        metrics_from_sums([1.0] * 4)
    # SILog never takes the root of a rounding-negative variance
    assert metrics_from_sums([3, 0, 0, 0, 0, 3 * 0.1, 3 * 0.01 - 1e-12, 0, 0, 3, 3, 3])["SILog"] == 0.0


def test_depth_eval_host_side_surface():
    """What needs no device: bins, cap validation, empty results, CPU tensors refused."""
    import torch
    from camradepth_amd.lib import CrdError
    from camradepth_amd.metrics import DepthEval
    ev = DepthEval()
    assert (ev.max_depth, ev.min_depth, ev.bin_width, ev.n_bins) == (100.0, 1e-3, 10.0, 10)
    assert DepthEval(128.0, bin_width=16.0).n_bins == 8 and DepthEval(95.0).n_bins == 10
    assert ev.result() is None and ev.per_frame() == [] and ev.sums().shape == (0, 10, 12)
    assert [(r["lo"], r["hi"]) for r in ev.by_range()] == [(10.0 * b, 10.0 * b + 10.0) for b in range(10)]
    for bad in (0.0, 5.0, 55.0, 110.0, -10.0):
        with pytest.raises(CrdError):
            ev.result(cap=bad)
    with pytest.raises(CrdError):
        ev.update(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    for kw in (dict(max_depth=0.0), dict(min_depth=-1.0), dict(bin_width=float("nan")), dict(min_depth=100.0), dict(bin_width=1.0)):
        with pytest.raises(CrdError):
            DepthEval(**kw)


def test_trainer_test_signature_has_the_new_keywords_off_by_default():
    from camradepth_amd.runner import Trainer
    p = inspect.signature(Trainer.test).parameters
    assert list(p) == ["self", "save", "extended", "caps"]
    assert p["save"].default is False and p["extended"].default is False and p["caps"].default is None
