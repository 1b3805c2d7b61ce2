"""CPU: the float64 restatement of the segmentation criterion and metrics (tests/seg_loss_ref.py) against torch's float64
cross_entropy(ignore_index=255) with autograd through the focal transform, at the shapes, label mixes and logit families of the
GPU tests (tests/seg_loss_cases.py); the first-maximum rule against np.argmax; the confusion matrix against oracle.losses; and
the argument checks of crd_seg_confusion, which are refused before any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import seg_loss_cases as cases
from tests import seg_loss_ref as ref


def _torch_focal(logits, labels):
    """-> (ce, focal, dlogits) of torch in float64; NaN loss and zero gradient when nothing is valid."""
    x = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    B, C, HW = logits.shape
    ce = F.cross_entropy(x, torch.from_numpy(labels), ignore_index=255)
    focal = (1 - torch.exp(-ce)) ** 2 * ce
    focal.backward()
    return float(ce.detach()), float(focal.detach()), x.grad.numpy()


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_restatement_equals_torch_float64(case):
    (B, C, HW), mix, fam = case
    logits, labels = cases.make_case(case)
    s, n, oor = ref.ce_sums(logits, labels, C)
    assert oor == 0 and n == int((labels != 255).sum())
    ce_t, focal_t, grad_t = _torch_focal(logits, labels)
    grad = ref.focal_grad(logits, labels, C, 1.0)
    if n == 0:                                        # torch: mean over nothing = NaN, and a backward that writes zeros
        assert np.isnan(ce_t) and np.isnan(focal_t) and np.isnan(ref.focal(s, n))
        assert not grad_t.any() and not grad.any() and s == 0.0
        return
    assert s / n == pytest.approx(ce_t, rel=1e-12, abs=1e-300)
    assert ref.focal(s, n) == pytest.approx(focal_t, rel=1e-11, abs=1e-300)
    scale = np.abs(grad_t).max()
    assert np.abs(grad - grad_t).max() <= 1e-11 * scale
    assert np.array_equal(grad == 0, grad_t == 0)     # ignored pixels and -inf classes: exactly zero in both
    assert not grad[np.broadcast_to((labels == 255)[:, None, :], grad.shape)].any()
    if fam == "neg_inf" and C > 1:
        assert np.isinf(logits).any() and np.isfinite(s) and not grad[np.isinf(logits)].any()
    if C == 1:
        assert s == 0.0 and ref.focal(s, n) == 0.0 and not grad.any()
    # the gradient is linear in g
    np.testing.assert_allclose(ref.focal_grad(logits, labels, C, -1.75), -1.75 * grad, rtol=1e-15, atol=0)


def test_the_cases_cover_what_they_are_chosen_for():
    have = set(cases.CASES)
    assert {c[0] for c in have} == set(cases.SHAPES)
    for shape in (cases.MAIN,):
        assert {(m, f) for s, m, f in have if s == shape} == {(m, f) for m in cases.MIXES for f in cases.FAMILIES}
    assert {f for s, m, f in have if s == cases.SECOND} == set(cases.FAMILIES)
    B, C, HW = cases.BIG
    assert B * HW > 2048 * 256 and (B * HW) % 256 and B * C * HW < 1.2e6
    lab = cases.make_labels(cases.MAIN, "one_valid")
    assert (lab != 255).sum() == 1 and lab[-1, -1] != 255
    lab = cases.make_labels(cases.MAIN, "sample_ignored")
    assert (lab[1] == 255).all() and (lab[0] != 255).any() and (lab[2] != 255).any()
    assert (cases.make_labels(cases.MAIN, "all_ignored") == 255).all()
    lab = cases.make_labels(cases.MAIN, "uniform")
    assert 0.05 < (lab == 255).mean() < 0.15 and set(np.unique(lab)) == set(range(21)) | {255}
    x = cases.make_logits(cases.MAIN, "confident", lab)
    top2 = np.sort(x, axis=1)[:, -2:, :]
    assert np.allclose(top2[:, 1] - top2[:, 0], 30.0, atol=1e-4)
    assert ref.ce_sums(x, lab, 21)[0] < 1e-6
    x = cases.make_logits(cases.MAIN, "shift1e4", lab)
    assert x.min() > 9900 and np.isfinite(ref.ce_sums(x, lab, 21)[0])
    x = cases.make_logits(cases.MAIN, "randn50", lab)
    ce = ref.ce_terms(x, lab, 21)[0]
    assert ce.max() > 104                              # a target probability below fp32's exp underflow (e^-104 < 2^-149)


def test_out_of_range_labels_are_skipped_and_counted():
    logits, labels = cases.make_oor_case()
    B, C, HW = cases.OOR_SHAPE
    valid, oor = ref.label_masks(labels, C)
    assert set(np.unique(labels[oor])) == set(cases.OOR_VALUES) and np.abs(labels).max() <= 300
    assert 3 < oor.sum() < 0.1 * labels.size and (labels == 255).any() and valid.sum() > 0.7 * labels.size
    s, n, bad = ref.ce_sums(logits, labels, C)
    assert n == valid.sum() and bad == oor.sum()
    # the same as torch on the labels with the out-of-range ones turned into ignored ones (on the labels as they are it raises)
    clean = np.where(oor, 255, labels)
    ce_t, focal_t, grad_t = _torch_focal(logits, clean)
    assert s / n == pytest.approx(ce_t, rel=1e-12)
    grad = ref.focal_grad(logits, labels, C, 1.0)
    assert np.abs(grad - grad_t).max() <= 1e-11 * np.abs(grad_t).max()
    assert not grad[np.broadcast_to(oor[:, None, :], grad.shape)].any()
    with pytest.raises((IndexError, RuntimeError)):
        F.cross_entropy(torch.from_numpy(logits.astype(np.float64)), torch.from_numpy(labels), ignore_index=255)


def test_argmax_first_is_numpys_rule_on_ties():
    rs = np.random.RandomState(21)
    for shape, axis in (((300, 21), 1), ((5, 300), 0), ((2, 7, 129), 1), ((40, 1), 1), ((300, 2), 1), ((64, 300), 0)):
        x = cases.tied_logits(rs, shape)
        got = ref.argmax_first(x, axis)
        assert np.array_equal(got, np.argmax(x, axis=axis))
        if x.shape[axis] >= 2:
            assert cases.tied_fraction(x, axis) >= 0.05
    x = np.zeros((3, 4), dtype=np.float32)
    assert np.array_equal(ref.argmax_first(x, 1), [0, 0, 0])
    x[:, 2] = -np.inf
    x[1, 3] = 1.0
    assert np.array_equal(ref.argmax_first(x, 1), [0, 3, 0])


def test_confusion_equals_the_oracle_on_the_iou_test_data():
    """The data of tests/test_gpu_data.py::test_seg_iou_matches_oracle; oracle.losses.seg_iou holds the existing restatement
    (bincount of target * C + argmax, macro IoU with absent classes at 0, NaN for a frame with a label outside the classes)."""
    from oracle import losses as ol
    rs = np.random.RandomState(5)
    B, C, H, W = 4, 21, 48, 80
    logits = torch.from_numpy(rs.standard_normal(size=(B, C, H, W)).astype(np.float32))
    labels = torch.from_numpy(rs.randint(0, 21, size=(B, H, W)).astype(np.int64))
    labels[1, :5, :7] = 255
    labels[2][labels[2] > 14] = 3
    logits[3, :, :, :] += 3.0 * torch.nn.functional.one_hot(labels[3], C).permute(2, 0, 1)
    for f in range(B):
        mat, oor = ref.confusion(logits[f].numpy().reshape(C, -1), labels[f].numpy().reshape(-1), C)
        want = ol.seg_iou(logits[f:f + 1], labels[f:f + 1], C)
        assert mat.sum() + oor == H * W
        if f == 1:
            assert oor == 35 and np.isnan(want)
            continue
        assert oor == 0
        t, p = labels[f].reshape(-1), logits[f].argmax(0).reshape(-1)
        assert np.array_equal(mat, torch.bincount(t * C + p, minlength=C * C).reshape(C, C).numpy())
        m = mat.astype(np.float64)
        inter = np.diag(m)
        union = m.sum(0) + m.sum(1) - inter
        iou = np.where(union > 0, inter / np.maximum(union, 1), 0.0).mean()
        assert iou == pytest.approx(want, rel=1e-12)


def test_confusion_counts_every_label_outside_the_classes():
    rs = np.random.RandomState(8)
    C, HW = 5, 400
    x = cases.tied_logits(rs, (C, HW))
    lab = rs.randint(-1, C + 1, size=HW).astype(np.int64)
    lab[::17] = 255
    mat, oor = ref.confusion(x, lab, C)
    assert oor == ((lab < 0) | (lab >= C)).sum() > 0 and mat.sum() == HW - oor
    pred = np.argmax(x, axis=0)
    for t in range(C):
        for p in range(C):
            assert mat[t, p] == ((lab == t) & (pred == p)).sum()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_seg_confusion_refuses_class_counts_outside_its_histogram(built):
    """The LDS histogram holds C * C + 1 counters for 1 <= C <= 64; anything else is refused before any launch."""
    L = built.load()
    buf = ctypes.create_string_buffer(64)          # any non-NULL host address: a refused call launches nothing and reads none of it
    a = ctypes.addressof(buf)
    for C in (65, 0, -1):
        rc = L.crd_seg_confusion(a, a, 1, C, 16, a, a, None)
        msg = L.crd_last_error()
        assert rc != 0 and b"crd_seg_confusion" in msg, (C, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, "crd_seg_confusion")
    assert L.crd_seg_confusion(None, a, 1, 21, 16, a, a, None) != 0
    assert L.crd_seg_confusion(a, a, 1, 21, 0, a, a, None) != 0


def test_stat_frac_bits_of_the_header_equal_the_binding(built):
    """The GPU test derives the rounding of one workgroup partial from this constant."""
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "camradepth_hip.h")).read()
    assert int(re.search(r"#define\s+CRD_STAT_FRAC_BITS\s+(\d+)", h).group(1)) == built.STAT_FRAC_BITS


def test_train_step_losses_raise_on_out_of_range_labels(monkeypatch):
    """TrainStep.losses() reads crd_ce_fwd's count of out-of-range labels (slot 14 of acc) where it reads the loss sums anyway."""
    from camradepth_amd import lib as L
    from tests.trainstep_stub import stub_model, stub_trainstep
    monkeypatch.setattr(L, "nonfinite", lambda reset=True: False)
    ts = stub_trainstep(stub_model())
    one = 1 << L.STAT_FRAC_BITS
    for i in range(4):
        ts.acc[4 * i], ts.acc[4 * i + 1] = 3 * one, 2 * one
    ts.acc[2] = one
    ts.sup = True
    v = ts.losses()
    assert v["full"] == 1.5 and v["seg"] == pytest.approx((1 - np.exp(-1.5)) ** 2 * 1.5)
    ts.acc[14] = 5 * one
    with pytest.raises(L.CrdError, match=r"\b5 segmentation label"):
        ts.losses()
    ts.sup = False                              # without the segmentation loss the slot belongs to nobody
    assert ts.losses()["seg"] == 0.0
