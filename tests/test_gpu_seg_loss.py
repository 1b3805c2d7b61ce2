"""GPU: the segmentation criterion (crd_ce_fwd, crd_ce_focal_bwd) and metrics (crd_seg_argmax, crd_seg_confusion) through the C ABI
against the float64 restatement tests/seg_loss_ref.py, at the edge shapes, label mixes and logit families of
tests/seg_loss_cases.py.  The reference is always the restatement, never the kernel.

Bounds.  The cross-entropy SUM: |got - ref| <= nblk 2^-(CRD_STAT_FRAC_BITS + 1) + SUM_REL sum_i |ce_i| -- the rounding of each of the
nblk = min(ceil(rows / 256), 1024) workgroup partials to the fixed-point grid, plus a relative term.  The gradient: the helper of
test_gpu_ops.py at rel = REL, elem = 1e-4 |g| (g = gmul * gout), and exact zeros where the reference is exactly zero.
The relative terms started at the bounds of test_gpu_ops.py::test_losses (1e-5 on the sum, rel-L2 1e-4 on the gradient); on an
MI355X every case measured more than 10x below both (worst relative sum error 1.35e-7, worst rel-L2 1.3e-7), so each is set to
4x its worst measured value.  The element bound stays: the worst case (g = 0.2 / 3.2 / 4) measures 0.18 of it.
Run with -s for the measured error over its bound, per case."""
import functools
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import seg_loss_cases as cases
from tests import seg_loss_ref as ref
from tests.test_gpu_ops import L, P, assert_close, ok
from tests.util import zsum

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TPB, FWD_CAP = 256, 1024
# (gout, gmul): the plain call; a host scale of the trainer's size, 0.2 / 3.2 / 4, and the trainer's own LOSS_W[3] / sum(LOSS_W) /
# update_interval at update_interval = 4; MaskedFocalLoss's device gout
CONVENTIONS = ((None, 1.0), (None, 0.2 / 3.2 / 4), (None, 0.2 / 3.4 / 4), (-1.75, 1.0))
REL, ELEM, SUM_REL = 5.2e-7, 1e-4, 5.4e-7


@functools.lru_cache(maxsize=None)
def frac_bits():
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    return int(re.search(r"#define\s+CRD_STAT_FRAC_BITS\s+(\d+)", h).group(1))


def sum_bound(rows, ce_abs_sum):
    nblk = min(-(-rows // TPB), FWD_CAP)
    return nblk * 2.0 ** -(frac_bits() + 1) + SUM_REL * ce_abs_sum


@functools.lru_cache(maxsize=None)
def reference(case):
    """Computed once per case and shared read-only: inputs, float64 sums, and the gradient for g = 1 (linear in g)."""
    (B, C, HW), mix, fam = case
    logits, labels = cases.make_case(case)
    ce, valid, oor = ref.ce_terms(logits, labels, C)
    grad = ref.focal_grad(logits, labels, C, 1.0)
    for a in (logits, labels, grad):
        a.flags.writeable = False
    return types.SimpleNamespace(logits=logits, labels=labels, sum=float(ce.sum()), abs_sum=float(np.abs(ce).sum()),
                                 count=int(valid.sum()), oor=int(oor.sum()), grad=grad)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def ce_fwd(ld, lab, B, C, HW):
    lib, lb = L()
    acc = zsum(4)
    ok(lb.crd_ce_fwd(P(ld), P(lab), B, C, HW, P(acc), lib.stream()), "crd_ce_fwd")
    return acc


def ce_bwd(ld, lab, B, C, HW, acc, gout, gmul, out=None):
    """-> dlogits; the output starts as NaN everywhere, so an element the kernel does not write shows."""
    lib, lb = L()
    dl = torch.full_like(ld, float("nan")) if out is None else out
    go = None if gout is None else torch.tensor([gout], dtype=torch.float32, device="cuda")
    ok(lb.crd_ce_focal_bwd(P(ld), P(lab), B, C, HW, P(acc), P(go), gmul, P(dl), lib.stream()), "crd_ce_focal_bwd")
    return dl


def check_sum(acc, r, rows, what):
    """Count exact, sum within its bound; -> measured error / bound."""
    a = [int(v) for v in acc.cpu()]
    one = 1 << frac_bits()
    assert a[1] == r.count * one, f"{what}: count {a[1] / one} != {r.count}"
    assert a[2] == r.oor * one and a[3] == 0, f"{what}: acc[2:] = {a[2] / one}, {a[3]}"
    err, bound = abs(a[0] / one - r.sum), sum_bound(rows, r.abs_sum)
    print(f"  {what}: ce sum {a[0] / one:.9g} ref {r.sum:.9g} err {err:.3e} (rel {err / max(r.abs_sum, 1e-300):.3e}) bound {bound:.3e} "
          f"ratio {err / bound:.3f}")
    assert err <= bound, f"{what}: ce sum {a[0] / one!r} vs {r.sum!r}: err {err:.3e} > {bound:.3e}"
    return err / bound


def check_grad(got, want, g, what):
    """want: float64 numpy.  No NaN, exact zeros where the reference has them, the helper's bounds elsewhere; -> the measured
    (max error / (elem |g| scale), rel-L2 / rel)."""
    got = got.detach().cpu()
    assert not torch.isnan(got).any(), f"{what}: NaN in dlogits"
    w = torch.from_numpy(np.ascontiguousarray(want))
    zero = w == 0
    assert not got[zero].any(), f"{what}: {int((got[zero] != 0).sum())} non-zero where the reference is exactly 0"
    scale = w.abs().max().item() + 1e-12
    e = (got.double() - w).abs().max().item() / (ELEM * abs(g) * scale)
    r = ((got.double() - w).norm() / (w.norm() + 1e-30)).item() / REL
    print(f"  {what}: g {g:.6g} max err / bound {e:.3f}  rel-L2 {r * REL:.3e} / bound {r:.4f}")
    assert_close(got, w, what, rel=REL, elem=ELEM * abs(g))
    return e, r


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_ce_forward_and_focal_backward(case):
    (B, C, HW), mix, fam = case
    r = reference(case)
    what = cases.case_id(case)
    ld, lab = dev(r.logits), dev(r.labels)
    lib, _ = L()
    lib.nonfinite(reset=True)
    acc = ce_fwd(ld, lab, B, C, HW)
    assert not lib.nonfinite(reset=True), f"{what}: a partial of the sums was not finite"
    check_sum(acc, r, B * HW, what)
    assert torch.equal(ce_fwd(ld, lab, B, C, HW), acc), "a second run into a fresh accumulator gives other bits"
    if C == 1:
        assert int(acc[0]) == 0                    # one class: every term is exactly 0
    for gout, gmul in CONVENTIONS:
        g = gmul * (1.0 if gout is None else gout)
        dl = ce_bwd(ld, lab, B, C, HW, acc, gout, gmul)
        if r.count == 0 or C == 1:
            assert not torch.isnan(dl).any() and not dl.any(), f"{what}: dlogits must be exactly zero everywhere"
            continue
        check_grad(dl, r.grad * g, g, what)
        if fam == "neg_inf":
            assert not dl[torch.isinf(ld)].any()


def test_all_ignored_through_the_module():
    """Nothing valid: count 0, a NaN loss (0 / 0, as torch's mean) and a gradient of exact zeros, no NaN written."""
    from camradepth_amd.losses import MaskedFocalLoss
    case = (cases.MAIN, "all_ignored", "randn2")
    r = reference(case)
    B, C, HW = cases.MAIN
    x = dev(r.logits).reshape(B, C, 1, HW).requires_grad_(True)
    loss = MaskedFocalLoss()(x, dev(r.labels).reshape(B, 1, HW))
    assert r.count == 0 and math.isnan(float(loss.detach()))
    loss.backward()
    assert not torch.isnan(x.grad).any() and not x.grad.any()


def test_module_equals_the_direct_calls():
    """MaskedFocalLoss forward and backward on (3, 21, 257): the same sums and the same kernel with a device gout."""
    from camradepth_amd import lib
    from camradepth_amd.losses import MaskedFocalLoss
    case = (cases.MAIN, "uniform", "randn2")
    r = reference(case)
    B, C, HW = cases.MAIN
    ld, lab = dev(r.logits), dev(r.labels)
    acc = ce_fwd(ld, lab, B, C, HW)
    a = lib.stat_value(acc)
    ce = (a[0] / a[1]).float()
    direct = (1 - torch.exp(-ce)) ** 2 * ce
    x = ld.clone().reshape(B, C, HW, 1).requires_grad_(True)
    loss = MaskedFocalLoss()(x, lab.reshape(B, HW, 1))
    assert torch.equal(loss.detach(), direct)
    assert float(loss.detach()) == pytest.approx(ref.focal(r.sum, r.count), rel=1e-5)
    (loss * -1.75).backward()
    want = ce_bwd(ld, lab, B, C, HW, acc, -1.75, 1.0)
    assert torch.equal(x.grad.reshape(B, C, HW), want)
    check_grad(x.grad.reshape(B, C, HW), r.grad * -1.75, -1.75, "MaskedFocalLoss")


def test_total_loss_with_supervised_seg_equals_the_restatement():
    """total_loss at update_interval = 4 on a synthetic batch: the value against the float64 terms combined at total_loss's weights,
    and the gradient that reaches the logits against focal_grad at g = 0.2 / sum(w) / 4 (w = 1, 1, 1, 0.2, 0.2 in total_loss)."""
    from camradepth_amd import synth
    from camradepth_amd.losses import total_loss
    from oracle import losses as ol
    B, H, W, C, k = 2, 32, 48, 21, 4
    batch = synth.make_batch(B, H, W, seed=17)
    g = torch.Generator().manual_seed(23)
    seg = torch.randn(B, C, H, W, generator=g) * 2
    final = torch.rand(B, 1, H, W, generator=g) * 1.4 - 0.2
    half = torch.rand(B, 1, H // 2, W // 2, generator=g) * 1.4 - 0.2
    quarter = torch.rand(B, 1, H // 4, W // 4, generator=g) * 1.4 - 0.2
    segd = seg.cuda().requires_grad_(True)
    out = {"depth": {"final_depth": final.cuda().requires_grad_(True),
                     "intermediate_depths": [quarter.cuda().requires_grad_(True), half.cuda().requires_grad_(True)]},
           "seg": {"final_seg": segd}}
    loss, parts = total_loss(out, {n: v.cuda() for n, v in batch.items()}, True, update_interval=k)
    loss.backward()
    logits, labels = seg.numpy().reshape(B, C, H * W), batch["seg"].numpy().reshape(B, H * W)
    s, n, oor = ref.ce_sums(logits, labels, C)
    l_seg = ref.focal(s, n)
    l_full = float(ol.masked_smooth_l1(final.double(), batch["gt_full"].double()))
    l_half = float(ol.masked_smooth_l1(half.double().squeeze(1), batch["gt_half"].double().squeeze(1)))
    l_quarter = float(ol.masked_smooth_l1(quarter.double().squeeze(1), batch["gt_quarter"].double().squeeze(1)))
    w = [1, 1, 1, 0.2, 0.2]
    want = (w[0] * l_full + w[1] * l_half + w[2] * l_quarter + w[3] * l_seg + w[4] * 0) / sum(w) / k
    assert oor == 0 and float(parts["seg"].detach()) == pytest.approx(l_seg, rel=1e-5)
    assert float(loss.detach()) == pytest.approx(want, rel=1e-5)          # every term a positive mean held to 1e-5, positive weights
    gm = w[3] / sum(w) / k
    check_grad(segd.grad.reshape(B, C, H * W), ref.focal_grad(logits, labels, C, gm), gm, "total_loss")


def test_out_of_range_labels_are_never_dereferenced():
    """Labels that are neither a class nor 255.  The logits are a view inside one buffer of sentinels with 320 planes of margin on
    each side: a read through any label of the case lands inside the buffer, on a sentinel, and shows in the sum."""
    from camradepth_amd import lib
    from camradepth_amd.losses import MaskedFocalLoss
    B, C, HW = cases.OOR_SHAPE
    logits, labels = cases.make_oor_case()
    assert np.abs(labels).max() <= 300 < cases.OOR_MARGIN_PLANES
    valid, oor = ref.label_masks(labels, C)
    ce, _, _ = ref.ce_terms(logits, labels, C)
    r = types.SimpleNamespace(sum=float(ce.sum()), abs_sum=float(np.abs(ce).sum()), count=int(valid.sum()), oor=int(oor.sum()))
    assert r.oor >= len(cases.OOR_VALUES) and r.count > 0
    margin, n = cases.OOR_MARGIN_PLANES * HW, B * C * HW

    def guarded(fill):
        buf = torch.full((margin + n + margin,), cases.SENTINEL, dtype=torch.float32, device="cuda")
        view = buf[margin:margin + n].view(B, C, HW)
        if fill is not None:
            view.copy_(fill)
        return buf, view

    def margins_intact(buf):
        return bool((buf[:margin] == cases.SENTINEL).all()) and bool((buf[margin + n:] == cases.SENTINEL).all())

    lbuf, ld = guarded(dev(logits))
    dbuf, dl = guarded(None)
    lab = dev(labels)
    try:
        acc = ce_fwd(ld, lab, B, C, HW)
        check_sum(acc, r, B * HW, "out-of-range labels")               # the valid pixels' sum and count, acc[2] = their number
        gm = 0.2 / 3.2 / 4
        ce_bwd(ld, lab, B, C, HW, acc, None, gm, out=dl)
        check_grad(dl, ref.focal_grad(logits, labels, C, gm), gm, "out-of-range labels")
        assert not dl[dev(np.broadcast_to(oor[:, None, :], (B, C, HW)))].any()
        assert margins_intact(lbuf) and margins_intact(dbuf)
        assert torch.equal(ld.cpu(), torch.from_numpy(logits))
        with pytest.raises(lib.CrdError, match=rf"\b{r.oor} target label"):
            MaskedFocalLoss()(ld.view(B, C, 7, 11), lab.view(B, 7, 11))
    finally:
        lib.nonfinite(reset=True)            # (a sentinel that reached a sum would have raised the sticky flag: leave it clear)


# ---- crd_seg_argmax -------------------------------------------------------------------------------------------------------
ARGMAX_CASES = [
    # B, P, C, ld, num_classes, y_f32, y_ld, y_coff
    (2, 257, 21, 24, 21, 0, 8, 3),
    (2, 257, 21, 21, 21, 1, 1, 0),
    (3, 65, 5, 8, 21, 1, 4, 2),
    (3, 65, 5, 5, 5, 0, 1, 0),
    (1, 1, 21, 24, 21, 1, 1, 0),
    (1, 1, 5, 8, 5, 0, 8, 7),
    (2, 257, 1, 1, 1, 0, 8, 3),
    (2, 65, 1, 8, 21, 1, 1, 0),
    (1, 257, 2, 2, 2, 1, 2, 1),
    (5, 257, 21, 24, 21, 0, 1, 0),           # 1285 rows: more than one workgroup, bf16 rows packed
]


@pytest.mark.parametrize("case", ARGMAX_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_seg_argmax_takes_the_first_maximum(case):
    lib, lb = L()
    B, Pn, C, ld, nc, y_f32, y_ld, y_coff = case
    rs = np.random.RandomState(31 + B * Pn + C)
    x = np.full((B * Pn, ld), 100.0, dtype=np.float32)           # the padding columns would win if they were read
    x[:, :C] = cases.tied_logits(rs, (B * Pn, C))
    if C >= 2 and B * Pn >= 65:
        assert cases.tied_fraction(x[:, :C], 1) >= 0.05
    dt = torch.float32 if y_f32 else torch.bfloat16
    y = torch.full((B * Pn, y_ld), -7.0, dtype=dt, device="cuda")
    xd = dev(x)
    ok(lb.crd_seg_argmax(P(xd), ld, B, Pn, C, nc, P(y), y_f32, y_ld, y_coff, lib.stream()), "crd_seg_argmax")
    want = torch.from_numpy(ref.argmax_first(x[:, :C], 1).astype(np.float32) / np.float32(nc)).to(dt)    # the same roundings
    got = y.cpu()
    assert torch.equal(got[:, y_coff], want)
    others = [c for c in range(y_ld) if c != y_coff]
    assert (got[:, others] == -7.0).all()
    if C == 1:
        assert not got[:, y_coff].any()


# ---- crd_seg_confusion ----------------------------------------------------------------------------------------------------
CONFUSION_CASES = [(C, HW, F) for C in (1, 2, 21, 64) for HW in (1, 255, 257, 40000) for F in (1, 3) if C * HW * F <= 3_000_000]


@pytest.mark.parametrize("C,HW,frames", CONFUSION_CASES)
def test_seg_confusion_equals_the_restatement(C, HW, frames):
    """40000 pixels are more than 128 workgroups of 256: the stride loop is taken.  Labels include 255, -1 and C."""
    lib, lb = L()
    rs = np.random.RandomState(1000 * C + HW + frames)
    x = cases.tied_logits(rs, (frames, C, HW))
    lab = rs.randint(0, C, size=(frames, HW)).astype(np.int64)
    u = rs.random_sample((frames, HW))
    lab[u < 0.09] = np.asarray([255, -1, C])[rs.randint(0, 3, size=int((u < 0.09).sum()))]
    if HW == 1:
        lab[:, 0] = [C - 1, -1, C][:frames]
    else:
        lab[0, :3], lab[-1, -1] = [255, -1, C], C
    if C >= 2 and HW >= 255:
        assert cases.tied_fraction(x, 1) >= 0.05
    want = [ref.confusion(x[f], lab[f], C) for f in range(frames)]
    mat = torch.zeros(frames, C, C, dtype=torch.int64, device="cuda")
    oor = torch.zeros(frames, dtype=torch.int64, device="cuda")
    xd, labd = dev(x), dev(lab)
    for k in (1, 2):                                   # the second call accumulates
        ok(lb.crd_seg_confusion(P(xd), P(labd), frames, C, HW, P(mat), P(oor), lib.stream()), "crd_seg_confusion")
        for f in range(frames):
            assert np.array_equal(mat[f].cpu().numpy(), k * want[f][0]), (f, k)
            assert int(oor[f]) == k * want[f][1], (f, k)
    assert all(int(want[f][0].sum()) + want[f][1] == HW for f in range(frames))


def test_seg_iou_updates_append_frames():
    """SegIoU on tied logits: two updates keep their frames apart, each the restatement's matrix."""
    from camradepth_amd.metrics import SegIoU
    rs = np.random.RandomState(77)
    C, H, W = 21, 5, 51
    x = cases.tied_logits(rs, (3, C, H * W))
    lab = rs.randint(0, C, size=(3, H * W)).astype(np.int64)
    lab[1, 7] = 255
    iou = SegIoU(C)
    iou.update(dev(x[:2]).view(2, C, H, W), dev(lab[:2]).view(2, H, W))
    iou.update(dev(x[2:]).view(1, C, H, W), dev(lab[2:]).view(1, H, W))
    mats, oor = torch.cat(iou.mats).cpu().numpy(), torch.cat(iou.oor).cpu().numpy()
    for f in range(3):
        m, bad = ref.confusion(x[f], lab[f], C)
        assert np.array_equal(mats[f], m) and oor[f] == bad
    got = iou.per_frame()
    assert math.isnan(got[1]) and not math.isnan(got[0]) and not math.isnan(got[2])
