"""The inputs of the segmentation-loss tests (test_seg_loss_ref_cpu.py, test_gpu_seg_loss.py): shapes (B, C, HW), label mixes and
logit families, each chosen for an edge of crd_ce_fwd / crd_ce_focal_bwd (256 threads per workgroup, 64 per wave, one pixel per
thread, grid-stride loops capped at 1024 workgroups forward and 2048 backward)."""
import zlib

import numpy as np

SHAPES = {
    (1, 1, 1): "one class: loss exactly 0, gradient exactly 0",
    (1, 2, 1): "one pixel, one workgroup, one lane",
    (3, 21, 257): "HW odd: waves and workgroups straddle sample boundaries",
    (2, 5, 255): "one short of the workgroup size",
    (4, 21, 65): "one over the wave size",
    (1, 64, 129): "many classes, small plane",
    (2, 150, 33): "long class loop, small planes",
    (2, 21, 960): "the case of test_gpu_ops.py::test_losses",
    (3, 2, 180001): "540003 rows > 2048 x 256: both grid-stride loops take a second trip with an odd tail",
}
MIXES = ("uniform", "sample_ignored", "all_ignored", "one_valid", "one_class")
FAMILIES = ("randn2", "randn50", "shift1e4", "neg_inf", "confident")
MAIN, SECOND, BIG = (3, 21, 257), (2, 5, 255), (3, 2, 180001)


def _cases():
    out = [(s, "uniform", "randn2") for s in SHAPES]
    out += [(MAIN, m, f) for m in MIXES for f in FAMILIES]
    out += [(SECOND, "uniform", f) for f in FAMILIES]
    out += [(SECOND, "sample_ignored", "randn2"), (SECOND, "one_valid", "confident"), (BIG, "one_valid", "randn2"),
            (BIG, "sample_ignored", "randn50"), ((1, 64, 129), "uniform", "neg_inf"), ((2, 150, 33), "one_class", "randn50"),
            ((4, 21, 65), "sample_ignored", "shift1e4"), ((1, 2, 1), "uniform", "confident")]
    return list(dict.fromkeys(out))


CASES = _cases()


def case_id(case):
    (B, C, HW), mix, fam = case
    return f"{B}x{C}x{HW}-{mix}-{fam}"


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def make_labels(shape, mix):
    """int64 [B, HW]."""
    B, C, HW = shape
    rs = _rs("labels", shape, mix)
    lab = rs.randint(0, C, size=(B, HW)).astype(np.int64)
    if mix == "uniform":
        lab[rs.random_sample((B, HW)) < 0.1] = 255
    elif mix == "sample_ignored":
        lab[rs.random_sample((B, HW)) < 0.1] = 255
        lab[B // 2] = 255
    elif mix == "all_ignored":
        lab[:] = 255
    elif mix == "one_valid":                    # the last row of the last sample
        keep = lab[B - 1, HW - 1]
        lab[:] = 255
        lab[B - 1, HW - 1] = keep
    elif mix == "one_class":
        lab[:] = C - 1
    else:
        raise ValueError(mix)
    return lab


def make_logits(shape, family, labels):
    """float32 [B, C, HW]: what the kernel and the reference both read.  Where a family speaks of the target class, an ignored
    pixel takes class 0 for it."""
    B, C, HW = shape
    rs = _rs("logits", shape, family)
    x = rs.standard_normal((B, C, HW)) * (50.0 if family == "randn50" else 2.0)
    tgt = np.where((labels >= 0) & (labels < C), labels, 0)
    is_tgt = np.arange(C)[None, :, None] == tgt[:, None, :]
    if family == "shift1e4":
        x = x + 1e4
    elif family == "neg_inf":                   # as masking produces: about 20 % of the non-target entries
        x[(rs.random_sample((B, C, HW)) < 0.2) & ~is_tgt] = -np.inf
    elif family == "confident":                 # the target logit 30 above the largest of the rest
        rest = np.where(is_tgt, -np.inf, x).max(axis=1, keepdims=True) if C > 1 else x
        x = np.where(is_tgt, rest + 30.0, x)
    elif family not in ("randn2", "randn50"):
        raise ValueError(family)
    return x.astype(np.float32)


def make_case(case):
    shape, mix, fam = case
    labels = make_labels(shape, mix)
    return make_logits(shape, fam, labels), labels


# ---- the label-range case: labels that are neither a class nor 255 next to valid and ignored ones ----
OOR_SHAPE = (2, 21, 77)
OOR_VALUES = (-3, -1, 21, 22, 254, 256, 300)       # with |label| <= 300 a stray read through one stays within 320 planes of the logits
OOR_MARGIN_PLANES = 320
SENTINEL = 1e30


def make_oor_case():
    B, C, HW = OOR_SHAPE
    rs = _rs("oor")
    lab = rs.randint(0, C, size=(B, HW)).astype(np.int64)
    u = rs.random_sample((B, HW))
    lab[u < 0.1] = 255
    bad = (u >= 0.1) & (u < 0.15)
    lab[bad] = np.asarray(OOR_VALUES)[rs.randint(0, len(OOR_VALUES), size=int(bad.sum()))]
    for k, v in enumerate(OOR_VALUES):           # every value at least once, the first and the last pixel among them
        lab[k % B, (0, HW - 1, 5, 11, 23, 40, 64)[k]] = v
    return (rs.standard_normal((B, C, HW)) * 2.0).astype(np.float32), lab


# ---- arg-max ties: continuous random logits never tie, these often do ----
def tied_logits(rs, shape):
    """float32 logits of standard deviation 0.25 rounded to bf16 and then to one decimal: with two classes about one pixel in ten has
    a tied maximum, with 21 about one in four."""
    import torch
    x = torch.from_numpy((rs.standard_normal(shape) * 0.25).astype(np.float32)).to(torch.bfloat16).float().numpy()
    return np.round(x, 1).astype(np.float32)


def tied_fraction(x, axis):
    return float(((x == x.max(axis=axis, keepdims=True)).sum(axis=axis) > 1).mean())
