"""Inputs of tests/golden/loss_zoo.npz (tests/golden/make_loss_zoo_golden.py), rebuilt from seeds by the generator and the tests
alike: the fixture keeps loss values and gradients only (the 8 x 256 x 416 case's gradients as tests/util.py:subsample views)."""
import numpy as np

# name -> (B, H, W, seed, kind)
CASES = {
    "rand": (2, 24, 40, 11, "rand"),
    "odd": (3, 37, 53, 12, "rand"),
    "bench": (8, 256, 416, 13, "rand"),
    "dzero": (2, 24, 40, 14, "dzero"),          # a tenth of the valid elements have pred == target
    "edge": (2, 24, 40, 15, "edge"),            # max |d| = 5, so BerHu's c = 0.2 * 5 = 1 exactly; elements at |d| == c
    "equal": (2, 24, 40, 16, "equal"),          # pred == target on the whole mask: BerHu's c = 0
    "edge_f32": (2, 24, 40, 17, "edge_f32"),    # c = 0.2 * max |d| not dyadic, elements at |d| == fp32(c) with fp32(c)^2 > fp32(c^2)
}
EDGE_F32_MAX = 4.432113     # (exactly: the nearest fp32) c = 0.8864226..., where fp32(|d|^2) - fp32(c^2) is 0 and the unrounded one is not
FULL_GRAD_MAX = 20000       # cases with more elements store subsampled gradients


def depth_pair(name):
    """-> pred, target float32 [B, 1, H, W]; the mask is target > 0 (about 60 % of the elements)."""
    B, H, W, seed, kind = CASES[name]
    rs = np.random.RandomState(seed)
    shape = (B, 1, H, W)
    valid = rs.uniform(size=shape) >= 0.4
    if kind == "edge":
        # dyadic values: pred - target is exact, |d| in {0, 1/8, ..., 5}, with +-1 (= c) and +-5 (the max) present
        target = np.where(valid, 2.0, 0.0).astype(np.float32)
        d = rs.randint(-40, 41, size=shape).astype(np.float32) / 8.0
        flat = d.reshape(-1)
        vi = np.flatnonzero(valid.reshape(-1))
        flat[vi[:4]] = [5.0, -5.0, 1.0, -1.0]
        flat[vi[4:12]] = 1.0
        flat[vi[12:20]] = -1.0
        pred = (target + d).astype(np.float32)
        return pred, target
    target = np.where(valid, rs.uniform(0.01, 1.0, size=shape), 0.0).astype(np.float32)
    pred = rs.uniform(-0.2, 1.2, size=shape).astype(np.float32)
    if kind == "edge_f32":
        # target = 2x, pred = x gives |d| == x exactly (Sterbenz); the max |d| on one element, x = fp32(0.2 * max) on sixteen
        mx = np.float32(EDGE_F32_MAX)
        cf = np.float32(0.2 * float(mx))
        vi = np.flatnonzero(valid.reshape(-1))
        t, p = target.reshape(-1), pred.reshape(-1)
        t[vi[0]], p[vi[0]] = 2 * mx, mx
        t[vi[1:17]], p[vi[1:17]] = 2 * cf, cf
        return pred, target
    if kind == "dzero":
        same = valid & (rs.uniform(size=shape) < 0.1)
        pred = np.where(same, target, pred).astype(np.float32)
    elif kind == "equal":
        pred = np.where(valid, target, pred).astype(np.float32)
    return pred, target


def smooth_pair(name, channels=3):
    """-> pred_depth float32 [B, 1, H, W] (positive, with a run of equal neighbours), image float32 [B, channels, H, W]."""
    B, H, W, seed, kind = CASES[name]
    rs = np.random.RandomState(seed + 100)
    pred = rs.uniform(0.05, 1.0, size=(B, 1, H, W)).astype(np.float32)
    pred[:, :, 1, :W // 2] = pred[:, :, 1, :1]         # equal neighbours: |grad| = 0, sign 0
    if kind == "equal":
        pred[:] = 0.5
    image = rs.uniform(0.0, 1.0, size=(B, channels, H, W)).astype(np.float32)
    return pred, image


def subsample(a, maxn=8192):
    a = np.asarray(a).reshape(-1)
    stride = max(1, -(-a.size // maxn))
    return a[::stride].copy()


def grad_view(name, g):
    """What the fixture stores of a gradient: all of it, or the strided subsample of a large case."""
    g = np.asarray(g, dtype=np.float32)
    return g.copy() if g.size <= FULL_GRAD_MAX else subsample(g)
