"""NumPy restatement of the visualisation back end (camradepth_amd.viz; include/camradepth_hip.h, "Visualisation back end"), shared by
test_viz_ref_cpu.py and test_gpu_viz.py.  Every function takes and returns host arrays; the kernels agree with it bit for bit.  fp32
arithmetic is NumPy's on float32 arrays: one correctly rounded operation per line, never fused."""
import numpy as np

F = np.float32


def finite_range(m):
    """(vmin, vmax) of one frame over its finite values, in the map's own type; (0, 0) when it has none."""
    m = np.asarray(m)
    v = m[np.isfinite(m)] if m.dtype.kind == "f" else m.reshape(-1)
    if v.size == 0:
        return m.dtype.type(0), m.dtype.type(0)
    return v.min(), v.max()


def frame_range(x):
    """fp32 [B, 2]: finite_range of every frame (what viz.frame_range returns for float maps and for labels)."""
    return np.array([finite_range(f) for f in x], dtype=F).reshape(len(x), 2)


def _index(y):
    """The table row of the scaled value y: truncation, y < 0 -> 0, y >= 256 -> 255 (y == 256 among them), NaN -> 0."""
    inside = (y >= 0) & (y < 256)
    idx = np.where(inside, y, 0).astype(np.int64)
    return np.where(y >= 256, 255, idx)


def index_f32(m, vmin, vmax):
    """Item 1 for one frame.  The map and the scaling by 256 are fp32, the range is held in fp64, as matplotlib holds it: the
    difference and the quotient are computed in fp64 and each rounded to fp32.  Non-finite pixels get row 0 here; colorize paints
    them in bad_colour."""
    m = np.asarray(m, dtype=F)
    vmin, vmax = np.float64(F(vmin)), np.float64(F(vmax))
    if vmin == vmax:
        return np.zeros(m.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        t = (m.astype(np.float64) - vmin).astype(F)
        q = (t.astype(np.float64) / (vmax - vmin)).astype(F)
        y = q * F(256)
    assert y.dtype == F
    return _index(y)


def index_f64(lab, vmin, vmax):
    """Item 2 for one frame of labels: the same in fp64."""
    lab = np.asarray(lab).astype(np.float64)
    vmin, vmax = np.float64(vmin), np.float64(vmax)
    if vmin == vmax:
        return np.zeros(lab.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        y = (lab - vmin) / (vmax - vmin) * 256.0
    return _index(y)


def _ranges(x, vmin, vmax):
    """Per-frame (vmin, vmax): the frames' own, two numbers for every frame, or a [B, 2] array."""
    assert (vmin is None) == (vmax is None)
    if vmin is None:
        return [finite_range(f) for f in x]
    if np.ndim(vmin) == 0:
        return [(vmin, vmax)] * len(x)
    return list(zip(vmin, vmax))


def colorize(x, table, vmin=None, vmax=None, bad_colour=(0, 0, 0)):
    """Items 1 and 2: x fp32 [B,h,w] (fp32 arithmetic) or uint8 [B,h,w] (fp64 arithmetic) -> uint8 RGB [B,h,w,3]."""
    x = np.asarray(x)
    labels = x.dtype == np.uint8
    assert labels or x.dtype == F
    out = np.empty(x.shape + (3,), dtype=np.uint8)
    for b, (lo, hi) in enumerate(_ranges(x, vmin, vmax)):
        lo, hi = F(lo), F(hi)                                    # a range travels as fp32
        idx = index_f64(x[b], lo, hi) if labels else index_f32(x[b], lo, hi)
        out[b] = table[idx]
        if not labels:
            out[b][~np.isfinite(x[b])] = np.asarray(bad_colour, dtype=np.uint8)
    return out


def seg_labels(logits):
    """Item 4: the first index of the maximum over C; a NaN is larger than everything and the first NaN wins.  Written as the loop."""
    logits = np.asarray(logits, dtype=F)
    best, idx = logits[:, 0].copy(), np.zeros(logits[:, 0].shape, dtype=np.uint8)
    for c in range(1, logits.shape[1]):
        v = logits[:, c]
        with np.errstate(invalid="ignore"):
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
        best, idx = np.where(take, v, best), np.where(take, np.uint8(c), idx)
    return idx


def to_rgb(image, image_order="bgr"):
    assert image_order in ("bgr", "rgb")
    return image[..., ::-1] if image_order == "bgr" else image


def grey(rgb):
    """Item 7: the 15-bit fixed point of 0.299 / 0.587 / 0.114, replicated to three channels."""
    v = rgb.astype(np.int64)
    g = ((v[..., 0] * 9798 + v[..., 1] * 19235 + v[..., 2] * 3735 + 16384) >> 15).astype(np.uint8)
    return np.repeat(g[..., None], 3, axis=-1)


def paste(rgb, x, colour):
    """Item 5: the colour where x > 0, the image elsewhere."""
    with np.errstate(invalid="ignore"):
        return np.where((np.asarray(x) > 0)[..., None], colour, rgb)


def blend(rgb, colour, alpha=0.8, beta=0.75):
    """Item 6: three fp32 operations, round half to even, clamp."""
    t = rgb.astype(F) * F(alpha)
    u = colour.astype(F) * F(beta)
    s = t + u
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def overlay(image, x, table, mode="paste", alpha=0.8, beta=0.75, vmin=None, vmax=None, image_order="bgr", bad_colour=(0, 0, 0)):
    rgb = to_rgb(image, image_order)
    colour = colorize(x, table, vmin, vmax, bad_colour)
    return paste(rgb, x, colour) if mode == "paste" else blend(rgb, colour, alpha, beta)


def radar_transform(r):
    r = np.asarray(r, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.where((r != 0) & np.isfinite(r), F(1) - r, F(0)).astype(F)


def dilate(t, k):
    """The k x k maximum over the part of the window inside the frame, t fp32 [B,h,w]."""
    assert k % 2 == 1
    B, h, w = t.shape
    rad = k // 2
    padded = np.full((B, h + 2 * rad, w + 2 * rad), -np.inf, dtype=F)
    padded[:, rad:rad + h, rad:rad + w] = t
    out = np.full(t.shape, -np.inf, dtype=F)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, padded[:, dy:dy + h, dx:dx + w])
    return out


def radar_overlay(image, r, table, k=5, image_order="bgr"):
    """Item 7."""
    d = dilate(radar_transform(r), k)
    return paste(grey(to_rgb(image, image_order)), d, colorize(d, table))


def collage(panels, B, h, w):
    """Item 8's tiling: `panels` maps (row, column) to a [B,h,w,3] picture; missing panels are black."""
    out = np.zeros((B, 2 * h, 3 * w, 3), dtype=np.uint8)
    for (i, j), p in panels.items():
        out[:, i * h:(i + 1) * h, j * w:(j + 1) * w] = p
    return out
