"""NumPy fp64 restatement of the lidar ground-truth front end (include/camradepth_hip.h: crd_lidar_project, crd_lidar_ground_truth),
written from that contract and vectorised over points and pixels.  The reference side of each step is lib/fuse_lidar.py at the line
numbers given.  test_lidar_ref_cpu.py ties the ground-truth stage to a fixture the reference itself produced
(tests/golden/lidar_gt.npz) and both stages to plain sequential loops; test_gpu_lidar.py ties the kernels to this file.

Frames: points of all frames lie in one array, frame b owns offsets[b] .. offsets[b + 1] - 1."""
import numpy as np

PROJ_KEYS = ("x1", "y1", "depth1", "x2", "y2")
FLAG_KEYS = ("low_h", "in_box", "valid")


def _K(K, b):
    K = np.asarray(K, dtype=np.float64)
    return K[b] if K.ndim == 3 else K[None].repeat(len(b), axis=0)


def frame_of(offsets, N):
    """The frame of every point 0 .. N - 1, or -1."""
    off = np.asarray(offsets, dtype=np.int64)
    j = np.searchsorted(off, np.arange(N), side="right")            # the first j with off[j] > p
    return np.where((j == 0) | (j == len(off)), -1, j - 1)


def rigid(M, p):
    """M . (x, y, z, 1) for 3 x 4 matrices M [..., 12] and points p [n, 3], the sums from left to right."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([M[..., 4 * r] * x + M[..., 4 * r + 1] * y + M[..., 4 * r + 2] * z + M[..., 4 * r + 3] for r in range(3)], axis=1)


def project(points, sweep_index, offsets, cam1, cam2, car_z, K, sweep_boxes=None, entries=None, box_id=None, cam1_box=None, cam2_box=None,
            vehicle=None, image_size=(900, 1600), min_distance=2.5, min_z=2.0, h_min=0.3, h_max=2.0):
    """-> dict of x1, y1, depth1, x2, y2 (float64 [N]), low_h, in_box, valid (uint8 [N]) and box_entry (int32 [N]).  Besides the outputs
    the dictionary holds 'margin': per point, the smallest distance of a compared quantity from its threshold (box faces of every
    entry of its sweep, both heights, the min_distance square, min_z, the image borders), for tests that keep away from them."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    N = len(pts)
    sw = np.asarray(sweep_index, dtype=np.int64)
    S = len(cam1)
    cam1, cam2 = np.asarray(cam1, dtype=np.float64).reshape(S, 12), np.asarray(cam2, dtype=np.float64).reshape(S, 12)
    car_z = np.asarray(car_z, dtype=np.float64).reshape(S, 4)
    E = 0 if entries is None else len(entries)
    sweep_boxes = np.zeros(S + 1, dtype=np.int64) if sweep_boxes is None else np.asarray(sweep_boxes, dtype=np.int64)
    im_h, im_w = float(image_size[0]), float(image_size[1])
    md, mz = float(np.float32(min_distance)), float(np.float32(min_z))          # the C ABI takes them as float
    b = frame_of(offsets, N)
    good = (b >= 0) & (sw >= 0) & (sw < S)
    hit = np.full(N, -1, dtype=np.int64)
    q_hit = np.zeros((N, 3))
    margin = np.full(N, np.inf)
    with np.errstate(all="ignore"):
        for s in range(S):                                            # per sweep and entry; every step is over all its points
            idx = np.nonzero(good & (sw == s))[0]
            for e in range(max(int(sweep_boxes[s]), 0), min(int(sweep_boxes[s + 1]), E)):
                ent = np.asarray(entries[e], dtype=np.float64)
                q = rigid(ent[:12], pts[idx])
                inside = (np.abs(q) < ent[12:15]).all(axis=1)         # :132-137, six strict inequalities
                new = inside & (hit[idx] < 0)                         # the first entry that holds the point keeps it
                hit[idx[new]], q_hit[idx[new]] = e, q[new]
                margin[idx] = np.minimum(margin[idx], np.abs(np.abs(q) - ent[12:15]).min(axis=1))
        k = np.where(hit >= 0, np.asarray(box_id, dtype=np.int64)[np.maximum(hit, 0)] if E else -1, -1)
        n_boxes = 0 if cam1_box is None else len(cam1_box)
        good &= ~((hit >= 0) & ((k < 0) | (k >= n_boxes)))
        hit[~good] = -1
        boxed = good & (hit >= 0)
        s_ = np.where(good, sw, 0)
        k_ = np.where(boxed, k, 0)
        zc = car_z[s_, 0] * pts[:, 0] + car_z[s_, 1] * pts[:, 1] + car_z[s_, 2] * pts[:, 2] + car_z[s_, 3]
        low = good & (zc >= h_min) & (zc <= h_max)                    # :54
        cams = []
        for cs, cb in ((cam1, cam1_box), (cam2, cam2_box)):
            X = rigid(cs[s_], pts)
            if n_boxes:
                X = np.where(boxed[:, None], rigid(np.asarray(cb, dtype=np.float64).reshape(n_boxes, 12)[k_], q_hit), X)
            cams.append(X)
        Kb = _K(K, np.maximum(b, 0))
        fx, fy, cx, cy = Kb[:, 0, 0], Kb[:, 1, 1], Kb[:, 0, 2], Kb[:, 1, 2]
        out, ok = {}, good & ~((np.abs(pts[:, 0]) < md) & (np.abs(pts[:, 1]) < md))          # remove_close
        margin = np.minimum(margin, np.abs(np.maximum(np.abs(pts[:, 0]), np.abs(pts[:, 1])) - md))
        margin = np.minimum(margin, np.minimum(np.abs(zc - h_min), np.abs(zc - h_max)))
        for X, (kx, ky, kd) in zip(cams, (("x1", "y1", "depth1"), ("x2", "y2", None))):
            px, py, Z = (fx * X[:, 0] + cx * X[:, 2]) / X[:, 2], (fy * X[:, 1] + cy * X[:, 2]) / X[:, 2], X[:, 2]      # :176
            ok &= (Z >= mz) & (px > 0) & (px < im_w) & (py > 0) & (py < im_h)                                          # :175-178
            for v in (Z - mz, px, px - im_w, py, py - im_h):
                margin = np.minimum(margin, np.abs(v))
            out[kx], out[ky] = np.where(good, px, 0.0), np.where(good, py, 0.0)
            if kd:
                out[kd] = np.where(good, Z, 0.0)
    out["low_h"], out["valid"] = low.astype(np.uint8), ok.astype(np.uint8)
    out["in_box"] = (boxed & (np.asarray(vehicle)[k_] != 0 if n_boxes else False)).astype(np.uint8)
    out["box_entry"] = hit.astype(np.int32)
    out["margin"] = np.where(good, margin, np.inf)
    return out


def scaled(v, s, hi):
    """:293-301: the coordinate in the small image, clipped into it."""
    return np.clip((np.asarray(v, dtype=np.float64) + 0.5) / s - 0.5, 0, hi)


def winners(proj, offsets, image_size=(900, 1600), s=2, y_cutoff=34):
    """-> (b, r, c, i): output pixel (r, c) of frame b goes to point i -- of the points on it the one of smallest depth1, the lowest
    index among equal depths (:308-317 replace on a strictly smaller depth only).  Skipped: valid == 0, a non-finite value, depth1 <= 0,
    rows above the cutoff (:319).  One sort by (pixel, depth, index); the first of every pixel's run is its winner."""
    h_new, w_new = int(image_size[0]) // s, int(image_size[1]) // s
    arrs = [np.asarray(proj[k], dtype=np.float64) for k in PROJ_KEYS]
    N = len(arrs[0])
    b = frame_of(offsets, N)
    with np.errstate(invalid="ignore"):
        ok = (b >= 0) & np.isfinite(np.stack(arrs)).all(axis=0) & (arrs[2] > 0)
        if proj.get("valid") is not None:
            ok &= np.asarray(proj["valid"]) != 0
        i = np.nonzero(ok)[0]
        col = np.rint(scaled(arrs[0][i], s, w_new - 1)).astype(np.int64)              # :305, half to even
        row = np.rint(scaled(arrs[1][i], s, h_new - 1)).astype(np.int64) - y_cutoff
    keep = row >= 0
    i, row, col = i[keep], row[keep], col[keep]
    pix = (b[i] * (h_new - y_cutoff) + row) * w_new + col
    order = np.lexsort((i, arrs[2][i], pix))
    first = np.ones(len(order), dtype=bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    w = order[first]
    return b[i][w], row[w], col[w], i[w]


def rectangles(corners, s, y_cutoff, h, w):
    """[(x0, x1, y0, y1, d_max)] per box of corners [n, 8, 4] = x, y, depth, in_view (:650-668); x0 > x1 for a box that does nothing."""
    out = []
    for c in np.asarray(corners, dtype=np.float64).reshape(-1, 8, 4):
        m = c[:, 3] != 0
        with np.errstate(invalid="ignore"):
            d_max = c[:, 2].max()                                                      # all eight, in view or not (:665)
        if not m.any() or not np.isfinite(c[m, :2]).all():
            out.append((1, 0, 1, 0, d_max))
            continue
        xs = np.clip((c[m, 0] + 0.5) / s - 0.5, 0, w - 1)
        ys = np.clip(((c[m, 1] + 0.5) / s - 0.5) - y_cutoff, 0, h - 1)
        out.append((int(np.rint(xs.min())), int(np.rint(xs.max())), int(np.rint(ys.min())), int(np.rint(ys.max())), d_max))
    return out


def ground_truth64(proj, offsets, K, image_size=(900, 1600), s=2, y_cutoff=34, seg=None, corners=None, corner_offsets=None, flow_im=None,
                   thres=3.0):
    """The entries that are left, before the cast to fp32: float64 [n, 7] = b, r, c, depth, u, v, low_h."""
    h_new, w_new = int(image_size[0]) // s, int(image_size[1]) // s
    h = h_new - y_cutoff
    x1, y1, d1, x2, y2 = (np.asarray(proj[k], dtype=np.float64) for k in PROJ_KEYS)
    b, r, c, i = winners(proj, offsets, image_size, s, y_cutoff)
    d = d1[i]
    keep = np.ones(len(i), dtype=bool)
    if seg is not None:                                                                # :672, the union over the frame's boxes
        free = (np.asarray(seg)[b, r, c] != 0) & (np.asarray(proj["in_box"])[i] == 0)
        frame = frame_of(corner_offsets, len(np.asarray(corners).reshape(-1, 8, 4)))
        for (x0, x1_, y0, y1_, d_max), fb in zip(rectangles(corners, s, y_cutoff, h, w_new), frame):
            with np.errstate(invalid="ignore"):
                keep &= ~(free & (b == fb) & (c >= x0) & (c <= x1_) & (r >= y0) & (r <= y1_) & (d > d_max))
    fx_ = scaled(x2[i], s, w_new - 1) - scaled(x1[i], s, w_new - 1)                    # :310
    fy_ = scaled(y2[i], s, h_new - 1) - scaled(y1[i], s, h_new - 1)
    if flow_im is not None:                                                            # :557-560
        fi = np.asarray(flow_im)[b, r, c].astype(np.float64)
        ex, ey = fx_ - fi[:, 0], fy_ - fi[:, 1]
        with np.errstate(invalid="ignore"):
            keep &= ~(np.sqrt(ex * ex + ey * ey) > thres)
    xm = (c.astype(np.float64) + fx_).astype(np.float32)                               # :581-582: float32 map += float64 flow, rounded once
    ym = (r.astype(np.float64) + fy_).astype(np.float32)
    Kb = _K(K, b)
    f, cx, cy = Kb[:, 0, 0] / s, Kb[:, 0, 2] / s, Kb[:, 1, 2] / s - y_cutoff            # :585-587
    u, v = (xm.astype(np.float64) - cx) / f, (ym.astype(np.float64) - cy) / f          # :589-590, fx in both
    out = np.stack([b.astype(np.float64), r.astype(np.float64), c.astype(np.float64), d, u, v,
                    (np.asarray(proj["low_h"])[i] != 0).astype(np.float64)], axis=1)
    return out[keep]


def ground_truth(proj, offsets, K, image_size=(900, 1600), s=2, y_cutoff=34, **filters):
    """-> gt float32 [B, h, w, 3] = (depth, u, v), depth float32 [B, h, w], msk_lh uint8 [B, h, w]; zero where nothing is left."""
    B = len(offsets) - 1
    h, w = int(image_size[0]) // s - y_cutoff, int(image_size[1]) // s
    gt, msk = np.zeros((B, h, w, 3), dtype=np.float32), np.zeros((B, h, w), dtype=np.uint8)
    e = ground_truth64(proj, offsets, K, image_size, s, y_cutoff, **filters)
    b, r, c = (e[:, j].astype(np.int64) for j in range(3))
    gt[b, r, c] = e[:, 3:6].astype(np.float32)
    msk[b, r, c] = e[:, 6].astype(np.uint8)
    return gt, np.ascontiguousarray(gt[..., 0]), msk
