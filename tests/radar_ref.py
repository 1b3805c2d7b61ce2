"""NumPy fp64 restatement of the radar front end (include/camradepth_hip.h: crd_radar_project, crd_radar_rasterize), written from
that contract.  The reference side of each step is lib/fuse_radar.py at the line numbers given.  test_radar_ref_cpu.py ties the
rasteriser to a fixture the reference itself produced (tests/golden/radar_raster.npz); test_gpu_radar.py ties the kernels to this file.

Frames: points of all frames lie in one array, frame b owns offsets[b] .. offsets[b + 1] - 1."""
import numpy as np

PROJ_KEYS = ("x1", "y1", "depth1", "x2", "y2", "v_comp")


def _K(K, b):
    K = np.asarray(K, dtype=np.float64)
    return K[b] if K.ndim == 3 else K


def project(points, sweep_index, offsets, cam1, cam2, lags, K, image_size=(900, 1600), min_distance=1.0, min_z=2.0):
    """-> dict of x1, y1, depth1, x2, y2, v_comp (float64 [N]) and valid (uint8 [N]).  Besides the outputs the dictionary holds
    'margins': per point, the distances of every compared quantity from its threshold (for tests that keep away from them)."""
    pts = np.asarray(points, dtype=np.float64)
    N = len(pts)
    im_h, im_w = float(image_size[0]), float(image_size[1])
    out = {k: np.zeros(N) for k in PROJ_KEYS}
    valid = np.zeros(N, dtype=np.uint8)
    margins = np.full((N, 12), np.inf)
    md, mz = float(np.float32(min_distance)), float(np.float32(min_z))          # the C ABI takes them as float
    with np.errstate(all="ignore"):
        for b in range(len(offsets) - 1):
            Kb = _K(K, b)
            fx, fy, cx, cy = Kb[0, 0], Kb[1, 1], Kb[0, 2], Kb[1, 2]
            for p in range(max(int(offsets[b]), 0), min(int(offsets[b + 1]), N)):
                s = int(sweep_index[p])
                if not 0 <= s < len(lags):
                    continue
                x, y, z, vx, vy = pts[p]
                cams = []
                for M, lag in ((cam1[s], lags[s][0]), (cam2[s], lags[s][1])):
                    xs, ys = x + vx * lag, y + vy * lag                           # :49-50
                    X, Y, Z = (M[r][0] * xs + M[r][1] * ys + M[r][2] * z + M[r][3] for r in range(3))      # :52
                    cams.append(((fx * X + cx * Z) / Z, (fy * Y + cy * Z) / Z, Z))           # :69, view_points(normalize=True)
                (px1, py1, Z1), (px2, py2, Z2) = cams
                out["x1"][p], out["y1"][p], out["depth1"][p], out["x2"][p], out["y2"][p] = px1, py1, Z1, px2, py2
                out["v_comp"][p] = np.sqrt(vx * vx + vy * vy)                     # :65
                ok = not (abs(x) < md and abs(y) < md)                            # :32, remove_close
                for (px, py, Z) in cams:                                          # :68, :73
                    ok = ok and bool(Z >= mz and 0 < px < im_w and 0 < py < im_h)
                valid[p] = ok
                margins[p] = [abs(max(abs(x), abs(y)) - md)] + \
                             [abs(v) for (px, py, Z) in cams for v in (Z - mz, px, px - im_w, py, py - im_h)] + [np.inf]
    out["valid"] = valid
    out["margins"] = margins
    return out


def scaled(v, s, hi):
    """:169-177: the coordinate in the small image, clipped into it."""
    return np.clip((np.asarray(v, dtype=np.float64) + 0.5) / s - 0.5, 0, hi)


def winners(proj, offsets, image_size=(900, 1600), s=2, y_cutoff=34):
    """[(b, r, c, i)]: output pixel (r, c) of frame b goes to point i -- of the points on it the one of smallest depth1, the first of
    equal depths (:185-197: the loop replaces on a strictly smaller depth only).  Skipped: valid == 0, a non-finite value,
    depth1 <= 0 (the reference raises on NaN and takes a zero depth for an empty pixel), rows above the cutoff (:199)."""
    h_new, w_new = int(image_size[0]) // s, int(image_size[1]) // s
    arrs = [np.asarray(proj[k], dtype=np.float64) for k in PROJ_KEYS]
    N = len(arrs[0])
    valid = proj.get("valid")
    xa, ya = scaled(arrs[0], s, w_new - 1), scaled(arrs[1], s, h_new - 1)
    best = {}
    for b in range(len(offsets) - 1):
        for i in range(max(int(offsets[b]), 0), min(int(offsets[b + 1]), N)):
            if valid is not None and not valid[i]:
                continue
            if not all(np.isfinite(a[i]) for a in arrs) or not arrs[2][i] > 0:
                continue
            r, c = int(round(ya[i])) - y_cutoff, int(round(xa[i]))               # :183, half to even
            if r < 0:
                continue
            if (b, r, c) not in best or arrs[2][i] < arrs[2][best[(b, r, c)]]:
                best[(b, r, c)] = i
    return [(b, r, c, i) for (b, r, c), i in sorted(best.items())]


def rasterize64(proj, offsets, K, image_size=(900, 1600), s=2, y_cutoff=34):
    """The non-zero entries before the cast to fp32: [(b, r, c, depth, u, v, rad_vel)] in float64."""
    h_new, w_new = int(image_size[0]) // s, int(image_size[1]) // s
    x1, y1, d1, x2, y2, vc = (np.asarray(proj[k], dtype=np.float64) for k in PROJ_KEYS)
    out = []
    for (b, r, c, i) in winners(proj, offsets, image_size, s, y_cutoff):
        Kb = _K(K, b)
        xa, ya, xb, yb = scaled(x1[i], s, w_new - 1), scaled(y1[i], s, h_new - 1), scaled(x2[i], s, w_new - 1), scaled(y2[i], s, h_new - 1)
        xm = np.float32(np.float64(c) + (xb - xa))                               # :286-287: float32 map += float64 flow, rounded once
        ym = np.float32(np.float64(r) + (yb - ya))
        f, cx, cy = Kb[0, 0] / s, Kb[0, 2] / s, Kb[1, 2] / s - y_cutoff              # :290-292
        u, v = (np.float64(xm) - cx) / f, (np.float64(ym) - cy) / f               # :294-295, fx in both
        out.append((b, r, c, d1[i], u, v, 1.0 if vc[i] > 0.5 else 0.0))          # :202
    return out


def rasterize(proj, offsets, K, image_size=(900, 1600), s=2, y_cutoff=34):
    """-> radar float32 [B, h, w, 3] = (depth, u, v) and rad_vel float32 [B, h, w]; zero where no point landed."""
    B = len(offsets) - 1
    h, w = int(image_size[0]) // s - y_cutoff, int(image_size[1]) // s
    radar, rad_vel = np.zeros((B, h, w, 3), dtype=np.float32), np.zeros((B, h, w), dtype=np.float32)
    for (b, r, c, d, u, v, m) in rasterize64(proj, offsets, K, image_size, s, y_cutoff):
        radar[b, r, c] = (d, u, v)
        rad_vel[b, r, c] = m
    return radar, rad_vel
