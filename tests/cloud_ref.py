"""NumPy fp64 restatement of the point-cloud back end (include/camradepth_hip.h: crd_depth_unproject, crd_point_cloud), written from
that contract operation for operation and vectorised over pixels.  test_cloud_ref_cpu.py ties it to the lidar restatement
(tests/lidar_ref.py) and to the dataloader's encoding; test_gpu_cloud.py ties the kernels to this file, bit for bit."""
import numpy as np


def _per_frame(M, B, shape):
    """One matrix for all frames, or one per frame -> [B, *shape]."""
    M = np.asarray(M, dtype=np.float64)
    return M if M.ndim == len(shape) + 1 else np.broadcast_to(M, (B,) + shape)


def unproject(depth, K, s=2, y_cutoff=34, max_depth=100.0, encoding="inverse", T=None, min_range=0.0, max_range=np.inf,
              skip_empty=False, mask=None, labels=None, keep=None):
    """depth float32 [B, h, w] -> points float32 [B, h, w, 3], valid uint8 [B, h, w].  keep: a collection of class ids or a table of
    256 entries."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 3
    B, h, w = depth.shape
    p = depth.astype(np.float64)
    with np.errstate(all="ignore"):
        d = max_depth * (1.0 - p) if encoding == "inverse" else p                         # 1.
        valid = np.isfinite(p) & (d > 0) & (d >= min_range) & (d <= max_range)
        valid &= ~((p == 0) & bool(skip_empty)) if encoding == "inverse" else p > 0
        if mask is not None:
            valid &= np.asarray(mask) != 0
        if labels is not None:
            table = np.asarray(keep)
            if table.shape != (256,):
                table = np.zeros(256, dtype=np.uint8)
                table[list(keep)] = 1
            valid &= table[np.asarray(labels)] != 0
        r, c = np.arange(h, dtype=np.float64)[None, :, None], np.arange(w, dtype=np.float64)[None, None, :]
        xf = (c + 0.5) * s - 0.5                                                          # 2.
        yf = ((r + y_cutoff) + 0.5) * s - 0.5
        Kb = _per_frame(K, B, (3, 3))
        fx, cx, fy, cy = (Kb[:, i, j][:, None, None] for i, j in ((0, 0), (0, 2), (1, 1), (1, 2)))
        X, Y, Z = ((xf - cx) / fx) * d, ((yf - cy) / fy) * d, d                           # 3.
        if T is not None:                                                                 # 4.
            Tb = _per_frame(T, B, (3, 4))[:, :, :, None, None]
            X, Y, Z = (((Tb[:, i, 0] * X + Tb[:, i, 1] * Y) + Tb[:, i, 2] * Z) + Tb[:, i, 3] for i in range(3))
        points = np.stack([X, Y, Z], axis=-1).astype(np.float32)                          # 5.
    points[~valid] = 0.0
    return points, valid.astype(np.uint8)


def point_cloud(depth, K, s=2, y_cutoff=34, stride=1, image=None, labels=None, **kw):
    """-> {'xyz' float32 [n, 3], 'frame_offsets' int32 [B + 1], 'pixel' int32 [n][, 'rgb' uint8 [n, 3]][, 'label' uint8 [n]]}: the valid
    candidates (r % stride == 0 and c % stride == 0) in (b, r, c) order; n = frame_offsets[B]."""
    points, valid = unproject(depth, K, s, y_cutoff, labels=labels, **kw)
    B, h, w = valid.shape
    cand = np.zeros((h, w), dtype=bool)
    cand[::stride, ::stride] = True
    b, r, c = np.nonzero((valid != 0) & cand[None])                                       # row-major: (b, r, c) ascending
    out = {"xyz": points[b, r, c], "pixel": (r * w + c).astype(np.int32),
           "frame_offsets": np.concatenate([[0], np.cumsum(np.bincount(b, minlength=B))]).astype(np.int32)}
    if image is not None:
        out["rgb"] = np.asarray(image)[b, r, c]
    if labels is not None:
        out["label"] = np.asarray(labels)[b, r, c]
    return out
