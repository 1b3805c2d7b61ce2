"""The bird's-eye-view back end restated in NumPy fp64 from include/camradepth_hip.h (crd_bev_grid), step by step as the header numbers
them.  NumPy rounds every operation on its own, as the kernels do, so the two agree bit for bit.  Shared by the CPU test of this
restatement against a per-point loop and by the GPU tests of the kernels."""
import numpy as np

EMPTY = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def workspace_bytes(B, nx, ny):
    """The header's formula."""
    n_cells = B * nx * ny
    return 2 * ((8 * n_cells + 15) & ~15) + ((4 * n_cells + 15) & ~15)


def frames_of(n_rows, B, frame_offsets=None, rows_per_frame=0):
    """The frame of every row, -1 where it has none."""
    p = np.arange(n_rows, dtype=np.int64)
    if frame_offsets is not None:
        off = np.asarray(frame_offsets, dtype=np.int64)
        b = np.searchsorted(off, p, side="right") - 1              # the b with off[b] <= p < off[b + 1]; empty frames repeat a value
        return np.where((b >= 0) & (b < B), b, -1)
    b = p // rows_per_frame
    return np.where(b < B, b, -1)


def keys_of(Z):
    """The monotone uint64 key of every (finite, canonical) height."""
    u = np.ascontiguousarray(Z, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u ^ np.uint64(1 << 63))


def bev_grid(xyz, B, x_min, y_min, cell, nx, ny, frame_offsets=None, rows_per_frame=0, valid=None, label=None, T=None, z_lo=-np.inf,
             z_hi=np.inf, min_points=1, flip_x=False, flip_y=False):
    """-> {'count', 'z_max', 'z_min', 'top_index', 'occupancy'[, 'top_label']}, each [B, nx, ny]."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    b = frames_of(n, B, frame_offsets, rows_per_frame)
    keep = b >= 0                                                                           # step 1
    if valid is not None:
        keep &= np.asarray(valid).reshape(-1) != 0
    X, Y, Z = x, y, z
    with np.errstate(invalid="ignore", over="ignore"):
        if T is not None:                                                                   # step 2, summed left to right
            T = np.asarray(T, dtype=np.float64)
            Tb = T[np.maximum(b, 0)] if T.ndim == 3 else np.broadcast_to(T, (n, 3, 4))
            X, Y, Z = (Tb[:, i, 0] * x + Tb[:, i, 1] * y + Tb[:, i, 2] * z + Tb[:, i, 3] for i in range(3))
        keep &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)                            # step 3
        Z = Z + 0.0                                                                         # step 4
        keep &= (Z >= z_lo) & (Z <= z_hi)                                                   # step 5
        qx, qy = np.floor((X - x_min) / cell), np.floor((Y - y_min) / cell)                 # step 6
        keep &= (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)                               # step 7, on the doubles
    rows = np.nonzero(keep)[0]
    ix, iy = qx[rows].astype(np.int64), qy[rows].astype(np.int64)
    ix = nx - 1 - ix if flip_x else ix                                                      # step 8
    iy = ny - 1 - iy if flip_y else iy
    cells = (b[rows] * nx + ix) * ny + iy
    n_cells = B * nx * ny
    count = np.bincount(cells, minlength=n_cells).astype(np.int32)
    key = keys_of(Z[rows])
    key_max, key_min = np.zeros(n_cells, dtype=np.uint64), np.full(n_cells, ~np.uint64(0), dtype=np.uint64)
    np.maximum.at(key_max, cells, key)
    np.minimum.at(key_min, cells, key)
    winner = np.full(n_cells, n, dtype=np.int64)
    top = key == key_max[cells]
    np.minimum.at(winner, cells[top], rows[top])
    any_ = count > 0
    height = {}
    for name, k in (("z_max", key_max), ("z_min", key_min)):
        bits = np.where(k >> np.uint64(63) != 0, k ^ np.uint64(1 << 63), ~k)
        with np.errstate(over="ignore", invalid="ignore"):
            height[name] = np.where(any_, bits.view(np.float64).astype(np.float32), EMPTY)
    out = {"count": count, "z_max": height["z_max"], "z_min": height["z_min"],
           "top_index": np.where(any_, winner, -1).astype(np.int32), "occupancy": (count >= min_points).astype(np.uint8)}
    if label is not None:
        lab = np.append(np.asarray(label, dtype=np.uint8).reshape(-1), np.uint8(255))
        out["top_label"] = np.where(any_, lab[np.minimum(winner, n)], 255).astype(np.uint8)
    return {k: v.reshape(B, nx, ny) for k, v in out.items()}
