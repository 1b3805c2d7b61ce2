"""The distance field restated in NumPy from include/camradepth_hip.h (crd_distance_field, crd_field_paths): the two passes as the
header specifies them, the two tables of camradepth_amd.field.tables, and the path check.  Integer arithmetic and look-ups, plus fp64
divide, floor and compare in the path check, which NumPy rounds as the kernels do, so the two agree bit for bit.  Shared by the CPU
test of this restatement against brute-force loops (and scipy's EDT) and by the GPU tests of the kernels."""
import numpy as np


def workspace_bytes(M, nx, ny):
    """The header's formula."""
    return (4 * M * nx * ny + 15) & ~15


def is_source(state, sources):
    """Cell by cell: state < 8 and bit `state` of the mask `sources` set."""
    state = np.asarray(state, np.uint8).astype(np.int64)
    return (state < 8) & (((int(sources) >> np.minimum(state, 7)) & 1) == 1)


def tables(cell, max_cells, inscribed=0.0, inflation=None, scale=10.0):
    """clear_table fp32 and cost_table uint8, each [max_cells^2 + 2], from the squared distance in cells."""
    R = int(max_cells)
    far = R * R + 1
    inflation = R * cell if inflation is None else inflation
    d = np.float64(cell) * np.sqrt(np.arange(far + 1, dtype=np.float64))
    clear = d.astype(np.float32)
    clear[far] = np.inf
    decay = np.floor(252.0 * np.exp(-np.float64(scale) * (d - np.float64(inscribed))))
    cost = np.where(d <= inscribed, 253.0, np.where(d <= inflation, decay, 0.0)).astype(np.uint8)
    cost[0], cost[far] = 254, 0
    return clear, cost


def row_pass(state, sources, R):
    """Launch 1: row_near int32 [M,nx,ny], the nearest source of every cell inside its own row within R, the lower of two; -1."""
    src = is_source(state, sources)
    ny = src.shape[-1]
    j = np.broadcast_to(np.arange(ny, dtype=np.int64), src.shape)
    none = 1 << 40
    below = np.maximum.accumulate(np.where(src, j, -none), axis=-1)                          # the last source at or before j
    above = np.minimum.accumulate(np.where(src, j, none)[..., ::-1], axis=-1)[..., ::-1]      # the first source at or behind j
    d_below, d_above = j - below, above - j
    near = np.where(d_below <= d_above, below, above)
    return np.where(np.minimum(d_below, d_above) <= R, near, -1).astype(np.int32)


def column_pass(row_near, R):
    """Launch 2: (dist2, nearest), int32 [M,nx,ny], from the rows i - R .. i + R of every column; the lowest row among equal t."""
    row_near = np.asarray(row_near, np.int64)
    M, nx, ny = row_near.shape
    far = R * R + 1
    j = np.broadcast_to(np.arange(ny, dtype=np.int64), row_near.shape)
    g2 = np.where(row_near >= 0, (j - row_near) ** 2, far)
    i = np.arange(nx, dtype=np.int64)[None, :, None]
    best = np.full((M, nx, ny), far, np.int64)
    nearest = np.full((M, nx, ny), -1, np.int64)
    for d in range(-min(R, nx - 1), min(R, nx - 1) + 1):                                       # i' = i + d ascending: strictly less keeps the lowest
        lo, hi = max(0, -d), min(nx, nx - d)                                                  # the rows i with 0 <= i + d < nx
        t = d * d + g2[:, lo + d:hi + d]
        take = (t < best[:, lo:hi]) & (t <= R * R)
        best[:, lo:hi] = np.where(take, t, best[:, lo:hi])
        nearest[:, lo:hi] = np.where(take, (i[:, lo:hi] + d) * ny + row_near[:, lo + d:hi + d], nearest[:, lo:hi])
    return best.astype(np.int32), nearest.astype(np.int32)


def distance_field(state, sources, R, unknown_cost, clear_table, cost_table):
    """crd_distance_field -> 'row_near' (the workspace), 'dist2', 'nearest', 'clearance', 'cost'."""
    state = np.asarray(state, np.uint8)
    row_near = row_pass(state, sources, R)
    dist2, nearest = column_pass(row_near, R)
    cost = np.asarray(cost_table, np.uint8)[dist2]
    if unknown_cost > 0:
        cost = np.where((state == 0) & (cost < unknown_cost), np.uint8(unknown_cost), cost)
    return {"row_near": row_near, "dist2": dist2, "nearest": nearest, "clearance": np.asarray(clear_table, np.float32)[dist2],
            "cost": cost.astype(np.uint8)}


def check_paths(xy, n_poses, path_map, origin, cell, state, dist2, cost, R, blocked_at=253, outside_blocks=True):
    """crd_field_paths -> 'first_blocked', 'max_cost', 'min_dist2', 'n_outside', 'n_unknown' [K] and 'pose_cell' [K,P]."""
    xy = np.asarray(xy, np.float64)
    K, P = xy.shape[:2]
    M, nx, ny = state.shape
    far = R * R + 1
    n = np.full(K, P, np.int64) if n_poses is None else np.clip(np.asarray(n_poses, np.int64), 0, P)
    m = np.zeros(K, np.int64) if path_map is None else np.asarray(path_map, np.int64)
    has_map = (m >= 0) & (m < M)
    ms = np.where(has_map, m, 0)
    origin = np.asarray(origin, np.int64)
    ox, oy = origin[ms, 0][:, None], origin[ms, 1][:, None]
    X, Y = xy[..., 0], xy[..., 1]
    with np.errstate(all="ignore"):
        wx, wy = np.floor(X / np.float64(cell)), np.floor(Y / np.float64(cell))
        inside = has_map[:, None] & np.isfinite(X) & np.isfinite(Y) & (wx >= ox.astype(np.float64)) & (wx < (ox + nx).astype(np.float64)) & \
            (wy >= oy.astype(np.float64)) & (wy < (oy + ny).astype(np.float64))
    counts = np.arange(P)[None, :] < n[:, None]
    inside &= counts
    i = np.where(inside, wx, 0).astype(np.int64) - np.where(inside, ox, 0)
    j = np.where(inside, wy, 0).astype(np.int64) - np.where(inside, oy, 0)
    c = i * ny + j
    flat = ms[:, None] * nx * ny + c
    cost_at = np.where(inside, cost.reshape(-1)[flat].astype(np.int64), 0)
    d2_at = np.where(inside, dist2.reshape(-1)[flat].astype(np.int64), far)
    unknown = inside & (state.reshape(-1)[flat] == 0)
    outside = counts & ~inside
    blocked = (inside & (cost_at >= blocked_at)) | (outside & bool(outside_blocks))
    first = np.where(blocked.any(axis=1), blocked.argmax(axis=1), -1)
    return {"first_blocked": first.astype(np.int32), "max_cost": cost_at.max(axis=1).astype(np.uint8), "min_dist2": d2_at.min(axis=1).astype(np.int32),
            "n_outside": outside.sum(axis=1).astype(np.int32), "n_unknown": unknown.sum(axis=1).astype(np.int32),
            "pose_cell": np.where(counts, np.where(inside, c, -1), -2).astype(np.int32)}
