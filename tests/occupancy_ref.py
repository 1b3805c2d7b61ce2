"""The occupancy map restated in NumPy fp64 from include/camradepth_hip.h (crd_occupancy_update), launch by launch as the header
describes them.  NumPy rounds every operation on its own, as the kernels do, so the two agree bit for bit.  Shared by the CPU test of
this restatement against per-point and per-cell loops and by the GPU tests of the kernels.

`params` are the numbers of an OccupancyMap (PARAMS holds the keys); `state` is the caller's state as new_state() makes it, changed in
place by update()."""
import numpy as np

from tests.bev_ref import frames_of

PARAMS = ("M", "nx", "ny", "cell", "n_bins", "max_range", "z_floor", "z_lo", "z_hi", "min_points", "l_occ", "l_free", "l_max", "occupied_at",
          "free_at")
ORIGIN_LIMIT = 2.0 ** 31 - 65536
INF_BITS = np.uint64(0x7ff0000000000000)


def workspace_bytes(B, n_bins, M, nx, ny):
    """The header's formula."""
    return 2 * ((8 * B * n_bins + 15) & ~15) + ((24 * B + 15) & ~15) + ((4 * M * nx * ny + 15) & ~15) + ((4 * M + 15) & ~15)


def new_state(params):
    M, nx, ny = params["M"], params["nx"], params["ny"]
    return {"map": np.zeros((M, nx, ny), np.int16), "prev_origin": np.zeros((M, 2), np.int64), "cur_origin": np.zeros((M, 2), np.int64),
            "initialised": np.zeros(M, np.int32), "status": np.zeros(M, np.int32)}


def bins_of(dx, dy, n_bins):
    """The bin of every direction; 0 where the rule is not defined (both zero, or not finite), which no caller uses."""
    q_bins = n_bins // 4
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    ax, ay = np.abs(dx), np.abs(dy)
    first = ax >= ay
    with np.errstate(all="ignore"):
        s = np.where(first, dy / ax, dx / ay)
        face = np.where(first, np.where(dx > 0, 0, 2), np.where(dy > 0, 1, 3))
        q = np.minimum(np.floor(((s + 1.0) * 0.5) * np.float64(q_bins)), np.float64(q_bins - 1))
    q = np.where(np.isfinite(q), q, 0.0)
    return face * q_bins + q.astype(np.int64)


def transformed(T, b, v):
    """T_b . v for every row: T None, [3,4] or [B,3,4]; b the frame of every row; v [n,3]."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    if T is None:
        return x, y, z
    T = np.asarray(T, np.float64)
    Tb = T[b] if T.ndim == 3 else np.broadcast_to(T, (len(b), 3, 4))
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(Tb[:, i, 0] * x + Tb[:, i, 1] * y + Tb[:, i, 2] * z + Tb[:, i, 3] for i in range(3))      # summed left to right


def per_frame(v, B):
    """sensor or centre: None (the origin), [3] or [B,3] -> [B,3]."""
    if v is None:
        return np.zeros((B, 3))
    v = np.asarray(v, np.float64)
    return np.ascontiguousarray(np.broadcast_to(v, (B, 3)))


def update(params, state, xyz, B, frame_offsets=None, rows_per_frame=0, valid=None, T=None, sensor=None, centre=None):
    """-> {'log_odds', 'state', 'evidence', 'value' [M,nx,ny], 'origin' [M,2]}; `state` is updated in place.  'hits', 'hit_min' and
    'seen_max' (the workspace after launch 2) come along for the tests of this restatement."""
    p = params
    M, nx, ny, cell, n_bins = p["M"], p["nx"], p["ny"], np.float64(p["cell"]), p["n_bins"]
    assert M in (B, 1)
    max_r2 = np.float64(p["max_range"]) * np.float64(p["max_range"])
    frames = np.arange(B)
    map_of = np.zeros(B, np.int64) if M == 1 else frames
    # launch 1: the sensors, the windows
    S = np.stack(transformed(T, frames, per_frame(sensor, B)), axis=1)
    for b in frames[~np.isfinite(S).all(axis=1)]:
        state["status"][map_of[b]] |= 2
    fed_by = np.zeros(M, np.int64) if M == 1 else np.arange(M)
    C = np.stack(transformed(T, fed_by, per_frame(sensor if centre is None else centre, B)[fed_by]), axis=1)
    with np.errstate(all="ignore"):
        f = np.floor(C[:, :2] / cell)
        moved = np.isfinite(C).all(axis=1) & (np.abs(f) < ORIGIN_LIMIT).all(axis=1)
    live = state["initialised"] != 0
    for m in range(M):
        if moved[m]:
            state["prev_origin"][m] = state["cur_origin"][m]
            state["cur_origin"][m] = (int(f[m, 0]) - nx // 2, int(f[m, 1]) - ny // 2)
        else:
            state["status"][m] |= 1
    cur, prev = state["cur_origin"], state["prev_origin"]
    # launch 2: the rows
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    b = frames_of(n, B, frame_offsets, rows_per_frame)
    keep = b >= 0                                                                            # step 1
    if valid is not None:
        keep &= np.asarray(valid).reshape(-1) != 0
    bb = np.maximum(b, 0)
    X, Y, Z = transformed(T, bb, xyz.astype(np.float64))                                     # step 2
    keep &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & np.isfinite(S[bb]).all(axis=1)
    with np.errstate(all="ignore"):
        dx, dy = X - S[bb, 0], Y - S[bb, 1]                                                  # step 3
        r2 = dx * dx + dy * dy
        keep &= (r2 > 0) & (r2 <= max_r2)
        k = bb * n_bins + bins_of(dx, dy, n_bins)
        seen = keep & (Z >= p["z_floor"]) & (Z <= p["z_hi"])                                 # step 4
        hit = keep & (Z >= p["z_lo"]) & (Z <= p["z_hi"])                                     # step 5
        wx, wy = np.floor(X / cell), np.floor(Y / cell)
        m_of = map_of[bb]
        ox, oy = cur[m_of, 0], cur[m_of, 1]
        inside = hit & (wx >= ox.astype(np.float64)) & (wx < (ox + nx).astype(np.float64)) & (wy >= oy.astype(np.float64)) & \
            (wy < (oy + ny).astype(np.float64))
    bits = np.ascontiguousarray(r2).view(np.uint64)
    seen_max, hit_min = np.zeros(B * n_bins, np.uint64), np.full(B * n_bins, INF_BITS, np.uint64)
    np.maximum.at(seen_max, k[seen], bits[seen])
    np.minimum.at(hit_min, k[hit], bits[hit])
    at = (m_of[inside] * nx + (wx[inside].astype(np.int64) - ox[inside])) * ny + (wy[inside].astype(np.int64) - oy[inside])
    hits = np.bincount(at, minlength=M * nx * ny).astype(np.int32).reshape(M, nx, ny)
    first, far = hit_min.view(np.float64).reshape(B, n_bins), seen_max.view(np.float64).reshape(B, n_bins)
    # launch 3: the cells
    out = {"log_odds": np.zeros((M, nx, ny), np.int16), "state": np.zeros((M, nx, ny), np.uint8), "evidence": np.zeros((M, nx, ny), np.uint8)}
    for m in range(M):
        wx, wy = cur[m, 0] + np.arange(nx, dtype=np.int64), cur[m, 1] + np.arange(ny, dtype=np.int64)
        slot = (wx % nx)[:, None], (wy % ny)[None, :]                                       # the mathematical modulo
        stored = state["map"][m][slot].astype(np.int64)
        if not moved[m]:
            new = stored if live[m] else np.zeros_like(stored)
            out["log_odds"][m] = new
            out["state"][m] = np.where(new >= p["occupied_at"], 2, np.where(new <= -p["free_at"], 1, 0))
            continue
        was_there = ((wx >= prev[m, 0]) & (wx < prev[m, 0] + nx))[:, None] & ((wy >= prev[m, 1]) & (wy < prev[m, 1] + ny))[None, :]
        old = np.where(was_there, stored, 0) if live[m] else np.zeros_like(stored)
        cx, cy = (wx.astype(np.float64) + 0.5) * cell, (wy.astype(np.float64) + 0.5) * cell
        free = np.zeros((nx, ny), bool)
        for fb in (frames if M == 1 else [m]):
            with np.errstate(all="ignore"):
                dx = np.broadcast_to((cx - S[fb, 0])[:, None], (nx, ny))
                dy = np.broadcast_to((cy - S[fb, 1])[None, :], (nx, ny))
                r2c = dx * dx + dy * dy
                kc = bins_of(dx, dy, n_bins)
                free |= (r2c > 0) & (r2c < first[fb][kc]) & (r2c <= far[fb][kc])
        ev = np.where(hits[m] >= p["min_points"], 2, np.where(free, 1, 0))
        new = np.clip(old + np.where(ev == 2, p["l_occ"], np.where(ev == 1, -p["l_free"], 0)), -p["l_max"], p["l_max"])
        state["map"][m][slot] = new.astype(np.int16)
        state["initialised"][m] = 1
        out["log_odds"][m] = new
        out["evidence"][m] = ev
        out["state"][m] = np.where(new >= p["occupied_at"], 2, np.where(new <= -p["free_at"], 1, 0))
    out["value"] = out["log_odds"].astype(np.float32)
    out["origin"] = cur.copy()
    out.update(hits=hits, hit_min=hit_min.reshape(B, n_bins), seen_max=seen_max.reshape(B, n_bins))
    return out
