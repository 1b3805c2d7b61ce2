"""The scan matcher restated in NumPy fp64 from include/camradepth_hip.h (crd_match_scan).  NumPy rounds every operation on its own,
as the kernels do, and the score is a sum of integers, so the two agree bit for bit.  Shared by the CPU tests of this restatement
(a plain loop, planted offsets, invariants) and by the GPU tests of the kernels.

`params` and `state` are those of tests/occupancy_ref.py (the state is only read); `spec` holds n_xy, n_theta, d_theta, min_points
(None: the map's), min_cells and min_score."""
import math

import numpy as np

from tests.bev_ref import frames_of
from tests.occupancy_ref import per_frame, transformed

UNINITIALISED, NOT_FINITE, FEW_CELLS, LOW_SCORE, ON_BORDER = 1, 2, 4, 8, 16
KEEPS_PRIOR = 15
OUT = ("pose", "pick", "score", "prior_score", "n_cells", "status")
SPEC = dict(n_xy=4, n_theta=4, d_theta=math.radians(0.25), min_points=None, min_cells=8, min_score=1)


def spec(**changes):
    return dict(SPEC, **changes)


def workspace_bytes(B, M, nx, ny, n_xy, n_theta):
    """The header's formula."""
    nt, ns = 2 * n_theta + 1, 2 * n_xy + 1
    return ((96 * B * nt + 15) & ~15) + ((24 * B + 15) & ~15) + ((4 * M * nt * (nx + 2 * n_xy) * (ny + 2 * n_xy) + 15) & ~15) + \
        ((8 * M * nt * ns * ns + 15) & ~15)


def rot_table(n_theta, d_theta):
    """[2 n_theta + 1, 2]: (cos, sin) by math.cos and math.sin; the centre row is exactly (1, 0)."""
    return np.array([(1.0, 0.0) if t == n_theta else (math.cos((t - n_theta) * d_theta), math.sin((t - n_theta) * d_theta))
                     for t in range(2 * n_theta + 1)], np.float64)


def poses_of(T, B):
    """None (the identity), [3,4] or [B,3,4] -> [B,3,4]."""
    if T is None:
        T = np.eye(3, 4)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(T, np.float64), (B, 3, 4)))


def candidate_poses(T, S, rot, n_theta):
    """T [B,3,4], S [B,3] (the point every frame is turned about) -> T' [B,NT,3,4]."""
    B, nt = T.shape[0], rot.shape[0]
    out = np.empty((B, nt, 3, 4))
    with np.errstate(all="ignore"):
        for t in range(nt):
            c, s = rot[t]
            out[:, t] = T
            if t == n_theta:
                continue
            out[:, t, 0, :3] = c * T[:, 0, :3] - s * T[:, 1, :3]
            out[:, t, 1, :3] = s * T[:, 0, :3] + c * T[:, 1, :3]
            out[:, t, 0, 3] = (c * T[:, 0, 3] - s * T[:, 1, 3]) + (S[:, 0] - (c * S[:, 0] - s * S[:, 1]))
            out[:, t, 1, 3] = (s * T[:, 0, 3] + c * T[:, 1, 3]) + (S[:, 1] - (s * S[:, 0] + c * S[:, 1]))
    return out


def better(a, b, n_theta):
    """a, b: (score, t, dx, dy).  The header's order."""
    def key(c):
        return (-c[0], c[2] * c[2] + c[3] * c[3], abs(c[1] - n_theta), c[1], c[2], c[3])
    return key(a) < key(b)


def pick_of(table, n_xy, n_theta):
    """table [NT,NS,NS] -> (score, t, dx, dy), the least in the header's order."""
    best = None
    for t in range(table.shape[0]):
        for ix in range(table.shape[1]):
            for iy in range(table.shape[2]):
                c = (int(table[t, ix, iy]), t, ix - n_xy, iy - n_xy)
                if best is None or better(c, best, n_theta):
                    best = c
    return best


def window_log_odds(params, state, m):
    """The log-odds of map m in WINDOW order, int64 [nx,ny]; zeros when the map is not initialised."""
    nx, ny = params["nx"], params["ny"]
    if state["initialised"][m] == 0:
        return np.zeros((nx, ny), np.int64)
    ox, oy = state["cur_origin"][m]
    wx, wy = ox + np.arange(nx, dtype=np.int64), oy + np.arange(ny, dtype=np.int64)
    return state["map"][m][(wx % nx)[:, None], (wy % ny)[None, :]].astype(np.int64)


def obstacle_rows(params, xyz, B, frame_offsets, rows_per_frame, valid, T, S):
    """Steps 1 to 3 of the update's launch 2 and the hit test -> (the frame of every row, clipped to 0; the rows that are obstacle rows)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    b = frames_of(xyz.shape[0], B, frame_offsets, rows_per_frame)
    keep = b >= 0
    if valid is not None:
        keep &= np.asarray(valid).reshape(-1) != 0
    bb = np.maximum(b, 0)
    X, Y, Z = transformed(T, bb, xyz.astype(np.float64))
    keep &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & np.isfinite(S[bb]).all(axis=1)
    with np.errstate(all="ignore"):
        dx, dy = X - S[bb, 0], Y - S[bb, 1]
        r2 = dx * dx + dy * dy
        max_r2 = np.float64(params["max_range"]) * np.float64(params["max_range"])
        keep &= (r2 > 0) & (r2 <= max_r2) & (Z >= params["z_lo"]) & (Z <= params["z_hi"])
    return bb, keep


def match_scan(params, state, spec, xyz, B, frame_offsets=None, rows_per_frame=0, valid=None, T=None, sensor=None):
    """-> {'pose' [B,3,4], 'pick' [M,3], 'score', 'prior_score', 'n_cells', 'status' [M], 'scores' [M,NT,NS,NS]}; 'counts', int32
    [M,NT,nx + 2 n_xy,ny + 2 n_xy], and 'T_c', [B,NT,3,4], come along for the tests of this restatement."""
    p = params
    M, nx, ny, cell = p["M"], p["nx"], p["ny"], np.float64(p["cell"])
    n_xy, n_theta = spec["n_xy"], spec["n_theta"]
    assert M in (B, 1) and 0 <= n_xy <= 16 and 0 <= n_theta <= 32
    min_points = p["min_points"] if spec["min_points"] is None else spec["min_points"]
    nt, ns, ex, ey = 2 * n_theta + 1, 2 * n_xy + 1, nx + 2 * n_xy, ny + 2 * n_xy
    frames = np.arange(B)
    map_of = np.zeros(B, np.int64) if M == 1 else frames
    Tm = poses_of(T, B)
    S = np.stack(transformed(Tm, frames, per_frame(sensor, B)), axis=1)
    Tc = candidate_poses(Tm, S[map_of if M == 1 else frames], rot_table(n_theta, spec["d_theta"]), n_theta)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    bb, hit = obstacle_rows(p, xyz, B, frame_offsets, rows_per_frame, valid, Tm, S)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    cur = state["cur_origin"]
    m_of = map_of[bb]
    ox, oy = cur[m_of, 0] - n_xy, cur[m_of, 1] - n_xy                     # the origin of the grown window
    counts = np.zeros((M, nt, ex, ey), np.int32)
    for t in range(nt):
        A = Tc[bb, t]
        with np.errstate(all="ignore"):
            Xt = A[:, 0, 0] * x + A[:, 0, 1] * y + A[:, 0, 2] * z + A[:, 0, 3]          # summed left to right
            Yt = A[:, 1, 0] * x + A[:, 1, 1] * y + A[:, 1, 2] * z + A[:, 1, 3]
            wx, wy = np.floor(Xt / cell), np.floor(Yt / cell)
            inside = hit & (wx >= ox.astype(np.float64)) & (wx < (ox + ex).astype(np.float64)) & (wy >= oy.astype(np.float64)) & \
                (wy < (oy + ey).astype(np.float64))
        at = (m_of[inside] * ex + (wx[inside].astype(np.int64) - ox[inside])) * ey + (wy[inside].astype(np.int64) - oy[inside])
        counts[:, t] = np.bincount(at, minlength=M * ex * ey).reshape(M, ex, ey)
    scores = np.zeros((M, nt, ns, ns), np.int64)
    k = np.arange(ns)
    for m in range(M):
        Lp = np.pad(window_log_odds(p, state, m), 2 * n_xy)                # window cell w sits at w + 2 n_xy
        for t in range(nt):
            ei, ej = np.nonzero(counts[m, t] >= min_points)                # count cell e is window cell e - n_xy; shifted by k - n_xy
            scores[m, t] = Lp[ei[:, None, None] + k[None, :, None], ej[:, None, None] + k[None, None, :]].sum(axis=0)
    out = {"pose": Tm.copy(), "pick": np.zeros((M, 3), np.int32), "score": np.zeros(M, np.int64), "prior_score": np.zeros(M, np.int64),
           "n_cells": np.zeros(M, np.int32), "status": np.zeros(M, np.int32), "scores": scores, "counts": counts, "T_c": Tc}
    finite = np.isfinite(Tm).all(axis=(1, 2)) & np.isfinite(S).all(axis=1)
    for m in range(M):
        fed = frames if M == 1 else [m]
        best = pick_of(scores[m], n_xy, n_theta)
        n_cells = int((counts[m, n_theta, n_xy:n_xy + nx, n_xy:n_xy + ny] >= min_points).sum())
        status = (UNINITIALISED if state["initialised"][m] == 0 else 0) | (0 if finite[fed].all() else NOT_FINITE) | \
            (FEW_CELLS if n_cells < spec["min_cells"] else 0) | (LOW_SCORE if best[0] < spec["min_score"] else 0)
        _, t, dx, dy = best
        if not status & KEEPS_PRIOR:
            if (n_xy > 0 and n_xy in (abs(dx), abs(dy))) or (n_theta > 0 and abs(t - n_theta) == n_theta):
                status |= ON_BORDER
            for b in fed:
                out["pose"][b] = Tc[b, t]
                out["pose"][b, 0, 3] = Tc[b, t, 0, 3] + np.float64(dx) * cell
                out["pose"][b, 1, 3] = Tc[b, t, 1, 3] + np.float64(dy) * cell
        out["pick"][m] = (t - n_theta, dx, dy)
        out["score"][m], out["prior_score"][m] = best[0], scores[m, n_theta, n_xy, n_xy]
        out["n_cells"][m], out["status"][m] = n_cells, status
    return out
