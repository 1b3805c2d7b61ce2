"""The terrain map restated in NumPy fp64 and int64 from include/camradepth_hip.h (crd_terrain_update), launch by launch as the header
describes them.  NumPy rounds every operation on its own, as the kernels do, so the two agree bit for bit.  Shared by the CPU test of
this restatement against per-point and per-cell loops, by the host test of csrc/terrain_cell.h and by the GPU tests of the kernels.

`params` are the numbers of a TerrainMap (PARAMS holds the keys); `state` is the caller's state as new_state() makes it, changed in
place by update()."""
import math

import numpy as np

from tests.bev_ref import frames_of
from tests.occupancy_ref import ORIGIN_LIMIT, per_frame, transformed

PARAMS = ("M", "nx", "ny", "cell", "z_quantum", "z_range", "max_range", "headroom", "min_points", "w_max", "step_max", "slope_max")
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
OUT = ("ground", "top", "step", "slope2", "weight", "state", "hazard", "evidence", "value", "origin")


def workspace_bytes(B, M, nx, ny):
    """The header's formula."""
    return 3 * ((4 * M * nx * ny + 15) & ~15) + ((24 * B + 15) & ~15) + ((4 * M + 15) & ~15)


def thresholds(p):
    """-> head_q, step_max_q, slope2_max: the header's integers."""
    def capped(v, cap):
        return cap if not v < cap else int(math.floor(v))
    zq = float(p["z_quantum"])
    run = 2.0 * float(p["cell"]) * float(p["slope_max"]) / zq
    return capped(float(p["headroom"]) / zq, 2 ** 30), max(capped(float(p["step_max"]) / zq, 2 ** 30), 1), max(capped(run * run, 2 ** 62), 1)


def new_state(params):
    M, nx, ny = params["M"], params["nx"], params["ny"]
    return {"ground": np.zeros((M, nx, ny), np.int32), "top": np.zeros((M, nx, ny), np.int32), "weight": np.zeros((M, nx, ny), np.int16),
            "prev_origin": np.zeros((M, 2), np.int64), "cur_origin": np.zeros((M, 2), np.int64), "initialised": np.zeros(M, np.int32),
            "status": np.zeros(M, np.int32)}


def shifted(a, di, dj, fill):
    """b[i, j] = a[i + di, j + dj], `fill` outside."""
    nx, ny = a.shape
    b = np.full_like(a, fill)
    i0, i1, j0, j1 = max(0, -di), min(nx, nx - di), max(0, -dj), min(ny, ny - dj)
    if i0 < i1 and j0 < j1:
        b[i0:i1, j0:j1] = a[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return b


def gradient(before, has_before, here, after, has_after):
    return np.where(has_before & has_after, after - before, np.where(has_after, 2 * (after - here), np.where(has_before, 2 * (here - before), 0)))


def derive(ground, top, weight, step_max_q, slope2_max, z_quantum):
    """Launch 5 for one map in window order: ground, top int64 and weight [nx,ny] -> the header's outputs but evidence and origin."""
    g, known = ground.astype(np.int64), weight != 0
    step = top.astype(np.int64) - g
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di or dj:
                nb, has = shifted(g, di, dj, 0), shifted(known, di, dj, False)
                step = np.maximum(step, np.where(has, np.abs(nb - g), 0))
    gx = gradient(shifted(g, -1, 0, 0), shifted(known, -1, 0, False), g, shifted(g, 1, 0, 0), shifted(known, 1, 0, False))
    gy = gradient(shifted(g, 0, -1, 0), shifted(known, 0, -1, False), g, shifted(g, 0, 1, 0), shifted(known, 0, 1, False))
    slope2 = gx * gx + gy * gy
    occupied = (step > step_max_q) | (slope2 > slope2_max)
    hazard = np.maximum(step * 253 // step_max_q, slope2 * 253 // slope2_max)
    return {"ground": np.where(known, g, I32_MIN).astype(np.int32), "top": np.where(known, top, I32_MIN).astype(np.int32),
            "step": np.where(known, step, 0).astype(np.int32), "slope2": np.where(known, slope2, 0).astype(np.int64),
            "weight": weight.astype(np.int16), "state": np.where(known, np.where(occupied, 2, 1), 0).astype(np.uint8),
            "hazard": np.where(known, np.where(occupied, 254, hazard), 255).astype(np.uint8),
            "value": np.where(known, (g.astype(np.float64) * np.float64(z_quantum)).astype(np.float32), np.float32(np.nan)).astype(np.float32)}


def update(params, state, xyz, B, frame_offsets=None, rows_per_frame=0, valid=None, T=None, sensor=None, centre=None):
    """-> the header's ten outputs; `state` is updated in place.  'lo', 'hi' and 'n' (the workspace after launch 3) come along for the
    tests of this restatement and of terrain_cell.h, and 'before' (w, ground, top as launch 4 counts them, in window order)."""
    p = params
    M, nx, ny, cell, zq = p["M"], p["nx"], p["ny"], np.float64(p["cell"]), np.float64(p["z_quantum"])
    assert M in (B, 1)
    z_min, z_max = (np.float64(v) for v in p["z_range"])
    head_q, step_max_q, slope2_max = thresholds(p)
    max_r2 = np.float64(p["max_range"]) * np.float64(p["max_range"])
    frames = np.arange(B)
    map_of = np.zeros(B, np.int64) if M == 1 else frames
    # launch 1: the sensors, the windows (crd_occupancy_update's)
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
    # launches 2 and 3: the rows
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n_rows = xyz.shape[0]
    b = frames_of(n_rows, B, frame_offsets, rows_per_frame)
    keep = b >= 0                                                                            # step 1
    if valid is not None:
        keep &= np.asarray(valid).reshape(-1) != 0
    bb = np.maximum(b, 0)
    X, Y, Z = transformed(T, bb, xyz.astype(np.float64))
    keep &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & np.isfinite(S[bb]).all(axis=1)
    with np.errstate(all="ignore"):
        dx, dy = X - S[bb, 0], Y - S[bb, 1]                                                  # step 2
        r2 = dx * dx + dy * dy
        keep &= ~(r2 > max_r2)
        keep &= ~(Z < z_min) & ~(Z > z_max)                                                  # step 3
        q = np.where(keep, np.floor(Z / zq), 0.0).astype(np.int64)                           # step 4
        wx, wy = np.floor(X / cell), np.floor(Y / cell)                                      # step 5
        m_of = map_of[bb]
        ox, oy = cur[m_of, 0], cur[m_of, 1]
        keep &= (wx >= ox.astype(np.float64)) & (wx < (ox + nx).astype(np.float64)) & (wy >= oy.astype(np.float64)) & \
            (wy < (oy + ny).astype(np.float64))
    at = (m_of[keep] * nx + (wx[keep].astype(np.int64) - ox[keep])) * ny + (wy[keep].astype(np.int64) - oy[keep])
    q = q[keep]
    lo, hi = np.full(M * nx * ny, I32_MAX, np.int64), np.full(M * nx * ny, I32_MIN, np.int64)
    np.minimum.at(lo, at, q)
    n = np.bincount(at, minlength=M * nx * ny).astype(np.int32)
    under = q <= lo[at] + head_q
    np.maximum.at(hi, at[under], q[under])
    lo, hi, n = (a.reshape(M, nx, ny) for a in (lo, hi, n))
    # launches 4 and 5: the cells
    out = {k: [] for k in OUT if k not in ("evidence", "origin")}
    before = np.zeros((3, M, nx, ny), np.int64)
    evidence = np.zeros((M, nx, ny), np.uint8)
    for m in range(M):
        wx, wy = cur[m, 0] + np.arange(nx, dtype=np.int64), cur[m, 1] + np.arange(ny, dtype=np.int64)
        slot = (wx % nx)[:, None], (wy % ny)[None, :]                                       # the mathematical modulo
        w, g, t = (state[k][m][slot].astype(np.int64) for k in ("weight", "ground", "top"))
        if not moved[m]:
            if not live[m]:
                w = np.zeros_like(w)
        else:
            was_there = ((wx >= prev[m, 0]) & (wx < prev[m, 0] + nx))[:, None] & ((wy >= prev[m, 1]) & (wy < prev[m, 1] + ny))[None, :]
            w = np.where(was_there, w, 0) if live[m] else np.zeros_like(w)
            g, t = np.where(w > 0, g, 0), np.where(w > 0, t, 0)
            before[:, m] = w, g, t
            observed = n[m] >= p["min_points"]
            first = observed & (w == 0)
            g = np.where(first, lo[m], np.where(observed, (w * g + lo[m]) // (w + 1), g))
            t = np.where(first, hi[m], np.where(observed, (w * t + hi[m]) // (w + 1), t))
            w = np.where(observed, np.minimum(w + 1, p["w_max"]), w)
            state["ground"][m][slot], state["top"][m][slot], state["weight"][m][slot] = g.astype(np.int32), t.astype(np.int32), w.astype(np.int16)
            state["initialised"][m] = 1
            evidence[m] = observed
        for k, v in derive(g, t, w, step_max_q, slope2_max, zq).items():
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(evidence=evidence, origin=cur.copy(), lo=lo.astype(np.int32), hi=hi.astype(np.int32), n=n, before=before, moved=moved)
    return out
