"""The navigation field restated in NumPy from include/camradepth_hip.h (crd_nav_field, crd_nav_paths): the row sweeps in the header's
order, the direction map as a function of the final togo, and the path following.  Integer arithmetic in int64, plus the fp64 divide,
floor and compare that find a cell and the multiply of a cell centre, which NumPy rounds as the kernels do, so the two agree bit for
bit.  Shared by the CPU test of this restatement against heap Dijkstra and scipy's (tests/test_nav_ref_cpu.py) and by the GPU tests."""
import numpy as np

UNREACHED = 0x7FFFFFFF
ON_GOAL, NO_STEP = 8, 255
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
WEIGHTS = tuple(7 if di and dj else 5 for di, dj in NEIGHBOURS)
_BIG, _WALL = 1 << 40, 1 << 60


def window_cells(xy, origin, cell, nx, ny):
    """crd_field_paths' INSIDE rule for points xy [..., 2] of one map with origin (ox, oy): i * ny + j, or -1."""
    xy = np.asarray(xy, np.float64)
    ox, oy = int(origin[0]), int(origin[1])
    X, Y = xy[..., 0], xy[..., 1]
    with np.errstate(all="ignore"):
        wx, wy = np.floor(X / np.float64(cell)), np.floor(Y / np.float64(cell))
        inside = np.isfinite(X) & np.isfinite(Y) & (wx >= np.float64(ox)) & (wx < np.float64(ox + nx)) & (wy >= np.float64(oy)) & \
            (wy < np.float64(oy + ny))
    i = np.where(inside, wx, 0).astype(np.int64) - np.where(inside, ox, 0)
    j = np.where(inside, wy, 0).astype(np.int64) - np.where(inside, oy, 0)
    return np.where(inside, i * ny + j, -1)


def _along(t, step, passable):
    """d[j] = min(t[j], d[j - 1] + step[j]) on the passable cells, a wall or the row's start giving nothing: a prefix minimum of t - S
    over the prefix sum S of the steps, in which a wall is a step no value gets over."""
    S = np.cumsum(np.where(passable, step, _BIG))
    d = S + np.minimum.accumulate(np.where(passable, t, _WALL) - S)
    return np.where(passable & (d < UNREACHED), d, UNREACHED)


def row_step(togo, w, passable, i, p):
    """Row i of one map from row p (None: no row), then left to right, then right to left.  -> whether a value fell."""
    t = togo[i].copy()
    if p is not None:
        above = np.concatenate([[UNREACHED], togo[p], [UNREACHED]])
        for dj, k in ((-1, 7), (0, 5), (1, 7)):
            v = above[1 + dj:1 + dj + t.size]
            t = np.where(passable[i] & (v != UNREACHED), np.minimum(t, v + k * w[i]), t)
    d = _along(t, 5 * w[i], passable[i])
    d = _along(d[::-1], 5 * w[i][::-1], passable[i][::-1])[::-1]
    changed = bool((d < togo[i]).any())
    togo[i] = d
    return changed


def nav_field(cost, goals, n_goals, origin, cell, neutral=50, blocked_at=253, max_rounds=64, with_next=True):
    """crd_nav_field -> 'togo' int32 [M,nx,ny], 'next' uint8 [M,nx,ny], 'info' int32 [M,4]."""
    cost = np.asarray(cost, np.uint8)
    M, nx, ny = cost.shape
    goals = np.asarray(goals, np.float64)
    G = goals.shape[1]
    n = np.full(M, G, np.int64) if n_goals is None else np.clip(np.asarray(n_goals, np.int64), 0, G)
    out = np.full((M, nx, ny), UNREACHED, np.int64)
    info = np.zeros((M, 4), np.int32)
    for m in range(M):
        passable = cost[m] < blocked_at
        w = neutral + cost[m].astype(np.int64)
        togo = out[m]
        c = window_cells(goals[m, :n[m]], origin[m], cell, nx, ny)
        used = (c >= 0) & passable.reshape(-1)[np.maximum(c, 0)]
        togo.reshape(-1)[c[used]] = 0
        rounds = 0
        while True:
            changed = False
            for i in range(nx):
                changed |= row_step(togo, w, passable, i, i - 1 if i else None)
            for i in range(nx - 2, -1, -1):
                changed |= row_step(togo, w, passable, i, i + 1)
            rounds += 1
            if not changed or rounds >= max_rounds:
                break
        info[m] = (0 if changed else 1, rounds, int(used.sum()), int(n[m] - used.sum()))
    res = {"togo": out.astype(np.int32), "info": info}
    if with_next:
        res["next"] = next_map(res["togo"], cost, neutral)
    return res


def next_map(togo, cost, neutral=50):
    """The direction map of a cost-to-go: 8 where togo is 0, 255 where UNREACHED, else the lowest code n that minimises togo[a + n] +
    k_n * w(a) over the neighbours inside the window with togo != UNREACHED."""
    togo = np.asarray(togo, np.int64)
    M, nx, ny = togo.shape
    w = neutral + np.asarray(cost, np.uint8).astype(np.int64)
    pad = np.full((M, nx + 2, ny + 2), UNREACHED, np.int64)
    pad[:, 1:-1, 1:-1] = togo
    best = np.full(togo.shape, 1 << 62, np.int64)
    code = np.full(togo.shape, NO_STEP, np.int64)
    for n, ((di, dj), k) in enumerate(zip(NEIGHBOURS, WEIGHTS)):                               # ascending: strictly less keeps the lowest
        there = pad[:, 1 + di:1 + di + nx, 1 + dj:1 + dj + ny]
        v = np.where(there != UNREACHED, there + k * w, 1 << 62)
        take = v < best
        best, code = np.where(take, v, best), np.where(take, n, code)
    return np.where(togo == 0, ON_GOAL, np.where(togo == UNREACHED, NO_STEP, code)).astype(np.uint8)


def plan_paths(starts, path_map, origin, cell, togo, nxt, P):
    """crd_nav_paths -> 'cells' [K,P], 'xy' [K,P,2], 'n_cells', 'start_togo', 'status' [K]."""
    starts = np.asarray(starts, np.float64)
    K = starts.shape[0]
    M, nx, ny = togo.shape
    origin = np.asarray(origin, np.int64)
    m_of = np.zeros(K, np.int64) if path_map is None else np.asarray(path_map, np.int64)
    cells = np.full((K, P), -1, np.int32)
    xy = np.full((K, P, 2), np.nan, np.float64)
    n_cells, start_togo, status = np.zeros(K, np.int32), np.full(K, UNREACHED, np.int32), np.full(K, 2, np.int32)
    for k in range(K):
        m = int(m_of[k])
        if not 0 <= m < M:
            continue
        c = int(window_cells(starts[k], origin[m], cell, nx, ny))
        if c < 0:
            continue
        start_togo[k] = togo[m].reshape(-1)[c]
        if start_togo[k] == UNREACHED:
            status[k] = 3
            continue
        status[k] = 1
        n = 0
        while n < P:
            i, j = divmod(c, ny)
            cells[k, n] = c
            xy[k, n] = ((np.float64(origin[m, 0] + i) + np.float64(0.5)) * np.float64(cell),
                        (np.float64(origin[m, 1] + j) + np.float64(0.5)) * np.float64(cell))
            n += 1
            code = int(nxt[m, i, j])
            if code == ON_GOAL:
                status[k] = 0
                break
            if code > 7:
                break
            i2, j2 = i + NEIGHBOURS[code][0], j + NEIGHBOURS[code][1]
            if not (0 <= i2 < nx and 0 <= j2 < ny):
                break
            c = i2 * ny + j2
        n_cells[k] = n
    return {"cells": cells, "xy": xy, "n_cells": n_cells, "start_togo": start_togo, "status": status}
