"""The local planner restated in NumPy from include/camradepth_hip.h (crd_plan_rollouts): the host tables, the map-frame poses, the static
and the track test, the per-candidate values, the score and the pick.  fp64 add, subtract, multiply, divide, floor and compare, which
NumPy rounds one by one as the kernels do, and integers in int64, so the two agree bit for bit.  Shared by the CPU tests of this
restatement against a plain loop (tests/test_rollout_ref_cpu.py), by the host test of the pick and by the GPU tests."""
import math

import numpy as np

UNREACHED = 0x7FFFFFFF
NOT_FINITE, NO_CANDIDATE = 1, 2
ADMISSIBLE, CLEAR_STATIC, CLEAR, VALID = 1, 2, 4, 8
STATUS_COL, N_CELLS_COL = 0, 5                       # the columns of crd_track_objects' `tracks` that are read
OUT = ("best", "command", "score", "info")
TABLES = ("scores", "first_blocked", "first_track", "max_cost", "end_togo")
WEIGHTS = dict(togo=1, max_cost=0, sum_cost=1, slow=0, turn=0)
SPEC = dict(v=(0.0, 2.0, 8), w=(1.0, 17), dt=0.1, n_poses=32, track_dt=None, keep_out=0.0, min_speed=0.0, max_object_cells=64, min_status=2,
            accel=None, blocked_at=253, outside_blocks=True, weights=WEIGHTS, cell=None)


def spec(**changes):
    s = dict(SPEC, **changes)
    s["weights"] = dict(WEIGHTS, **(s["weights"] or {}))
    return s


def workspace_bytes(M, K):
    return 32 * M * K


def host_tables(s):
    """-> vw [K,2], arc [K,P,2], tau [P] of a spec, with Python floats and math.sin / math.cos as the header's host side says."""
    (v_min, v_max, n_v), (w_max, n_w), dt, P = s["v"], s["w"], float(s["dt"]), s["n_poses"]
    v_min, v_max, w_max = float(v_min), float(v_max), float(w_max)
    track_dt = dt if s["track_dt"] is None else float(s["track_dt"])
    c = (n_w - 1) // 2
    vw = np.zeros((n_v * n_w, 2))
    arc = np.zeros((n_v * n_w, P, 2))
    for iv in range(n_v):
        for iw in range(n_w):
            k = iv * n_w + iw
            v = v_min if n_v == 1 else v_min + iv * (v_max - v_min) / (n_v - 1)
            w = 0.0 if iw == c else (iw - c) * w_max / c
            vw[k] = v, w
            for p in range(P):
                t = (p + 1) * dt
                arc[k, p] = (v * t, 0.0) if w == 0.0 else (v / w * math.sin(w * t), v / w * (1.0 - math.cos(w * t)))
    tau = np.array([(p + 1) * dt / track_dt for p in range(P)])
    return vw, arc, tau


def numbers(s):
    """The scalars the host passes: keep_out2, min_speed2, a_v_dt, a_w_dt."""
    a = s["accel"]
    dt = float(s["dt"])
    return dict(keep_out2=float(s["keep_out"]) * float(s["keep_out"]), min_speed2=float(s["min_speed"]) * float(s["min_speed"]),
                a_v_dt=0.0 if a is None else float(a[0]) * dt, a_w_dt=0.0 if a is None else float(a[1]) * dt)


def turn_of(k, n_w):
    return np.abs(np.asarray(k) % n_w - (n_w - 1) // 2)


def better(a, b, n_w):
    """rollout_pick.h's rp_better over (valid, score, k)."""
    if a[0] != b[0]:
        return a[0] > b[0]
    if a[0]:
        if a[1] != b[1]:
            return a[1] < b[1]
        ta, tb = int(turn_of(a[2], n_w)), int(turn_of(b[2], n_w))
        if ta != tb:
            return ta < tb
        if a[2] // n_w != b[2] // n_w:
            return a[2] // n_w > b[2] // n_w
    return a[2] < b[2]


def pick_of(valid, scores, n_w):
    """The least candidate in the header's order as one lexicographic sort -> k (valid or not)."""
    k = np.arange(valid.size)
    v = np.asarray(valid, bool)
    keys = (k, np.where(v, -(k // n_w), 0), np.where(v, turn_of(k, n_w), 0), np.where(v, scores, 0), ~v)       # the last key is the first
    return int(np.lexsort(keys)[0])


def counting(tracks, pos, vel, min_status, max_object_cells, min_speed2):
    """The slots [T] of one map that count."""
    with np.errstate(all="ignore"):
        speed2 = vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]
        return (tracks[:, STATUS_COL] >= min_status) & np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1) & \
            (tracks[:, N_CELLS_COL] <= max_object_cells) & (speed2 >= np.float64(min_speed2))


def plan_rollouts(s, pose, origin, cell, cost, togo=None, tracks=None, pos=None, vel=None, twist=None, chunk=64):
    """crd_plan_rollouts -> 'best', 'command', 'score', 'info', the five tables [M,K], 'flags' and 'sum_cost' [M,K] (the records') and 'xy'."""
    vw, arc, tau = host_tables(s)
    num, w = numbers(s), dict(WEIGHTS, **(s["weights"] or {}))
    (_, _, n_v), (_, n_w), P = s["v"], s["w"], s["n_poses"]
    K = n_v * n_w
    pose, origin, cost = np.asarray(pose, np.float64), np.asarray(origin, np.int64), np.asarray(cost, np.uint8)
    M, nx, ny = cost.shape
    cell = np.float64(cell)
    out = {"best": np.zeros(M, np.int32), "command": np.zeros((M, 2)), "score": np.zeros(M, np.int64), "info": np.zeros((M, 8), np.int32),
           "scores": np.zeros((M, K), np.int64), "first_blocked": np.zeros((M, K), np.int32), "first_track": np.zeros((M, K), np.int32),
           "max_cost": np.zeros((M, K), np.int32), "end_togo": np.zeros((M, K), np.int32), "flags": np.zeros((M, K), np.int32),
           "sum_cost": np.zeros((M, K), np.int32),
           "xy": np.zeros((M, K, P, 2))}
    k = np.arange(K)
    iv = k // n_w
    x, y = arc[..., 0], arc[..., 1]
    for m in range(M):
        T = pose[m]
        with np.errstate(all="ignore"):
            X = T[0, 0] * x + T[0, 1] * y + T[0, 3]
            Y = T[1, 0] * x + T[1, 1] * y + T[1, 3]
            wx, wy = np.floor(X / cell), np.floor(Y / cell)
            ox, oy = int(origin[m, 0]), int(origin[m, 1])
            inside = np.isfinite(X) & np.isfinite(Y) & (wx >= np.float64(ox)) & (wx < np.float64(ox + nx)) & (wy >= np.float64(oy)) & \
                (wy < np.float64(oy + ny))
        i = np.where(inside, wx, 0).astype(np.int64) - np.where(inside, ox, 0)
        j = np.where(inside, wy, 0).astype(np.int64) - np.where(inside, oy, 0)
        c = i * ny + j
        cost_at = np.where(inside, cost[m].reshape(-1)[c].astype(np.int64), 0)
        blocked = (inside & (cost_at >= s["blocked_at"])) | (~inside & bool(s["outside_blocks"]))
        first_static = np.where(blocked.any(axis=1), blocked.argmax(axis=1), P)
        end = np.full(K, UNREACHED, np.int64)
        if togo is not None:
            end = np.where(inside[:, P - 1], np.asarray(togo[m]).reshape(-1)[c[:, P - 1]].astype(np.int64), UNREACHED)
        hit_pose, hit_slot = np.full(K, P, np.int64), np.full(K, -1, np.int64)
        if tracks is not None:
            slots = np.flatnonzero(counting(tracks[m], pos[m], vel[m], s["min_status"], s["max_object_cells"], num["min_speed2"]))
            if slots.size:
                px, py, vx, vy = pos[m][slots, 0], pos[m][slots, 1], vel[m][slots, 0], vel[m][slots, 1]
                with np.errstate(all="ignore"):
                    qx, qy = px[None, :] + vx[None, :] * tau[:, None], py[None, :] + vy[None, :] * tau[:, None]      # [P, slots]
                    for k0 in range(0, K, chunk):
                        dx, dy = X[k0:k0 + chunk, :, None] - qx[None], Y[k0:k0 + chunk, :, None] - qy[None]
                        hit = dx * dx + dy * dy <= np.float64(num["keep_out2"])                                        # [k, P, slots]
                        any_p = hit.any(axis=2)
                        first_p = np.where(any_p.any(axis=1), any_p.argmax(axis=1), P)
                        at = np.minimum(first_p, P - 1)
                        row = hit[np.arange(hit.shape[0]), at]
                        hit_pose[k0:k0 + chunk] = first_p
                        hit_slot[k0:k0 + chunk] = np.where(first_p < P, slots[row.argmax(axis=1)], -1)
        first = np.minimum(first_static, hit_pose)
        admissible = np.ones(K, bool)
        if twist is not None:
            with np.errstate(all="ignore"):
                admissible = (np.abs(vw[:, 0] - twist[m, 0]) <= np.float64(num["a_v_dt"])) & \
                    (np.abs(vw[:, 1] - twist[m, 1]) <= np.float64(num["a_w_dt"]))
        clear = first == P
        valid = admissible & clear & ~((togo is not None) & (w["togo"] > 0) & (end == UNREACHED))
        max_cost, sum_cost = cost_at.max(axis=1), cost_at.sum(axis=1)
        scores = (w["togo"] * end if togo is not None else 0) + w["max_cost"] * max_cost + w["sum_cost"] * sum_cost + \
            w["slow"] * (n_v - 1 - iv) + w["turn"] * turn_of(k, n_w)
        bad = not np.isfinite(T).all() or (twist is not None and not np.isfinite(twist[m]).all())
        status = (NOT_FINITE if bad else 0) | (0 if valid.any() else NO_CANDIDATE)
        best = pick_of(valid, scores, n_w) if status == 0 else -1
        out["best"][m], out["score"][m] = best, scores[best] if best >= 0 else 0
        out["command"][m] = vw[best] if best >= 0 else (0.0, 0.0)
        out["info"][m, :5] = admissible.sum(), (first_static == P).sum(), clear.sum(), valid.sum(), status
        out["scores"][m], out["first_blocked"][m], out["first_track"][m] = scores, np.where(clear, -1, first), hit_slot
        out["max_cost"][m], out["end_togo"][m], out["sum_cost"][m] = max_cost, end, sum_cost
        out["flags"][m] = admissible * ADMISSIBLE + (first_static == P) * CLEAR_STATIC + clear * CLEAR + valid * VALID
        out["xy"][m, ..., 0], out["xy"][m, ..., 1] = X, Y
    return out


def plan_rollouts_loop(s, pose, origin, cell, cost, togo=None, tracks=None, pos=None, vel=None, twist=None):
    """The header read as a plain Python loop over maps, candidates, poses and slots, one scalar operation at a time -> the same
    dictionary without 'xy'.  Slow: for small problems."""
    vw, arc, tau = host_tables(s)
    num, w = numbers(s), dict(WEIGHTS, **(s["weights"] or {}))
    (_, _, n_v), (_, n_w), P = s["v"], s["w"], s["n_poses"]
    K, c_w = n_v * n_w, (n_w - 1) // 2
    M, nx, ny = np.asarray(cost).shape
    f = np.float64
    res = {k: [] for k in OUT + TABLES + ("flags",)}
    with np.errstate(all="ignore"):
        for m in range(M):
            T = [[f(v) for v in r] for r in np.asarray(pose[m])]
            ox, oy = int(origin[m][0]), int(origin[m][1])
            rows = []
            for k in range(K):
                iv, iw = divmod(k, n_w)
                first_static = first = first_hit = -1
                first_slot, max_cost, sum_cost, end = -1, 0, 0, UNREACHED
                for p in range(P):
                    x, y = f(arc[k, p, 0]), f(arc[k, p, 1])
                    X = T[0][0] * x + T[0][1] * y + T[0][3]
                    Y = T[1][0] * x + T[1][1] * y + T[1][3]
                    wx, wy = np.floor(X / f(cell)), np.floor(Y / f(cell))
                    inside = bool(np.isfinite(X) and np.isfinite(Y) and f(ox) <= wx < f(ox + nx) and f(oy) <= wy < f(oy + ny))
                    if inside:
                        i, j = int(wx) - ox, int(wy) - oy
                        cst = int(cost[m][i][j])
                        max_cost, sum_cost = max(max_cost, cst), sum_cost + cst
                        blocked = cst >= s["blocked_at"]
                        if p == P - 1 and togo is not None:
                            end = int(togo[m][i][j])
                    else:
                        blocked = bool(s["outside_blocks"])
                    if blocked and first_static < 0:
                        first_static = p
                    hit = -1
                    if tracks is not None and first_hit < 0:
                        for slot in range(len(tracks[m])):
                            px, py, vx, vy = f(pos[m][slot][0]), f(pos[m][slot][1]), f(vel[m][slot][0]), f(vel[m][slot][1])
                            if not (tracks[m][slot][STATUS_COL] >= s["min_status"] and np.isfinite([px, py, vx, vy]).all() and
                                    tracks[m][slot][N_CELLS_COL] <= s["max_object_cells"] and vx * vx + vy * vy >= f(num["min_speed2"])):
                                continue
                            qx, qy = px + vx * f(tau[p]), py + vy * f(tau[p])
                            dx, dy = X - qx, Y - qy
                            if dx * dx + dy * dy <= f(num["keep_out2"]):
                                hit = slot
                                break
                    if hit >= 0:
                        first_hit, first_slot = p, hit
                    if (blocked or hit >= 0) and first < 0:
                        first = p
                admissible = True
                if twist is not None:
                    admissible = bool(abs(f(vw[k, 0]) - f(twist[m][0])) <= f(num["a_v_dt"]) and abs(f(vw[k, 1]) - f(twist[m][1])) <= f(num["a_w_dt"]))
                valid = admissible and first < 0 and not (togo is not None and w["togo"] > 0 and end == UNREACHED)
                score = (w["togo"] * end if togo is not None else 0) + w["max_cost"] * max_cost + w["sum_cost"] * sum_cost + \
                    w["slow"] * (n_v - 1 - iv) + w["turn"] * abs(iw - c_w)
                rows.append(dict(score=score, first_blocked=first, first_track=first_slot, max_cost=max_cost, end_togo=end,
                                 flags=admissible * ADMISSIBLE + (first_static < 0) * CLEAR_STATIC + (first < 0) * CLEAR + valid * VALID))
            bad = not np.isfinite(np.asarray(pose[m])).all() or (twist is not None and not np.isfinite(np.asarray(twist[m])).all())
            n_valid = sum(1 for r in rows if r["flags"] & VALID)
            status = (NOT_FINITE if bad else 0) | (0 if n_valid else NO_CANDIDATE)
            best = -1
            if status == 0:
                best = 0
                for k in range(1, K):
                    if better((bool(rows[k]["flags"] & VALID), rows[k]["score"], k), (bool(rows[best]["flags"] & VALID), rows[best]["score"], best), n_w):
                        best = k
            res["best"].append(best)
            res["score"].append(rows[best]["score"] if best >= 0 else 0)
            res["command"].append(vw[best] if best >= 0 else np.zeros(2))
            res["info"].append([sum(1 for r in rows if r["flags"] & b) for b in (ADMISSIBLE, CLEAR_STATIC, CLEAR, VALID)] + [status, 0, 0, 0])
            res["scores"].append([r["score"] for r in rows])
            for name in TABLES[1:] + ("flags",):
                res[name].append([r[name] for r in rows])
    types = dict(best=np.int32, command=np.float64, score=np.int64, info=np.int32, scores=np.int64)
    return {k: np.asarray(v, types.get(k, np.int32)) for k, v in res.items()}
