"""crd_track_objects restated in plain Python / NumPy fp64, operation by operation as include/camradepth_hip.h lists them: predict,
candidates, the assignment by rounds of mutual best choices, matched and unmatched tracks, tracks that left the window, births, counts.
Python floats are IEEE doubles and never fuse a multiply with an add, so the kernel is compared with this bit for bit."""
import math

import numpy as np

FREE, TENTATIVE, CONFIRMED = 0, 1, 2
FREE_ROW = (0, 0, 0, 0, -1, 0, 0, 0)
NOT, OPEN = -2, -1
INT_MAX = 2 ** 31 - 1
STATE = ("ids", "tracks", "pos", "vel", "box", "next_id")
OUT = ("track_of", "id_of", "info")


def new_state(M, T):
    """Every slot free, the ids from 0: ObjectTracks after construction and after reset()."""
    tracks = np.zeros((M, T, 8), np.int32)
    tracks[..., 4] = -1
    return {"ids": np.full((M, T), -1, np.int64), "tracks": tracks, "pos": np.full((M, T, 2), np.nan), "vel": np.full((M, T, 2), np.nan),
            "box": np.zeros((M, T, 4), np.int64), "next_id": np.zeros(M, np.int64)}


def d2_of(z, p):
    dx, dy = float(z[0]) - float(p[0]), float(z[1]) - float(p[1])
    return (dx * dx) + (dy * dy)


def associate(pred, live, z, candidate, gate2, cap):
    """Rounds of mutual best choices -> (trk_obj [T], obj_trk [N], rounds, guard): the row of every slot and the slot of every row, OPEN
    when untaken, NOT for a free slot and for a row that is no candidate."""
    T, N = len(live), len(candidate)
    trk_obj = [OPEN if live[t] else NOT for t in range(T)]
    obj_trk = [OPEN if candidate[k] else NOT for k in range(N)]
    rounds, took = 0, True
    while rounds < cap:
        obj_pick, trk_pick = {}, {}
        for k in range(N):
            if obj_trk[k] == OPEN:
                best = min(((d2_of(z[k], pred[t]), t) for t in range(T) if trk_obj[t] == OPEN and d2_of(z[k], pred[t]) <= gate2), default=None)
                obj_pick[k] = None if best is None else best[1]
        for t in range(T):
            if trk_obj[t] == OPEN:
                best = min(((d2_of(z[k], pred[t]), k) for k in range(N) if obj_trk[k] == OPEN and d2_of(z[k], pred[t]) <= gate2), default=None)
                trk_pick[t] = None if best is None else best[1]
        took = False
        for k, t in obj_pick.items():
            if t is not None and trk_pick[t] == k:
                obj_trk[k], trk_obj[t], took = t, k, True
        rounds += 1
        if not took:
            break
    return trk_obj, obj_trk, rounds, int(took)


def inside(X, Y, ox, oy, nx, ny, cell):
    """crd_field_paths' INSIDE rule."""
    if not (math.isfinite(X) and math.isfinite(Y)):
        return False
    wx, wy = np.floor(np.float64(X) / np.float64(cell)), np.floor(np.float64(Y) / np.float64(cell))
    return bool(float(ox) <= wx < float(ox + nx) and float(oy) <= wy < float(oy + ny))


def up(v):
    return min(int(v) + 1, INT_MAX)


def problem(state, m, centre, objects_info):
    """Steps 1 and 2 of map m -> (pred [T], live [T], z [N], candidate [N], n): what the association sees."""
    tracks, pos, vel = state["tracks"][m], state["pos"][m], state["vel"][m]
    T, N = tracks.shape[0], centre.shape[1]
    n = min(max(int(objects_info[m, 0]), 0), N)
    live = [int(tracks[t, 0]) != FREE for t in range(T)]
    pred = [(float(pos[t, 0]) + float(vel[t, 0]), float(pos[t, 1]) + float(vel[t, 1])) if live[t] else (0.0, 0.0) for t in range(T)]
    z = [(float(centre[m, k, 0]), float(centre[m, k, 1])) for k in range(N)]
    candidate = [k < n and math.isfinite(z[k][0]) and math.isfinite(z[k][1]) for k in range(N)]
    return pred, live, z, candidate, n


def track_objects(state, objects, centre, objects_info, origin, nx, ny, cell, gate, alpha, beta, confirm_hits, max_misses):
    """state: new_state()'s dictionary, updated IN PLACE.  objects int32 [M,N,8], centre fp64 [M,N,2], objects_info int32 [M,4], origin
    int64 [M,2] -> 'track_of' int32 [M,N], 'id_of' int64 [M,N], 'info' int32 [M,8]."""
    M, T = state["ids"].shape
    N = objects.shape[1]
    gate2 = float(gate) * float(gate)
    alpha, beta = float(alpha), float(beta)
    track_of, id_of, info = np.full((M, N), -1, np.int32), np.full((M, N), -1, np.int64), np.zeros((M, 8), np.int32)
    for m in range(M):
        ids, tracks, pos, vel, box = (state[k][m] for k in STATE[:5])
        ox, oy = int(origin[m, 0]), int(origin[m, 1])
        pred, live, z, candidate, _ = problem(state, m, centre, objects_info)
        trk_obj, obj_trk, rounds, guard = associate(pred, live, z, candidate, gate2, min(N, T) + 1)
        n_matched = n_missed_out = n_left = 0
        for t in range(T):
            if not live[t]:
                continue
            k = trk_obj[t]
            if k >= 0:
                n_matched += 1
                for c in range(2):
                    r = z[k][c] - pred[t][c]
                    pos[t, c] = pred[t][c] + alpha * r
                    vel[t, c] = float(vel[t, c]) + beta * r
                row = objects[m, k]
                tracks[t, 1], tracks[t, 2], tracks[t, 3], tracks[t, 4] = up(tracks[t, 1]), up(tracks[t, 2]), 0, k
                tracks[t, 5], tracks[t, 6] = row[1], row[6]
                box[t] = [ox + int(row[2]), ox + int(row[3]), oy + int(row[4]), oy + int(row[5])]
                if tracks[t, 2] >= confirm_hits:
                    tracks[t, 0] = CONFIRMED
            else:
                pos[t] = pred[t]
                tracks[t, 1], tracks[t, 3], tracks[t, 4] = up(tracks[t, 1]), up(tracks[t, 3]), -1
                if tracks[t, 3] > max_misses:
                    live[t] = False
                    n_missed_out += 1
            if live[t] and not inside(float(pos[t, 0]), float(pos[t, 1]), ox, oy, nx, ny, cell):
                live[t] = False
                n_left += 1
                if k >= 0:
                    obj_trk[k] = NOT
            if not live[t]:
                ids[t], tracks[t], pos[t], vel[t], box[t] = -1, FREE_ROW, np.nan, np.nan, 0
        free = [t for t in range(T) if not live[t]]
        new = [k for k in range(N) if obj_trk[k] == OPEN]
        births = min(len(new), len(free))
        for k in range(N):
            if obj_trk[k] >= 0:
                track_of[m, k], id_of[m, k] = obj_trk[k], ids[obj_trk[k]]
        for rank in range(births):
            k, t = new[rank], free[rank]
            row = objects[m, k]
            ids[t] = int(state["next_id"][m]) + rank
            tracks[t] = [CONFIRMED if confirm_hits <= 1 else TENTATIVE, 1, 1, 0, k, row[1], row[6], 0]
            pos[t], vel[t] = z[k], 0.0
            box[t] = [ox + int(row[2]), ox + int(row[3]), oy + int(row[4]), oy + int(row[5])]
            track_of[m, k], id_of[m, k] = t, ids[t]
        state["next_id"][m] += births
        info[m] = [int((tracks[:, 0] != FREE).sum()), n_matched, births, n_missed_out, n_left, len(new) - births, rounds, guard]
    return {"track_of": track_of, "id_of": id_of, "info": info}


def run_case(case):
    """A case of tests/tracks_cases.py through the restatement -> per frame (state after the frame, outputs), all copies."""
    spec = case["spec"]
    M, T = case["M"], spec["max_tracks"]
    state = new_state(M, T)
    frames = []
    for f in case["frames"]:
        if f.get("reset"):
            state = new_state(M, T)
        out = track_objects(state, f["objects"], f["centre"], f["info"], f["origin"], case["nx"], case["ny"], case["cell"], spec["gate"],
                            spec["alpha"], spec["beta"], spec["confirm_hits"], spec["max_misses"])
        frames.append(({k: v.copy() for k, v in state.items()}, out))
    return frames
