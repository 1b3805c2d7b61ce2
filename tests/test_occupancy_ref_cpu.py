"""CPU: tests/occupancy_ref.py, the vectorised NumPy restatement of crd_occupancy_update that the GPU tests compare the kernels with,
against an independent model in plain Python -- one loop per point and per cell in Python floats, and the map kept as a dictionary
keyed by world cell that forgets a cell when it leaves the window, in place of the torus -- over every case of tests/occupancy_cases.py;
then the bin rule's edge values and what the scenes are meant to show (a free fan, the wall occupied, unknown behind it)."""
import math

import numpy as np
import pytest

from tests import occupancy_cases, occupancy_ref

CASES = occupancy_cases.all_cases()


def bin_loop(dx, dy, n_bins):
    q_bins = n_bins // 4
    ax, ay = abs(dx), abs(dy)
    if ax >= ay:
        face, s = (0 if dx > 0 else 2), dy / ax
    else:
        face, s = (1 if dy > 0 else 3), dx / ay
    return face * q_bins + min(math.floor(((s + 1.0) * 0.5) * q_bins), q_bins - 1)


def through(T, b, v):
    x, y, z = (float(c) for c in v)
    if T is None:
        return x, y, z
    M = T[b] if np.ndim(T) == 3 else T
    return tuple(float(M[i][0]) * x + float(M[i][1]) * y + float(M[i][2]) * z + float(M[i][3]) for i in range(3))


def finite(*v):
    return all(math.isfinite(c) for c in v)


class LoopMap:
    """The header, read as loops.  world[m]: {(wx, wy): log-odds} of the cells of map m's window."""

    def __init__(self, params):
        self.p = params
        self.world = [{} for _ in range(params["M"])]
        self.origin = [(0, 0)] * params["M"]
        self.status = [0] * params["M"]

    def update(self, xyz, B, frame_offsets=None, rows_per_frame=0, valid=None, T=None, sensor=None, centre=None):
        p = self.p
        M, nx, ny, cell, n_bins = p["M"], p["nx"], p["ny"], p["cell"], p["n_bins"]
        point_of = lambda v, b: (0.0, 0.0, 0.0) if v is None else (v[b] if np.ndim(v) == 2 else v)      # noqa: E731
        S = [through(T, b, point_of(sensor, b)) for b in range(B)]
        for b in range(B):
            if not finite(*S[b]):
                self.status[0 if M == 1 else b] |= 2
        moved = []
        for m in range(M):
            b = 0 if M == 1 else m
            C = through(T, b, point_of(sensor if centre is None else centre, b))
            ok = finite(*C) and finite(C[0] / cell, C[1] / cell) and all(abs(math.floor(c / cell)) < 2 ** 31 - 65536 for c in C[:2])
            moved.append(ok)
            if ok:
                self.origin[m] = (math.floor(C[0] / cell) - nx // 2, math.floor(C[1] / cell) - ny // 2)
            else:
                self.status[m] |= 1
        hit_min = [[math.inf] * n_bins for _ in range(B)]
        seen_max = [[0.0] * n_bins for _ in range(B)]
        hits = [{} for _ in range(M)]
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        for i, row in enumerate(xyz):
            if valid is not None and not valid[i]:
                continue
            if frame_offsets is not None:
                b = next((f for f in range(B) if frame_offsets[f] <= i < frame_offsets[f + 1]), -1)
            else:
                b = i // rows_per_frame
            if b < 0 or b >= B:
                continue
            X, Y, Z = through(T, b, row)
            if not finite(X, Y, Z, *S[b]):
                continue
            dx, dy = X - S[b][0], Y - S[b][1]
            r2 = dx * dx + dy * dy
            if r2 == 0 or r2 > p["max_range"] * p["max_range"]:
                continue
            k = bin_loop(dx, dy, n_bins)
            if p["z_floor"] <= Z <= p["z_hi"]:
                seen_max[b][k] = max(seen_max[b][k], r2)
            if p["z_lo"] <= Z <= p["z_hi"]:
                hit_min[b][k] = min(hit_min[b][k], r2)
                m = 0 if M == 1 else b
                wx, wy = math.floor(X / cell), math.floor(Y / cell)
                if self.origin[m][0] <= wx < self.origin[m][0] + nx and self.origin[m][1] <= wy < self.origin[m][1] + ny:
                    hits[m][(wx, wy)] = hits[m].get((wx, wy), 0) + 1
        out = {k: np.zeros((M, nx, ny), t) for k, t in (("log_odds", np.int16), ("state", np.uint8), ("evidence", np.uint8))}
        for m in range(M):
            ox, oy = self.origin[m]
            after = {}
            for i in range(nx):
                for j in range(ny):
                    wx, wy = ox + i, oy + j
                    old = self.world[m].get((wx, wy), 0)
                    ev = 0
                    if moved[m]:
                        if hits[m].get((wx, wy), 0) >= p["min_points"]:
                            ev = 2
                        else:
                            cx, cy = (wx + 0.5) * cell, (wy + 0.5) * cell
                            for b in (range(B) if M == 1 else [m]):
                                dx, dy = cx - S[b][0], cy - S[b][1]
                                r2c = dx * dx + dy * dy
                                if r2c > 0 and math.isfinite(r2c):
                                    k = bin_loop(dx, dy, n_bins)
                                    if r2c < hit_min[b][k] and r2c <= seen_max[b][k]:
                                        ev = 1
                    new = max(-p["l_max"], min(p["l_max"], old + (p["l_occ"] if ev == 2 else -p["l_free"] if ev == 1 else 0)))
                    after[(wx, wy)] = new
                    out["log_odds"][m, i, j], out["evidence"][m, i, j] = new, ev
                    out["state"][m, i, j] = 2 if new >= p["occupied_at"] else 1 if new <= -p["free_at"] else 0
            if moved[m]:
                self.world[m] = after                       # the cells outside the window are forgotten
        out["origin"] = np.array(self.origin, np.int64)
        return out


def run_ref(case):
    state = occupancy_ref.new_state(case["params"])
    return [occupancy_ref.update(case["params"], state, B=case["B"], **f) for f in case["frames"]], state


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_loops_and_the_torus_the_dictionary(name):
    case = CASES[name]
    loops = LoopMap(case["params"])
    got, state = run_ref(case)
    for step, (frame, g) in enumerate(zip(case["frames"], got)):
        want = loops.update(B=case["B"], **frame)
        for k in ("origin", "evidence", "log_odds", "state"):
            assert g[k].dtype == want[k].dtype and np.array_equal(g[k], want[k]), (name, step, k, np.argwhere(g[k] != want[k])[:4].tolist())
        assert g["value"].dtype == np.float32 and np.array_equal(g["value"], want["log_odds"].astype(np.float32))
    assert state["status"].tolist() == loops.status


def test_the_bin_rule_at_its_edges():
    for n_bins in (4, 8, 720, 65536):
        q = n_bins // 4
        cases = {(1.0, 1.0): q - 1, (2.5, 2.5): q - 1,                   # |dx| == |dy|: the first rule takes it; s == 1 is clamped into the last bin
                 (-1.0, 1.0): 2 * q + q - 1, (-1.0, -1.0): 2 * q, (1.0, -1.0): 0,
                 (1.0, 0.0): q // 2, (0.0, 1.0): q + q // 2, (-1.0, 0.0): 2 * q + q // 2, (0.0, -1.0): 3 * q + q // 2,
                 (1.0, -0.0): q // 2, (-0.0, 3.0): q + q // 2,
                 (1.0, np.nextafter(1.0, 2.0)): q + q - 1,               # just past the diagonal: the second face, its last bin
                 (np.nextafter(1.0, 2.0), -1.0): 0, (-1.0, np.nextafter(-1.0, -2.0)): 3 * q,
                 (1e-300, 1e-310): bin_loop(1e-300, 1e-310, n_bins), (1e300, -1e300): 0}
        for (dx, dy), want in cases.items():
            assert bin_loop(dx, dy, n_bins) == want, (n_bins, dx, dy)
            assert int(occupancy_ref.bins_of(np.array([dx]), np.array([dy]), n_bins)[0]) == want, (n_bins, dx, dy)
        rs = np.random.RandomState(n_bins)
        dx, dy = rs.normal(size=2000) * 10.0 ** rs.randint(-3, 4, 2000), rs.normal(size=2000)
        got = occupancy_ref.bins_of(dx, dy, n_bins)
        assert got.min() >= 0 and got.max() < n_bins and got.tolist() == [bin_loop(a, b, n_bins) for a, b in zip(dx, dy)]
        turn = np.arange(16 * n_bins) * (2 * np.pi / (16 * n_bins))                    # once round
        swept = occupancy_ref.bins_of(np.cos(turn), np.sin(turn), n_bins)
        assert set(swept.tolist()) == set(range(n_bins))                 # every bin is some direction's


def test_the_scene_gives_a_free_fan_a_wall_and_unknown_behind_it():
    """A 90-degree fan of ground with a wall 6 m ahead, seven calls at one pose into 40 x 36 cells of 0.5 m, at 8, 64 and 720 bins."""
    for n_bins in (8, 64, 720):
        p = occupancy_cases.params(n_bins=n_bins, max_range=20.0)
        state = occupancy_ref.new_state(p)
        rs = np.random.RandomState(2)
        totals = np.zeros(3, np.int64)
        for _ in range(7):
            cloud = occupancy_cases.compact([occupancy_cases.fan(rs, 4000, 1500)])
            out = occupancy_ref.update(p, state, B=1, T=occupancy_cases.pose(0.1, 0.1, 0.0), **cloud)
            totals += np.bincount(out["evidence"].ravel(), minlength=3)
        assert (totals > 0).all() and totals[0] > totals[1] > totals[2], (n_bins, totals)          # unknown, free and occupied all occur
        ox, oy = out["origin"][0]
        cell_of = lambda x, y: (int(math.floor(x / 0.5)) - ox, int(math.floor(y / 0.5)) - oy)       # noqa: E731
        assert out["state"][0][cell_of(6.2, 0.3)] == 2 and out["state"][0][cell_of(6.2, -2.3)] == 2          # the wall
        assert out["state"][0][cell_of(3.1, 0.3)] == 1 and out["state"][0][cell_of(2.1, -1.2)] == 1          # the road in front of it
        assert out["state"][0][cell_of(8.3, 0.3)] == 0 and out["state"][0][cell_of(9.1, 2.2)] == 0           # behind the wall
        assert out["state"][0][cell_of(-3.0, 0.3)] == 0 and out["state"][0][cell_of(0.3, 5.2)] == 0          # outside the field of view
        assert int(out["log_odds"].max()) == p["l_max"] and int(out["log_odds"].min()) == -7 * p["l_free"]


def test_what_the_sequences_are_meant_to_show():
    """The cases do what their names say -- judged on the restatement's results: every class of evidence, a
    scroll by nothing, by one cell, into negative cells and by more than the window; the clamp and the flip; the hot cell."""
    name = "40 x 36, 720 bins, a map per frame, compact"
    want, _ = run_ref(CASES[name])
    origins = np.stack([w["origin"][0] for w in want])
    steps = np.diff(origins, axis=0)
    assert (steps[0] == 0).all() and steps[1].tolist() == [1, 0] and (origins[3] < 0).all() and (np.abs(steps[4]) > 40).any()
    for w in want:
        assert (np.bincount(w["evidence"].ravel(), minlength=3) > 0).all()
    jumped = want[5]
    assert np.array_equal(jumped["log_odds"], np.where(jumped["evidence"] == 2, 3, np.where(jumped["evidence"] == 1, -1, 0)))      # all read 0
    assert not np.array_equal(want[1]["log_odds"], want[0]["log_odds"]) and np.abs(want[4]["log_odds"]).max() > 3                  # fused
    edges, _ = run_ref(CASES["planted edges"])
    assert edges[0]["hits"].sum() == 16 and edges[1]["log_odds"].max() == 6 and (edges[0]["evidence"] == 1).sum() > 0
    sat, case = run_ref(CASES["saturation"])[0], CASES["saturation"]
    wall = sat[0]["evidence"] == 2
    assert (sat[case["n_occ"] - 1]["log_odds"][wall] == 10).all() and (sat[case["n_occ"] - 3]["log_odds"][wall] < 10).all()
    cleared = wall & (sat[case["n_occ"]]["evidence"] == 1)
    assert cleared.sum() > 3 and (sat[case["n_occ"]]["state"][cleared] == 2).all() and (sat[-1]["state"][cleared] == 1).all()
    hot = run_ref(CASES["contention"])[0][0]
    assert hot["hits"].max() == 4096 and (hot["hits"] > 0).sum() == 1 and (hot["hit_min"] != occupancy_ref.INF_BITS).sum() == 1


def test_saturation_then_the_flip():
    case = CASES["saturation"]
    got, _ = run_ref(case)
    p, n_occ = case["params"], case["n_occ"]
    wall = got[0]["evidence"] == 2
    assert wall.sum() > 5 and n_occ == p["l_max"] // p["l_occ"] + 2
    assert (got[n_occ - 3]["log_odds"][wall] < p["l_max"]).all() and (got[n_occ - 2]["log_odds"][wall] == p["l_max"]).all()
    assert (got[n_occ - 1]["log_odds"][wall] == p["l_max"]).all() and (got[n_occ - 1]["state"][wall] == 2).all()      # clamped, not wrapped
    cleared = wall & (got[n_occ]["evidence"] == 1)
    assert cleared.sum() > 3
    states = np.stack([g["state"][cleared] for g in got[n_occ:]])
    assert (states[0] == 2).all() and (states[-1] == 1).all() and (states == 0).any()                  # occupied -> unknown -> free
    assert (got[-1]["log_odds"][cleared] == -p["free_at"]).all()


def test_workspace_formula():
    assert occupancy_ref.workspace_bytes(1, 4, 1, 1, 1) == 2 * 32 + 32 + 16 + 16
    assert occupancy_ref.workspace_bytes(3, 720, 3, 40, 36) == 2 * 17280 + 80 + 17280 + 16
