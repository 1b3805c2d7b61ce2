"""CPU: tests/terrain_ref.py, the NumPy restatement of crd_terrain_update, held to include/camradepth_hip.h by plain Python loops --
one row at a time, the map kept as a dictionary keyed by world cell, so neither a torus nor a window order can hide an error -- and
to closed forms: a plane's slope, a kerb, the headroom, floor division of negative heights, the saturating weight, top >= ground,
scrolls, and cells that leave and come back."""
import math

import numpy as np
import pytest

from tests import terrain_cases, terrain_ref
from tests.terrain_cases import frame_of, params, surface

CASES = terrain_cases.all_cases()
OUT = terrain_ref.OUT
I32_MIN = -2 ** 31
NAN_BITS = np.float32(np.nan).tobytes()


class Loops:
    """The header, one row and one cell at a time."""

    def __init__(self, p):
        self.p = p
        self.head_q, self.step_max_q, self.slope2_max = terrain_ref.thresholds(p)
        M = p["M"]
        self.cells = [dict() for _ in range(M)]                        # (wx, wy) -> [ground, top, weight]
        self.origin = [(0, 0)] * M
        self.status = [0] * M

    @staticmethod
    def through(T, v):
        x, y, z = (float(c) for c in v)
        if T is None:
            return x, y, z
        return tuple(float(T[i][0]) * x + float(T[i][1]) * y + float(T[i][2]) * z + float(T[i][3]) for i in range(3))

    def update(self, xyz, B, frame_offsets=None, rows_per_frame=0, valid=None, T=None, sensor=None, centre=None):
        p, M, nx, ny = self.p, self.p["M"], self.p["nx"], self.p["ny"]
        cell, zq = float(p["cell"]), float(p["z_quantum"])
        pose_of = lambda b: None if T is None else (np.asarray(T)[b] if np.asarray(T).ndim == 3 else np.asarray(T))      # noqa: E731
        point_of = lambda v, b: (0.0, 0.0, 0.0) if v is None else (np.asarray(v)[b] if np.asarray(v).ndim == 2 else np.asarray(v))  # noqa: E731
        S = [self.through(pose_of(b), point_of(sensor, b)) for b in range(B)]
        for b in range(B):
            if not all(math.isfinite(c) for c in S[b]):
                self.status[0 if M == 1 else b] |= 2
        skipped = []
        for m in range(M):
            b = 0 if M == 1 else m
            C = self.through(pose_of(b), point_of(sensor if centre is None else centre, b))
            ok = all(math.isfinite(c) for c in C)
            if ok:
                fx, fy = math.floor(C[0] / cell), math.floor(C[1] / cell)
                ok = abs(fx) < 2 ** 31 - 65536 and abs(fy) < 2 ** 31 - 65536
            skipped.append(not ok)
            if ok:
                self.origin[m] = (fx - nx // 2, fy - ny // 2)
                ox, oy = self.origin[m]
                self.cells[m] = {k: v for k, v in self.cells[m].items() if ox <= k[0] < ox + nx and oy <= k[1] < oy + ny}
            else:
                self.status[m] |= 1
        seen = [dict() for _ in range(M)]                              # (wx, wy) -> the q of its rows
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        for r in range(len(xyz)):
            if valid is not None and not np.asarray(valid).reshape(-1)[r]:
                continue
            if frame_offsets is not None:
                owners = [b for b in range(B) if frame_offsets[b] <= r < frame_offsets[b + 1]]
                if not owners:
                    continue
                b = owners[0]
            else:
                b = r // rows_per_frame
                if b >= B:
                    continue
            X, Y, Z = self.through(pose_of(b), xyz[r])
            if not all(math.isfinite(c) for c in (X, Y, Z) + tuple(S[b])):
                continue
            dx, dy = X - S[b][0], Y - S[b][1]
            if dx * dx + dy * dy > float(p["max_range"]) * float(p["max_range"]):
                continue
            if Z < p["z_range"][0] or Z > p["z_range"][1]:
                continue
            m = 0 if M == 1 else b
            wx, wy = math.floor(X / cell), math.floor(Y / cell)
            ox, oy = self.origin[m]
            if not (ox <= wx < ox + nx and oy <= wy < oy + ny):
                continue
            seen[m].setdefault((wx, wy), []).append(math.floor(Z / zq))
        out = {k: np.zeros((M, nx, ny), dt) for k, dt in (("ground", np.int32), ("top", np.int32), ("step", np.int32), ("slope2", np.int64),
                                                          ("weight", np.int16), ("state", np.uint8), ("hazard", np.uint8), ("evidence", np.uint8),
                                                          ("value", np.float32))}
        out["origin"] = np.array(self.origin, np.int64).reshape(M, 2)
        for m in range(M):
            cells = self.cells[m]
            if not skipped[m]:
                for key, qs in seen[m].items():
                    if len(qs) < p["min_points"]:
                        continue
                    lo = min(qs)
                    hi = max(q for q in qs if q <= lo + self.head_q)
                    if key in cells:
                        g, t, w = cells[key]
                        cells[key] = [(w * g + lo) // (w + 1), (w * t + hi) // (w + 1), min(w + 1, p["w_max"])]
                    else:
                        cells[key] = [lo, hi, min(1, p["w_max"])]
                    out["evidence"][m, key[0] - self.origin[m][0], key[1] - self.origin[m][1]] = 1
            ox, oy = self.origin[m]
            for i in range(nx):
                for j in range(ny):
                    key = (ox + i, oy + j)
                    if key not in cells:
                        out["ground"][m, i, j] = out["top"][m, i, j] = I32_MIN
                        out["hazard"][m, i, j] = 255
                        out["value"][m, i, j] = np.nan
                        continue
                    g, t, w = cells[key]
                    near = {(di, dj): cells[(key[0] + di, key[1] + dj)][0] for di in (-1, 0, 1) for dj in (-1, 0, 1)
                            if (di or dj) and 0 <= i + di < nx and 0 <= j + dj < ny and (key[0] + di, key[1] + dj) in cells}
                    step = max([t - g] + [abs(v - g) for v in near.values()])
                    grad = []
                    for a, b2 in (((-1, 0), (1, 0)), ((0, -1), (0, 1))):
                        if a in near and b2 in near:
                            grad.append(near[b2] - near[a])
                        elif b2 in near:
                            grad.append(2 * (near[b2] - g))
                        elif a in near:
                            grad.append(2 * (g - near[a]))
                        else:
                            grad.append(0)
                    slope2 = grad[0] * grad[0] + grad[1] * grad[1]
                    occupied = step > self.step_max_q or slope2 > self.slope2_max
                    out["ground"][m, i, j], out["top"][m, i, j], out["weight"][m, i, j] = g, t, w
                    out["step"][m, i, j], out["slope2"][m, i, j] = step, slope2
                    out["state"][m, i, j] = 2 if occupied else 1
                    out["hazard"][m, i, j] = 254 if occupied else max(step * 253 // self.step_max_q, slope2 * 253 // self.slope2_max)
                    out["value"][m, i, j] = np.float32(float(g) * zq)
        return out


def same(got, want, what):
    for k in OUT:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, k, np.argwhere(a != b)[:4].tolist())


def run(p, frames, B=1):
    state = terrain_ref.new_state(p)
    return [terrain_ref.update(p, state, B=B, **f) for f in frames], state


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_against_plain_loops(name):
    case = CASES[name]
    state, loops = terrain_ref.new_state(case["params"]), Loops(case["params"])
    for step, f in enumerate(case["frames"]):
        got, want = terrain_ref.update(case["params"], state, B=case["B"], **f), loops.update(B=case["B"], **f)
        same(got, want, f"{name}, call {step}")
        assert state["status"].tolist() == loops.status, (name, step)
        known = state["weight"] != 0
        assert (state["top"] >= state["ground"]).all() and not state["ground"][~known].any() and not state["top"][~known].any()


def test_the_cases_reach_every_branch():
    seen = {"states": set(), "hazards": set(), "scrolled": set(), "skipped": False, "above": False, "one_sided": False}
    for name, case in CASES.items():
        results, _ = run(case["params"], case["frames"], case["B"])
        origins = [r["origin"][0].tolist() for r in results]
        seen["scrolled"] |= {(abs(a[0] - b[0]) >= case["params"]["nx"], a == b) for a, b in zip(origins, origins[1:])}
        for r in results:
            seen["states"] |= set(np.unique(r["state"]).tolist())
            seen["hazards"] |= set(np.unique(r["hazard"]).tolist())
            seen["skipped"] |= not r["moved"].all()
            seen["above"] |= bool(((r["hi"] > r["lo"] + 128) & (r["n"] > 0)).any()) or bool((r["n"] > 0).any() and name == "contention")
    assert seen["states"] == {0, 1, 2} and {0, 254, 255} <= seen["hazards"] and len(seen["hazards"]) > 20
    assert {(True, False), (False, True), (False, False)} <= seen["scrolled"] and seen["skipped"]
    assert any(min(o) < 0 for case in CASES.values() for o in [run(case["params"], case["frames"], case["B"])[0][-1]["origin"].ravel().tolist()])
    r = run(CASES["contention"]["params"], CASES["contention"]["frames"])[0][0]
    i, j = np.argwhere(r["n"][0] > 0)[0]
    assert r["n"][0, i, j] == 4096 and r["lo"][0, i, j] == -2048 and r["hi"][0, i, j] == -2048 + 128      # lo + head_q exactly
    assert (CASES["runs"]["frames"][0]["xyz"].shape[0] % 64, CASES["runs"]["frames"][0]["xyz"].shape[0] % 256) != (0, 0)


@pytest.mark.parametrize("a, b", [(1, 0), (0, 2), (2, -3), (-4, 1)])
def test_a_plane_has_its_slope_in_every_cell(a, b):
    """Z = (a' X + b' Y) with a' cell / z_quantum = a and b' cell / z_quantum = b whole, sampled at the cell centres: (2a)^2 + (2b)^2 in
    the interior and on the edges alike, since the one-sided difference is doubled; the state flips between slope2_max and
    slope2_max + 1."""
    nx, ny, q = 9, 7, 1.0 / 64
    cloud = surface(lambda wx, wy: (a * (wx + 0.5) + b * (wy + 0.5) + 0.5) * q, nx, ny)
    slope2 = 4 * a * a + 4 * b * b
    for slope2_max, state in ((slope2, 1), (slope2 - 1, 2)):
        slope_max = math.sqrt(slope2_max + 0.5) * q / (2 * 0.5)                       # floor((2 * cell * slope_max / z_quantum)^2) = slope2_max
        p = params(nx=nx, ny=ny, slope_max=slope_max, step_max=8.0)
        assert terrain_ref.thresholds(p)[2] == slope2_max
        r = run(p, [frame_of(cloud)])[0][0]
        assert (r["slope2"] == slope2).all() and (r["state"] == state).all() and (r["weight"] == 1).all()
        assert (r["step"][0, 1:-1, 1:-1] == abs(a) + abs(b)).all()                     # the diagonal neighbour, which two corners lack
        assert (r["step"] >= max(abs(a), abs(b))).all() and (r["step"] <= abs(a) + abs(b)).all()
        want = np.fromfunction(lambda i, j: np.floor(a * (i - nx // 2 + 0.5) + b * (j - ny // 2 + 0.5) + 0.5), (nx, ny))
        assert (r["ground"][0] == want).all() and (r["value"][0] == (want * q).astype(np.float32)).all()
        assert (r["hazard"] == (254 if state == 2 else max((abs(a) + abs(b)) * 253 // 512, slope2 * 253 // slope2_max))).all()
    lone = run(params(nx=1, ny=1), [frame_of(surface(lambda wx, wy: 0.25, 1, 1))])[0][0]
    assert lone["slope2"].tolist() == [[[0]]] and lone["step"].tolist() == [[[0]]] and lone["state"].tolist() == [[[1]]]
    strip = run(params(nx=3, ny=1, slope_max=8.0, step_max=8.0), [frame_of(surface(lambda wx, wy: np.array([[0.0], [5.0], [0.0]]) * q + wx * 0, 3, 1)[[0, 1, 4, 5]])])[0][0]
    assert strip["slope2"][0, :, 0].tolist() == [0, 0, 0] and strip["weight"][0, :, 0].tolist() == [1, 0, 1]      # no known neighbour along i


def test_a_kerb_of_15_quanta():
    nx, ny, q = 8, 6, 1.0 / 64
    cloud = surface(lambda wx, wy: np.where(wx >= 0, 15 * q, 0.0) + 0.25 * q, nx, ny)
    for step_max_q, state in ((20, 1), (14, 2), (15, 1)):
        p = params(nx=nx, ny=ny, step_max=step_max_q * q, slope_max=8.0)
        assert terrain_ref.thresholds(p)[1] == step_max_q
        r = run(p, [frame_of(cloud)])[0][0]
        edge = r["step"][0, 3:5] == 15
        assert edge.all() and (r["step"][0, :3] == 0).all() and (r["step"][0, 5:] == 0).all()
        assert (r["state"][0, 3:5] == state).all() and (r["state"][0, :3] == 1).all() and (r["state"][0, 5:] == 1).all()       # both cells that share the edge
        assert (r["hazard"][0, 3:5] == (254 if state == 2 else 15 * 253 // step_max_q)).all()


def test_the_headroom_is_closed_at_lo_plus_head_q():
    q = 1.0 / 64
    p = params(nx=1, ny=1, headroom=128 * q, min_points=1, step_max=8.0)
    at = lambda *z: frame_of([(0.1, 0.1 + 0.01 * k, v * q) for k, v in enumerate(z)])      # noqa: E731
    assert run(p, [at(-3, 125, 126)])[0][0]["top"].tolist() == [[[125]]]
    assert run(p, [at(126, 125, -3)])[0][0]["top"].tolist() == [[[125]]]
    assert run(p, [at(-3, 124, 126, 400)])[0][0]["top"].tolist() == [[[124]]]
    r = run(p, [at(7, 400, 500)])[0][0]
    assert (r["ground"].tolist(), r["top"].tolist(), r["step"].tolist(), r["n"].tolist()) == ([[[7]]], [[[7]]], [[[0]]], [[[3]]])
    assert run(params(nx=1, ny=1, headroom=0.0, min_points=1), [at(5, 6)])[0][0]["top"].tolist() == [[[5]]]


def test_negative_heights_use_floor_division():
    assert (3 * -7 + -8) // 4 == -8 and int((3 * -7 + -8) / 4) == -7
    q = 1.0 / 64
    p = params(nx=1, ny=1, min_points=1, w_max=15, step_max=8.0)
    at = lambda z: frame_of([(0.1, 0.1, z * q)])      # noqa: E731
    results, state = run(p, [at(-7)] * 3 + [at(-8)])
    assert [r["ground"][0, 0, 0] for r in results] == [-7, -7, -7, -8] and state["weight"].tolist() == [[[4]]]
    assert run(p, [frame_of([(0.1, 0.1, -0.5 * q)])])[0][0]["ground"].tolist() == [[[-1]]]                   # q itself is a floor as well


def test_the_weight_saturates_and_the_filter_follows():
    case = CASES["saturation"]
    w_max = case["params"]["w_max"]
    results, state = run(case["params"], case["frames"])
    assert [int(r["weight"].max()) for r in results] == [min(k + 1, w_max) for k in range(len(results))]
    ground = [int(r["ground"][0, 0, 0]) for r in results]
    assert ground[:w_max + 2] == [-32] * (w_max + 2)
    g = -32
    for k in range(4):
        g = (w_max * g + 31) // (w_max + 1)
        assert ground[w_max + 2 + k] == g
    assert ground[-1] < 31 and ground[-1] - ground[-2] == (31 - ground[-2]) // (w_max + 1)


def test_top_stays_above_ground_over_a_random_sequence():
    rs = np.random.RandomState(3)
    p = params(nx=6, ny=6, min_points=1, w_max=5)
    state = terrain_ref.new_state(p)
    for _ in range(40):
        n = rs.randint(1, 80)
        xyz = np.stack([rs.uniform(-1.5, 1.5, n), rs.uniform(-1.5, 1.5, n), rs.choice([-7.9, -1.0, 0.0, 0.3, 2.5, 7.9], n) + rs.uniform(-0.1, 0.1, n)], axis=1)
        r = terrain_ref.update(p, state, B=1, **frame_of(xyz, T=terrain_cases.pose(rs.uniform(-0.6, 0.6), rs.uniform(-0.6, 0.6), rs.uniform(-3, 3))))
        known = r["weight"] > 0
        assert (r["top"][known] >= r["ground"][known]).all() and (state["top"] >= state["ground"]).all()
        assert (r["step"][known] >= (r["top"] - r["ground"])[known]).all()


def test_scrolls_and_a_cell_that_leaves_and_comes_back():
    nx, ny = 6, 4
    p = params(nx=nx, ny=ny, min_points=1)
    ground = lambda wx, wy: (3 * wx + 5 * wy) / 64.0 + 1.0 / 128      # noqa: E731
    wide = surface(ground, 40, 40)                                      # the world cells -20 .. 19: whatever the window, it is covered
    none = np.zeros((0, 3), np.float32)
    at = lambda x, y, cloud=none: frame_of(cloud, sensor=np.array([x, y, 0.0]), centre=np.array([x, y, 0.0]))      # noqa: E731
    results, state = run(p, [at(0.1, 0.1, wide), at(0.1, 0.1), at(0.6, 0.1), at(-1.4, -0.9), at(0.1, 0.1), at(9.1, 0.1), at(0.1, 0.1)])
    first = results[0]
    assert first["origin"].tolist() == [[-3, -2]] and (first["weight"] == 1).all()
    want = np.fromfunction(lambda i, j: 3 * (i - 3) + 5 * (j - 2), (nx, ny))
    assert (first["ground"][0] == want).all()
    same(results[1], dict(first, evidence=np.zeros_like(first["evidence"])), "a scroll by nothing keeps everything")
    one = results[2]                                                     # one cell on along x: the last row of the window is new
    assert one["origin"].tolist() == [[-2, -2]] and (one["ground"][0, :-1] == want[1:]).all() and (one["weight"][0, -1] == 0).all()
    assert (one["state"][0, -1] == 0).all() and (one["hazard"][0, -1] == 255).all() and np.isnan(one["value"][0, -1]).all()
    neg = results[3]                                                     # into negative cells: the window -6 .. -1 by -4 .. -1
    assert neg["origin"].tolist() == [[-6, -4]]
    keeps = np.zeros((nx, ny), bool)
    keeps[4:, 2:] = True                                                # the world cells -2, -1 by -2, -1 were in every window so far
    assert ((neg["weight"][0] == 1) == keeps).all() and (neg["ground"][0][keeps] == want[1:3, :2].ravel()).all()
    back = results[4]                                                    # the first window again: what left it reads as unknown
    assert back["origin"].tolist() == [[-3, -2]] and ((back["weight"][0] == 1) == np.pad(np.ones((2, 2), bool), ((1, 3), (0, 2)))).all()
    far = results[5]                                                     # past the whole window: nothing is left
    assert far["origin"].tolist() == [[15, -2]] and not far["weight"].any() and (far["state"] == 0).all()
    assert not results[6]["weight"].any() and not state["weight"].any()


def test_workspace_bytes_and_thresholds():
    assert terrain_ref.workspace_bytes(3, 3, 40, 36) == 3 * 17280 + 80 + 16 and terrain_ref.workspace_bytes(1, 1, 1, 1) == 3 * 16 + 32 + 16
    assert terrain_ref.thresholds(dict(cell=0.5, z_quantum=0.01, headroom=2.5, step_max=0.25, slope_max=0.35)) == (250, 25, 1225)
    assert terrain_ref.thresholds(dict(cell=0.5, z_quantum=0.01, headroom=0.0, step_max=0.0, slope_max=0.0)) == (0, 1, 1)
    assert terrain_ref.thresholds(dict(cell=0.5, z_quantum=1e-300, headroom=1.0, step_max=1.0, slope_max=1.0)) == (2 ** 30, 2 ** 30, 2 ** 62)
