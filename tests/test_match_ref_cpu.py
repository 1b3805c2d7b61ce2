"""CPU: tests/match_ref.py, the NumPy restatement of crd_match_scan, held (a) to a plain loop over candidates and points into a
dictionary of world cells, (b) to planted offsets -- the scene fused from one pose and seen again with the prior off by a known (turn,
dx, dy) inside the window: the pick is the exact inverse; a corridor and a point-symmetric scene, where the tie rule is asserted and
not recovery -- and (c) to invariants: the centre candidate's scan cells are the cells where the update reports evidence 2 from the
same frame, prior_score is the table's centre, and every guard returns the prior's bits."""
import copy
import math

import numpy as np
import pytest

from tests import match_cases, match_ref, occupancy_ref
from tests.bev_ref import frames_of

CASES = match_cases.all_cases()
_OUT = {}


def out_of(name, i):
    """The restatement's outputs of match i of case `name`, computed once and left unchanged."""
    if (name, i) not in _OUT:
        _OUT[name, i] = match_cases.match_of(CASES[name], match_cases.state_of(name, CASES[name]), i)
    return _OUT[name, i]


def every_match():
    return [(name, i) for name, c in CASES.items() for i in range(len(c["matches"]))]


def loop_match(case, state, match):
    """The header, row by row and candidate by candidate in Python floats, every finite world cell of every turn in a dictionary ->
    (table [M,NT,NS,NS], n_cells [M])."""
    p, spec, kw, B = case["params"], match["spec"], match["kw"], case["B"]
    M, nx, ny, cell, n_xy, n_theta = p["M"], p["nx"], p["ny"], float(p["cell"]), spec["n_xy"], spec["n_theta"]
    min_points = p["min_points"] if spec["min_points"] is None else spec["min_points"]
    T = match_ref.poses_of(kw.get("T"), B).tolist()
    sensor = occupancy_ref.per_frame(kw.get("sensor"), B).tolist()

    def through(A, v):
        return [A[r][0] * v[0] + A[r][1] * v[1] + A[r][2] * v[2] + A[r][3] for r in range(3)]

    S = [through(T[b], sensor[b]) for b in range(B)]
    xyz = np.asarray(kw["xyz"], np.float32).reshape(-1, 3)
    frame = frames_of(len(xyz), B, kw.get("frame_offsets"), kw.get("rows_per_frame", 0))
    valid = kw.get("valid")
    cells = [[{} for _ in range(2 * n_theta + 1)] for _ in range(M)]
    for r, (b, row) in enumerate(zip(frame.tolist(), xyz.astype(np.float64).tolist())):
        if b < 0 or (valid is not None and not valid[r]):
            continue
        X, Y, Z = through(T[b], row)
        if not all(math.isfinite(v) for v in (X, Y, Z, *S[b])):
            continue
        dx, dy = X - S[b][0], Y - S[b][1]
        r2 = dx * dx + dy * dy
        if not (0.0 < r2 <= float(p["max_range"]) * float(p["max_range"]) and p["z_lo"] <= Z <= p["z_hi"]):
            continue
        m, about = (0, S[0]) if M == 1 else (b, S[b])
        for t in range(2 * n_theta + 1):
            A = T[b]
            if t != n_theta:
                a = (t - n_theta) * spec["d_theta"]
                c, s = math.cos(a), math.sin(a)
                A = [[c * A[0][k] - s * A[1][k] for k in range(3)] + [(c * A[0][3] - s * A[1][3]) + (about[0] - (c * about[0] - s * about[1]))],
                     [s * A[0][k] + c * A[1][k] for k in range(3)] + [(s * A[0][3] + c * A[1][3]) + (about[1] - (s * about[0] + c * about[1]))], A[2]]
            Xt, Yt, _ = through(A, row)
            if math.isfinite(Xt) and math.isfinite(Yt):
                key = (math.floor(Xt / cell), math.floor(Yt / cell))
                cells[m][t][key] = cells[m][t].get(key, 0) + 1
    table, n_cells = np.zeros((M, 2 * n_theta + 1, 2 * n_xy + 1, 2 * n_xy + 1), np.int64), np.zeros(M, np.int32)
    for m in range(M):
        ox, oy = (int(v) for v in state["cur_origin"][m])

        def L(wx, wy):
            if state["initialised"][m] == 0 or not (ox <= wx < ox + nx and oy <= wy < oy + ny):
                return 0
            return int(state["map"][m][wx % nx, wy % ny])

        for t in range(2 * n_theta + 1):
            scan = [k for k, count in cells[m][t].items() if count >= min_points]
            if t == n_theta:
                n_cells[m] = sum(1 for wx, wy in scan if ox <= wx < ox + nx and oy <= wy < oy + ny)
            for dx in range(-n_xy, n_xy + 1):
                for dy in range(-n_xy, n_xy + 1):
                    table[m, t, dx + n_xy, dy + n_xy] = sum(L(wx + dx, wy + dy) for wx, wy in scan)
    return table, n_cells


LOOPED = ["37 x 53, planted offsets", "64 x 65, turns only", "a point-symmetric scene", "two posts, one seen between them", "three maps, compact",
          "one rig of three frames, bare xyz", "three maps, a NaN pose for one", "contention", "the guards", "an uninitialised map"]


@pytest.mark.parametrize("name", LOOPED)
def test_the_restatement_equals_a_plain_loop(name):
    c = CASES[name]
    state = match_cases.state_of(name, c)
    for i, match in enumerate(c["matches"][:3]):
        table, n_cells = loop_match(c, state, match)
        out = out_of(name, i)
        assert np.array_equal(table, out["scores"]), (name, i, int((table != out["scores"]).sum()))
        assert np.array_equal(n_cells, out["n_cells"]), (name, i)
        n_xy, n_theta = match["spec"]["n_xy"], match["spec"]["n_theta"]
        for m in range(c["params"]["M"]):                                  # the pick: the least of a sorted list of keys
            keys = sorted((-int(v), (ix - n_xy) ** 2 + (iy - n_xy) ** 2, abs(t - n_theta), t, ix - n_xy, iy - n_xy) for (t, ix, iy), v in np.ndenumerate(table[m]))
            assert (keys[0][3] - n_theta, keys[0][4], keys[0][5]) == tuple(out["pick"][m].tolist()) and -keys[0][0] == out["score"][m]


def test_planted_offsets_are_recovered():
    seen = 0
    for name, i in every_match():
        planted = CASES[name]["matches"][i].get("planted")
        if planted is None or name in ("a corridor", "an uninitialised map"):
            continue
        out, M = out_of(name, i), CASES[name]["params"]["M"]
        for m in range(M):
            if out["status"][m] & match_ref.KEEPS_PRIOR:
                assert name == "three maps, a NaN pose for one" and m == 1
                continue
            assert tuple(out["pick"][m].tolist()) == planted, (name, i, m, out["pick"][m].tolist())
            assert out["score"][m] > out["prior_score"][m] or planted == (0, 0, 0)
            seen += 1
    assert seen >= 20


def test_the_corrected_pose_is_the_true_pose():
    """The pose that goes out of a planted match is the pose the map was built from, to rounding."""
    name = "37 x 53, planted offsets"
    truth = CASES[name]["build"][0]["T"]
    for i in range(len(CASES[name]["matches"])):
        assert np.abs(out_of(name, i)["pose"][0] - truth).max() < 1e-12, i


def test_the_tie_rule_on_a_corridor_and_on_symmetric_scenes():
    for i, want in ((0, (0, 0, 1)), (1, (0, 0, 0))):                        # along the corridor every shift scores the same: dx stays
        out = out_of("a corridor", i)
        table = out["scores"][0]
        assert tuple(out["pick"][0].tolist()) == want
        assert (table[1, :, 3 + want[2]] == out["score"][0]).all() and (table == out["score"][0]).sum() == 7
    out = out_of("a point-symmetric scene", 0)
    table = out["scores"][0]
    occupied = match_ref.window_log_odds(CASES["a point-symmetric scene"]["params"], match_cases.state_of("a point-symmetric scene", CASES["a point-symmetric scene"]), 0) > 0
    assert occupied.sum() == 4 and np.array_equal(occupied, occupied[::-1, ::-1])          # about the sensor's cell, the window's middle
    assert np.array_equal(table[2] == table.max(), (table[2] == table.max())[::-1, ::-1]) and table.max() > 0
    assert tuple(out["pick"][0].tolist()) == (0, 0, 0) and (table == out["score"][0]).sum() > 1 and out["status"][0] == 0
    assert out["pose"].tobytes() == match_ref.poses_of(CASES["a point-symmetric scene"]["matches"][0]["kw"]["T"], 1).tobytes()
    out = out_of("two posts, one seen between them", 0)
    table = out["scores"][0, 0]
    assert table[3 - 2, 3] == table[3 + 2, 3] == out["score"][0] > table[3, 3] and (table == out["score"][0]).sum() == 2
    assert tuple(out["pick"][0].tolist()) == (0, -2, 0)                                    # equal radius and turn: the least dx


@pytest.mark.parametrize("name,i", [("37 x 53, planted offsets", 0), ("a point-symmetric scene", 0), ("two posts, one seen between them", 0), ("the guards", 0)])
def test_the_centre_candidate_sees_the_updates_cells(name, i):
    c, match = CASES[name], CASES[name]["matches"][i]
    state = copy.deepcopy(match_cases.state_of(name, c))
    kw, spec, p = match["kw"], match["spec"], c["params"]
    before = state["cur_origin"].copy()
    res = occupancy_ref.update(p, state, kw["xyz"], c["B"], frame_offsets=kw.get("frame_offsets"), rows_per_frame=kw.get("rows_per_frame", 0),
                               valid=kw.get("valid"), T=kw.get("T"), sensor=kw.get("sensor"), centre=None)
    assert np.array_equal(before, state["cur_origin"])                                    # the window did not move
    out, n = out_of(name, i), spec["n_xy"]
    min_points = p["min_points"] if spec["min_points"] is None else spec["min_points"]
    assert min_points == p["min_points"]
    scan = out["counts"][:, spec["n_theta"], n:n + p["nx"], n:n + p["ny"]] >= min_points
    assert np.array_equal(scan, res["evidence"] == 2) and scan.sum() == out["n_cells"].sum() > 0


@pytest.mark.parametrize("name,i", every_match())
def test_invariants_of_every_match(name, i):
    c, out = CASES[name], out_of(name, i)
    spec, kw, B, M = c["matches"][i]["spec"], c["matches"][i]["kw"], c["B"], c["params"]["M"]
    n_xy, n_theta = spec["n_xy"], spec["n_theta"]
    prior = match_ref.poses_of(kw.get("T"), B)
    assert np.array_equal(out["prior_score"], out["scores"][:, n_theta, n_xy, n_xy])
    assert np.array_equal(out["score"], out["scores"].reshape(M, -1).max(axis=1)) and (out["score"] >= out["prior_score"]).all()
    assert out["T_c"][:, n_theta].tobytes() == prior.tobytes()
    for m in range(M):
        fed = range(B) if M == 1 else [m]
        if out["status"][m] & match_ref.KEEPS_PRIOR:
            assert all(out["pose"][b].tobytes() == prior[b].tobytes() for b in fed) and not out["status"][m] & match_ref.ON_BORDER
        elif not out["pick"][m].any():
            assert all(np.array_equal(out["pose"][b], prior[b]) for b in fed)


def test_scan_cells_outside_the_window_are_held():
    """The far posts stand outside a window 37 cells wide: one within n_xy = 3 cells of its edge, which the count grid holds, one beyond,
    which only the grid of n_xy = 16 holds."""
    for name, outside in (("37 x 53, planted offsets", 1), ("37 x 53, n_xy 16 with n_theta 2", 2), ("three maps, compact", 3)):
        c, out = CASES[name], out_of(name, 0)
        n, p = c["matches"][0]["spec"]["n_xy"], c["params"]
        scan = out["counts"][:, c["matches"][0]["spec"]["n_theta"]] >= p["min_points"]
        assert scan.sum() - scan[:, n:n + p["nx"], n:n + p["ny"]].sum() == outside and scan[:, n:n + p["nx"], n:n + p["ny"]].sum() == out["n_cells"].sum()


def test_the_guards_each_raise_their_bit():
    g = [int(out_of("the guards", i)["status"][0]) for i in range(5)]
    assert g[0] == match_ref.FEW_CELLS and g[1] == match_ref.LOW_SCORE and g[2] & match_ref.NOT_FINITE and g[3] == match_ref.ON_BORDER and g[4] == 0
    assert max(abs(v) for v in out_of("the guards", 3)["pick"][0].tolist()) == 1
    assert out_of("an uninitialised map", 0)["status"][0] & match_ref.UNINITIALISED and not out_of("an uninitialised map", 0)["scores"].any()
    assert out_of("three maps, a NaN pose for one", 0)["status"].tolist() == [0, 14, 0]
    assert [int(out_of("contention", i)["n_cells"][0]) for i in range(3)] == [1, 1, 0]


def test_the_workspace_formula_and_the_turn_table():
    assert match_ref.workspace_bytes(1, 1, 1, 1, 0, 0) == 96 + 32 + 16 + 16
    assert match_ref.workspace_bytes(3, 3, 37, 53, 2, 2) == 96 * 15 + 80 + ((4 * 3 * 5 * 41 * 57 + 15) & ~15) + ((8 * 3 * 5 * 25 + 15) & ~15)
    rot = match_ref.rot_table(4, math.radians(0.5))
    assert rot.shape == (9, 2) and rot[4].tolist() == [1.0, 0.0] and rot[5, 1] == math.sin(math.radians(0.5)) and rot[3, 1] == -rot[5, 1]
