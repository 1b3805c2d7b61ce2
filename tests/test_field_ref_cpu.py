"""CPU: tests/field_ref.py, the NumPy restatement of the distance field that the GPU tests compare the kernels with, against plain
statements of the same thing: a brute-force loop over all sources of the window (least squared distance, ties to the lowest window
index), scipy's exact Euclidean distance transform where the field is not truncated, a loop over the entries of the tables, and a
per-pose loop of the path check.  It also asserts what the case set has to hold so that no GPU test passes vacuously."""
import math

import numpy as np
import pytest

from tests import field_cases, field_ref

CASES = field_cases.all_cases()
PATHS = field_cases.path_cases()
_FIELD = {}


def field_of(name):
    """The restatement's field of case `name`, computed once and left unchanged."""
    if name not in _FIELD:
        c = CASES[name]
        clear, cost = field_ref.tables(c["cell"], c["R"], **c["table"])
        _FIELD[name] = field_ref.distance_field(c["state"], c["sources"], c["R"], c["unknown_cost"], clear, cost)
    return _FIELD[name]


def brute(src, R):
    """Per cell the least squared distance over ALL sources of the map, ties to the lowest i' * ny + j'; and how many reach it."""
    nx, ny = src.shape
    far = R * R + 1
    d2, near, ties = np.full((nx, ny), far, np.int64), np.full((nx, ny), -1, np.int64), np.zeros((nx, ny), np.int64)
    ii, jj = np.nonzero(src)
    if len(ii) == 0:
        return d2, near, ties
    for i in range(nx):
        for j in range(ny):
            t = (ii - i) ** 2 + (jj - j) ** 2
            least = t.min()
            ties[i, j] = (t == least).sum()
            if least <= R * R:
                d2[i, j] = least
                near[i, j] = (ii[t == least] * ny + jj[t == least]).min()
    return d2, near, ties


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_passes_equal_brute_force_and_the_case_holds_its_condition(name):
    c = CASES[name]
    got = field_of(name)
    R, far = c["R"], c["R"] * c["R"] + 1
    src = field_ref.is_source(c["state"], c["sources"])
    most_ties = 0
    for m in range(src.shape[0]):
        d2, near, ties = brute(src[m], R)
        assert np.array_equal(got["dist2"][m], d2) and np.array_equal(got["nearest"][m], near), (name, m)
        most_ties = max(most_ties, int(ties.max()))
    assert got["dist2"].dtype == got["nearest"].dtype == got["row_near"].dtype == np.int32
    far_share = float((got["dist2"] == far).mean())
    if c["kind"] == "mixed":
        assert 0.1 <= far_share <= 0.9, (name, far_share)
    elif c["kind"] == "covered":
        assert R >= max(src.shape[1:]) and src.any() and not src.all()
    elif c["kind"] == "uniform":
        assert far_share in (0.0, 1.0) and len(np.unique(got["dist2"])) == 1
    elif c["kind"] == "ties":
        assert most_ties >= 2, name
    cost = got["cost"]
    assert np.array_equal(got["clearance"] == np.inf, got["dist2"] == far)
    if c["unknown_cost"]:
        assert (cost[c["state"] == 0] >= c["unknown_cost"]).all()


def test_placed_ties_go_to_the_left_the_upper_and_the_lower_index():
    got = field_of("placed ties")
    ny = 11
    assert got["dist2"][0, 1, 4] == 4 and got["nearest"][0, 1, 4] == 1 * ny + 2 and got["row_near"][0, 1, 4] == 2        # the left one of a row
    assert got["dist2"][1, 5, 9] == 4 and got["nearest"][1, 5, 9] == 3 * ny + 9                                       # the upper one of a column
    assert got["dist2"][2, 5, 3] == 1 and got["nearest"][2, 5, 3] == 5 * ny + 2                                       # a diagonal pair
    assert got["dist2"][2, 6, 2] == 1 and got["nearest"][2, 6, 2] == 5 * ny + 2
    digits = field_of("states 0 .. 9")
    state = CASES["states 0 .. 9"]["state"]
    assert set(np.unique(state[digits["dist2"] == 0])) == {2, 5} and (state >= 8).any()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if field_ref.is_source(c["state"], c["sources"]).any()])
def test_against_scipy_where_the_field_is_not_truncated(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    c = CASES[name]
    got = field_of(name)
    src = field_ref.is_source(c["state"], c["sources"])
    for m in range(src.shape[0]):
        if not src[m].any():
            continue
        e = ndimage.distance_transform_edt(~src[m])
        e2 = np.rint(e * e).astype(np.int64)
        near = got["dist2"][m] <= c["R"] ** 2
        assert np.array_equal(e2[near], got["dist2"][m][near]) and (e2[~near] > c["R"] ** 2).all(), (name, m)


@pytest.mark.parametrize("cell,R,opts", [(0.5, 32, {}), (0.2, 255, dict(inscribed=0.6, inflation=20.0, scale=0.3)), (0.1, 1, {}),
                                         (0.5, 8, dict(inscribed=1.0, inflation=3.0, scale=1.0)), (2.0, 5, dict(scale=0.0))])
def test_tables_against_a_loop_over_the_squared_distances(cell, R, opts):
    from camradepth_amd import field
    clear, cost = field.tables(cell, R, **opts)
    clear_ref, cost_ref = field_ref.tables(cell, R, **opts)
    far = R * R + 1
    inscribed, scale = opts.get("inscribed", 0.0), opts.get("scale", 10.0)
    inflation = opts.get("inflation", R * cell)
    want_clear, want_cost = np.zeros(far + 1, np.float32), np.zeros(far + 1, np.uint8)
    for d2 in range(far + 1):
        d = np.float64(cell) * np.sqrt(np.float64(d2))
        want_clear[d2] = np.float32(d) if d2 < far else np.inf
        if d2 == far:
            want_cost[d2] = 0
        elif d2 == 0:
            want_cost[d2] = 254
        elif d <= inscribed:
            want_cost[d2] = 253
        elif d <= inflation:
            want_cost[d2] = int(252 * np.exp(-np.float64(scale) * (d - np.float64(inscribed))))
    for a, b in ((clear, clear_ref), (clear, want_clear)):
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    for a, b in ((cost, cost_ref), (cost, want_cost)):
        assert a.dtype == b.dtype == np.uint8 and a.shape == (far + 1,) and np.array_equal(a, b)
    assert (np.diff(clear[:far]) > 0).all() and (np.diff(cost[1:far].astype(int)) <= 0).all() and cost.max() == 254


def path_field():
    state = field_cases.path_map_state()
    clear, cost = field_ref.tables(field_cases.PATH_CELL, field_cases.PATH_R)
    return state, field_ref.distance_field(state, 1 << field_cases.OCCUPIED, field_cases.PATH_R, 0, clear, cost)


def loop_paths(xy, n_poses, path_map, origin, cell, state, dist2, cost, R, blocked_at, outside_blocks):
    K, P = xy.shape[:2]
    M, nx, ny = state.shape
    out = {"first_blocked": np.full(K, -1, np.int32), "max_cost": np.zeros(K, np.uint8), "min_dist2": np.full(K, R * R + 1, np.int32),
           "n_outside": np.zeros(K, np.int32), "n_unknown": np.zeros(K, np.int32), "pose_cell": np.full((K, P), -2, np.int32)}
    for k in range(K):
        n = P if n_poses is None else int(n_poses[k])
        m = 0 if path_map is None else int(path_map[k])
        for p in range(min(max(n, 0), P)):
            X, Y = float(xy[k, p, 0]), float(xy[k, p, 1])
            inside = 0 <= m < M and math.isfinite(X) and math.isfinite(Y)
            if inside:
                wx, wy = math.floor(X / cell), math.floor(Y / cell)                   # exact integers of the fp64 quotient
                ox, oy = int(origin[m, 0]), int(origin[m, 1])
                inside = ox <= wx < ox + nx and oy <= wy < oy + ny
            if inside:
                i, j = wx - ox, wy - oy
                out["pose_cell"][k, p] = i * ny + j
                out["max_cost"][k] = max(out["max_cost"][k], cost[m, i, j])
                out["min_dist2"][k] = min(out["min_dist2"][k], dist2[m, i, j])
                out["n_unknown"][k] += state[m, i, j] == 0
                blocked = cost[m, i, j] >= blocked_at
            else:
                out["pose_cell"][k, p] = -1
                out["n_outside"][k] += 1
                blocked = bool(outside_blocks)
            if blocked and out["first_blocked"][k] < 0:
                out["first_blocked"][k] = p
    return out


def test_the_path_check_against_a_loop_over_the_poses():
    state, f = path_field()
    assert (f["dist2"][0, :, 6:] == field_cases.PATH_R ** 2 + 1).all() and (f["cost"][0, :, 6:] == 0).all()
    seen = {"blocked": 0, "clear": 0, "outside": 0, "unknown": 0, "border": 0}
    for name, c in PATHS.items():
        for outside_blocks in (True, False):
            for blocked_at in (253, 40):
                args = (c["xy"], c["n_poses"], c["path_map"], field_cases.PATH_ORIGIN, field_cases.PATH_CELL, state, f["dist2"], f["cost"],
                        field_cases.PATH_R, blocked_at, outside_blocks)
                got, want = field_ref.check_paths(*args), loop_paths(*args)
                assert set(got) == set(want)
                for k in want:
                    assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, outside_blocks, blocked_at, k)
                K, P = c["xy"].shape[:2]
                n = np.full(K, P) if c["n_poses"] is None else np.clip(c["n_poses"], 0, P)
                seen["blocked"] += int((got["first_blocked"] >= 0).sum())
                seen["clear"] += int(((got["first_blocked"] < 0) & (got["n_outside"] == 0) & (n > 0)).sum())
                seen["outside"] += int(((got["n_outside"] == n) & (n > 0)).sum())
                seen["unknown"] += int(got["n_unknown"].sum())
        seen["border"] += int((c["xy"] / field_cases.PATH_CELL == np.round(c["xy"] / field_cases.PATH_CELL)).sum())
    assert all(v > 0 for v in seen.values()), seen
    assert sorted(c["xy"].shape[1] for c in PATHS.values()) == [1, 63, 64, 65, 130] and sorted(c["xy"].shape[0] for c in PATHS.values()) == [1, 2, 3, 4, 5]
    assert (field_cases.PATH_ORIGIN < 0).any() and any((c["xy"] < 0).any() for c in PATHS.values())
    assert any(np.isnan(c["xy"]).any() for c in PATHS.values()) and any(np.isinf(c["xy"]).any() for c in PATHS.values())
    assert any(c["path_map"] is not None and (c["path_map"] >= state.shape[0]).any() for c in PATHS.values())


def test_the_workspace_formula():
    assert [field_ref.workspace_bytes(*s) for s in ((1, 1, 1), (1, 1, 5), (3, 40, 36), (2, 13, 17))] == [16, 32, 17280, 1776]
