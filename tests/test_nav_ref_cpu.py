"""CPU: tests/nav_ref.py, the NumPy restatement of crd_nav_field and crd_nav_paths that the GPU tests compare the kernels with, held to
independent algorithms on every case of tests/nav_cases.py: a plain heapq Dijkstra, scipy's Dijkstra on a graph built edge by edge
(integers below 2^53, so exact in its doubles), and the properties a planned path must have."""
import heapq

import numpy as np
import pytest

from tests import nav_cases, nav_ref

CASES = nav_cases.all_cases()
UNREACHED = nav_ref.UNREACHED
_REF, _TRUE = {}, {}


def ref_of(name):
    if name not in _REF:
        c = CASES[name]
        _REF[name] = nav_ref.nav_field(c["cost"], c["goals"], c["n_goals"], c["origin"], c["cell"], c["neutral"], c["blocked_at"], 64)
    return _REF[name]


def goal_cells(c, m):
    M, nx, ny = c["cost"].shape
    G = c["goals"].shape[1]
    n = G if c["n_goals"] is None else int(np.clip(c["n_goals"][m], 0, G))
    out = []
    for X, Y in c["goals"][m, :n]:                                     # the header's rule, written out once more
        if not (np.isfinite(X) and np.isfinite(Y)):
            continue
        wx, wy = np.floor(X / c["cell"]), np.floor(Y / c["cell"])
        i, j = int(wx) - int(c["origin"][m, 0]), int(wy) - int(c["origin"][m, 1])
        if 0 <= i < nx and 0 <= j < ny and c["cost"][m, i, j] < c["blocked_at"]:
            out.append((i, j))
    return out


def dijkstra(c, m):
    """togo of map m by a heap: the least sum of k * w(a) over the cells a left on the way to a goal."""
    cost = c["cost"][m].astype(np.int64)
    nx, ny = cost.shape
    dist = np.full((nx, ny), UNREACHED, np.int64)
    heap = []
    for g in goal_cells(c, m):
        dist[g] = 0
        heap.append((0, g))
    heapq.heapify(heap)
    while heap:
        d, (i, j) = heapq.heappop(heap)
        if d > dist[i, j]:
            continue
        for (di, dj), k in zip(nav_ref.NEIGHBOURS, nav_ref.WEIGHTS):
            a, b = i + di, j + dj                                      # the cell that would step to (i, j)
            if 0 <= a < nx and 0 <= b < ny and cost[a, b] < c["blocked_at"]:
                v = d + k * (c["neutral"] + cost[a, b])
                if v < dist[a, b]:
                    dist[a, b] = v
                    heapq.heappush(heap, (v, (a, b)))
    return dist


def true_of(name):
    if name not in _TRUE:
        c = CASES[name]
        _TRUE[name] = np.stack([dijkstra(c, m) for m in range(c["cost"].shape[0])]).astype(np.int32)
    return _TRUE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_togo_is_heap_dijkstra(name):
    c, got = CASES[name], ref_of(name)
    assert got["togo"].dtype == np.int32 and got["next"].dtype == np.uint8 and got["info"].dtype == np.int32
    assert np.array_equal(got["togo"], true_of(name))
    nav_cases.check_kind(name, c, got["togo"])
    M = c["cost"].shape[0]
    G = c["goals"].shape[1]
    for m in range(M):
        n = G if c["n_goals"] is None else int(np.clip(c["n_goals"][m], 0, G))
        used = len(goal_cells(c, m))
        assert got["info"][m].tolist()[2:] == [used, n - used] and got["info"][m, 0] == 1 and 1 <= got["info"][m, 1] <= 64
    if c["rounds"] is not None:
        assert got["info"][0, 1] == c["rounds"]
    assert np.array_equal(got["togo"] == UNREACHED, got["next"] == nav_ref.NO_STEP)
    assert np.array_equal(got["togo"] == 0, got["next"] == nav_ref.ON_GOAL)
    assert (got["togo"][c["cost"] >= c["blocked_at"]] == UNREACHED).all()


def test_particular_cases():
    got = ref_of("9 x 130, all 252, neutral 255")["togo"]
    assert got.max() == 331071 and got[0, 4, 0] == 0                    # the largest steps there are: 4 * 7 * 507 + 125 * 5 * 507
    got = ref_of("a goal on a cell border")["togo"]
    assert (got == 0).sum() == 1 and got[0, 8, 3] == 0
    got = ref_of("only goals that are skipped")
    assert got["info"].tolist() == [[1, 1, 0, 4]]
    got = ref_of("two maps of 13 x 17, n_goals 2 and 1")
    assert got["info"][:, 2:].tolist() == [[2, 0], [1, 0]] and [(t == 0).sum() for t in got["togo"]] == [2, 1]
    assert ref_of("1 x 1, the goal on it")["togo"].tolist() == [[[0]]] and ref_of("1 x 1, impassable")["togo"].tolist() == [[[UNREACHED]]]


@pytest.mark.parametrize("name", list(CASES))
def test_togo_is_scipys_dijkstra(name):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse import csgraph
    c, got = CASES[name], ref_of(name)
    M, nx, ny = c["cost"].shape
    for m in range(M):
        goals = [i * ny + j for i, j in goal_cells(c, m)]
        if not goals:
            assert (got["togo"][m] == UNREACHED).all()
            continue
        passable = c["cost"][m] < c["blocked_at"]
        w = c["neutral"] + c["cost"][m].astype(np.int64)
        rows, cols, vals = [], [], []
        for i in range(nx):                                             # the edge b -> a for every move a -> b, with the move's cost
            for j in range(ny):
                if not passable[i, j]:
                    continue
                for (di, dj), k in zip(nav_ref.NEIGHBOURS, nav_ref.WEIGHTS):
                    i2, j2 = i + di, j + dj
                    if 0 <= i2 < nx and 0 <= j2 < ny and passable[i2, j2]:
                        rows.append(i2 * ny + j2), cols.append(i * ny + j), vals.append(k * w[i, j])
        graph = sparse.csr_matrix((np.array(vals, np.float64), (rows, cols)), shape=(nx * ny, nx * ny))
        dist = csgraph.dijkstra(graph, directed=True, indices=goals, min_only=True)
        want = np.where(np.isfinite(dist), dist, UNREACHED).astype(np.int64).reshape(nx, ny)
        assert max(vals, default=0) * nx * ny < 2 ** 53 and np.array_equal(got["togo"][m], want)


def test_planned_paths():
    seen = set()
    for name, c in CASES.items():
        got = ref_of(name)
        M, nx, ny = c["cost"].shape
        p = nav_ref.plan_paths(c["starts"], c["path_map"], c["origin"], c["cell"], got["togo"], got["next"], c["P"])
        K, P = len(c["starts"]), c["P"]
        assert p["cells"].shape == (K, P) and p["xy"].shape == (K, P, 2)
        for k in range(K):
            st, n, m = int(p["status"][k]), int(p["n_cells"][k]), int(c["path_map"][k])
            seen.add(st)
            assert (p["cells"][k, n:] == -1).all() and np.isnan(p["xy"][k, n:]).all() and (p["cells"][k, :n] >= 0).all()
            if st in (2, 3):
                assert n == 0 and (p["start_togo"][k] == UNREACHED)
                continue
            cells = p["cells"][k, :n].astype(np.int64)
            i, j = cells // ny, cells % ny
            togo, cost = got["togo"][m].astype(np.int64), c["cost"][m].astype(np.int64)
            assert (cost[i, j] < c["blocked_at"]).all() and p["start_togo"][k] == togo[i[0], j[0]]
            di, dj = np.diff(i), np.diff(j)
            assert ((np.abs(di) <= 1) & (np.abs(dj) <= 1) & ((di != 0) | (dj != 0))).all()
            assert (np.diff(togo[i, j]) < 0).all()
            steps = np.where((di != 0) & (dj != 0), 7, 5) * (c["neutral"] + cost[i[:-1], j[:-1]])
            assert np.array_equal(p["xy"][k, :n, 0], (c["origin"][m, 0] + i + 0.5) * c["cell"])
            assert np.array_equal(p["xy"][k, :n, 1], (c["origin"][m, 1] + j + 0.5) * c["cell"])
            if st == 0:
                assert togo[i[-1], j[-1]] == 0 and steps.sum() == p["start_togo"][k]
            else:
                assert st == 1 and n == P and steps.sum() == p["start_togo"][k] - togo[i[-1], j[-1]]
    assert seen == {0, 1, 2, 3}


def test_one_round_of_the_serpentine_is_an_upper_bound():
    name = "33 x 65, a serpentine of column walls"
    c = CASES[name]
    got = nav_ref.nav_field(c["cost"], c["goals"], c["n_goals"], c["origin"], c["cell"], c["neutral"], c["blocked_at"], max_rounds=1)
    true = true_of(name)
    assert got["info"][0, :2].tolist() == [0, 1]
    assert (got["togo"] >= true).all() and (got["togo"] > true).any() and (got["togo"] == UNREACHED).sum() > (true == UNREACHED).sum()
    # every value is the cost of a real path: following next from any reached cell strictly falls and ends on the goal
    M, nx, ny = c["cost"].shape
    i, j = np.nonzero(got["togo"][0] != UNREACHED)
    starts = np.stack([(i + 0.5) * c["cell"], (j + 0.5) * c["cell"]], -1)
    p = nav_ref.plan_paths(starts, None, c["origin"], c["cell"], got["togo"], got["next"], nx * ny)
    assert (p["status"] == 0).all()
    for k in range(len(starts)):
        cells = p["cells"][k, :p["n_cells"][k]]
        assert (np.diff(got["togo"][0].reshape(-1)[cells].astype(np.int64)) <= -5).all()
