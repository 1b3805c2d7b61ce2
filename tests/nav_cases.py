"""The named cases of the navigation field for tests/test_nav_ref_cpu.py (the restatement against Dijkstra) and tests/test_gpu_nav.py
(the kernels against the restatement): the smallest shapes at which the kernels can go wrong.  The sweep holds 1, 2, 4 or 8 columns per
lane for rows of up to 64, 128, 256 and 512 cells and takes a longer row in chunks of 512, so there is a case on each side of every
switch and rows of two and three chunks.

A case holds 'cost' (uint8 [M,nx,ny]), 'goals' (fp64 [M,G,2], metres), 'n_goals' (int32 [M] or None), 'origin' (int64 [M,2]), 'cell',
'neutral', 'blocked_at', 'starts' (fp64 [K,2]), 'path_map' (int32 [K] or None), 'P', and 'kind': 'mixed' (at least 10 % of the cells
reached and at least 10 % not), 'reached' (every passable cell reached, at least one), 'none' (no cell reached) or 'plain'.  'rounds':
the rounds the restatement's order needs, where the case is about them.  all_cases() asserts every case's own precondition."""
import numpy as np

from tests import field_cases, field_ref

UNREACHED = 0x7FFFFFFF
KINDS = ("mixed", "reached", "none", "plain")
WALL = 254


def costmap(state, R, cell=0.5, unknown_cost=0, **table):
    clear, cost = field_ref.tables(cell, R, **table)
    return field_ref.distance_field(state, 1 << field_cases.OCCUPIED, R, unknown_cost, clear, cost)["cost"]


def centre(origin, cell, i, j):
    """The centre of window cell (i, j) in metres."""
    return ((origin[0] + i + 0.5) * cell, (origin[1] + j + 0.5) * cell)


def passable_near(cost_m, blocked_at, i, j):
    """The passable cell nearest to (i, j), the lowest index among equal ones."""
    ii, jj = np.nonzero(cost_m < blocked_at)
    assert ii.size, "the map has no passable cell"
    k = int(np.argmin((ii - i) ** 2 + (jj - j) ** 2))
    return int(ii[k]), int(jj[k])


def starts_of(cost, origin, cell, blocked_at, extra=()):
    """Per map the passable cells nearest to its corners, its centre and the middle of its last row, a little off their centres; a
    start on a wall if there is one; then one outside every window, one NaN, one on map M (no such map) and `extra`."""
    M, nx, ny = cost.shape
    starts, maps = [], []
    for m in range(M):
        spots = ((0, 0), (0, ny - 1), (nx - 1, 0), (nx - 1, ny - 1), (nx // 2, ny // 2), (nx - 1, ny // 2))
        for q, (i, j) in enumerate(spots if (cost[m] < blocked_at).any() else ()):
            i, j = passable_near(cost[m], blocked_at, i, j)
            x, y = centre(origin[m], cell, i, j)
            starts.append((x + 0.01 * cell * q, y - 0.02 * cell * q))
            maps.append(m)
        walls = np.argwhere(cost[m] >= blocked_at)
        if len(walls):
            starts.append(centre(origin[m], cell, *walls[len(walls) // 2]))
            maps.append(m)
    x0, y0 = centre(origin[0], cell, 0, 0)
    starts += [(x0 - 3 * cell, y0), (np.nan, y0), (x0, y0)] + list(extra)
    maps += [0, 0, M] + [0] * len(extra)
    return np.array(starts, np.float64), np.array(maps, np.int32)


def case(cost, goal_cells, kind, origin=None, cell=0.5, neutral=50, blocked_at=253, n_goals=None, goals=None, P=96, rounds=None, extra_starts=()):
    """goal_cells: per map a list of (i, j), turned into the cells' centres; goals: the points themselves instead."""
    assert kind in KINDS and cost.dtype == np.uint8 and cost.ndim == 3
    M = cost.shape[0]
    origin = np.zeros((M, 2), np.int64) if origin is None else np.asarray(origin, np.int64)
    if goals is None:
        goals = np.array([[centre(origin[m], cell, i, j) for i, j in goal_cells[m]] for m in range(M)], np.float64)
    goals = np.asarray(goals, np.float64).reshape(M, -1, 2)
    starts, path_map = starts_of(cost, origin, cell, blocked_at, extra_starts)
    return dict(cost=cost, goals=goals, n_goals=None if n_goals is None else np.asarray(n_goals, np.int32), origin=origin, cell=cell,
                neutral=neutral, blocked_at=blocked_at, kind=kind, starts=starts, path_map=path_map, P=P, rounds=rounds)


def raw(shape, walls=(), fill=0):
    cost = np.full(shape, fill, np.uint8)
    for c in walls:
        cost[c] = WALL
    return cost


def scattered(seed, shape, share=0.01, R=4, **table):
    return costmap(field_cases.scatter(seed, shape, share), R, **dict(dict(inscribed=0.5, scale=1.0), **table))


def with_goal_near(cost, i, j, kind="plain", blocked_at=253, **kw):
    """A case with one goal per map on the passable cell nearest to (i, j)."""
    return case(cost, [[passable_near(c, blocked_at, i, j)] for c in cost], kind, blocked_at=blocked_at, **kw)


def u_wall():
    st = np.full((40, 36), field_cases.FREE, np.uint8)
    st[10:25, 8] = st[10:25, 28] = field_cases.OCCUPIED
    st[24, 8:29] = field_cases.OCCUPIED
    return costmap(st[None], 3, inscribed=0.5, scale=1.0)


def serpentine():
    """33 x 65: walls on every 4th column, 16 of them, open alternately at row 0 and at row 32, the goal at (0, 0)."""
    cost = np.zeros((33, 65), np.uint8)
    for q, j in enumerate(range(3, 65, 4)):
        cost[:, j] = WALL
        cost[0 if q % 2 == 0 else 32, j] = 0
    return cost[None]


def all_cases():
    rs = np.random.RandomState(77)
    origin2 = field_cases.PATH_ORIGIN
    two = scattered(1, (2, 13, 17), 0.05, R=3, scale=2.0)
    two_goals = [[passable_near(two[m], 253, 2, 3), passable_near(two[m], 253, 10, 14)] for m in range(2)]
    border = raw((1, 12, 10), [(0, 5, j) for j in range(0, 7)])
    walled = raw((1, 9, 9), [(0, 4, 4)])
    cases = {
        "1 x 1, the goal on it": case(raw((1, 1, 1)), [[(0, 0)]], "reached"),
        "1 x 1, impassable": case(raw((1, 1, 1), [(0, 0, 0)]), [[(0, 0)]], "none"),
        "1 x 70, a wall cell": case(raw((1, 1, 70), [(0, 0, 40)]), [[(0, 3)]], "mixed"),
        "70 x 1, a wall cell": case(raw((1, 70, 1), [(0, 9, 0)]), [[(30, 0)]], "mixed", origin=[[-3, 1000]]),
        "two maps of 13 x 17, n_goals 2 and 1": case(two, two_goals, "plain", origin=origin2, n_goals=[2, 1]),
        "33 x 63": with_goal_near(scattered(2, (1, 33, 63)), 5, 60),
        "33 x 64": with_goal_near(scattered(3, (1, 33, 64)), 30, 63),
        "33 x 65": with_goal_near(scattered(4, (1, 33, 65)), 16, 64),
        "5 x 128": with_goal_near(scattered(14, (1, 5, 128), 0.02, R=2), 2, 127),
        "9 x 129": with_goal_near(scattered(5, (1, 9, 129), 0.02, R=2), 4, 128, cell=0.2, P=160),
        "3 x 256": with_goal_near(scattered(15, (1, 3, 256), 0.01, R=2), 1, 255, P=40),
        "3 x 257": with_goal_near(scattered(16, (1, 3, 257), 0.01, R=2), 1, 256, P=40),
        "3 x 512": with_goal_near(scattered(17, (1, 3, 512), 0.005, R=2), 1, 300, P=40),
        "3 x 513": with_goal_near(scattered(18, (1, 3, 513), 0.005, R=2), 1, 512, P=40),
        "3 x 600, two chunks": with_goal_near(scattered(9, (1, 3, 600), 0.005, R=2), 1, 511, P=40),
        "5 x 1100, three chunks": with_goal_near(scattered(10, (1, 5, 1100), 0.003, R=2), 2, 1030, P=96),
        "40 x 36, a U wall open upward": case(u_wall(), [[(18, 18)]], "reached", rounds=3),
        "33 x 65, a serpentine of column walls": case(serpentine(), [[(0, 0)]], "reached", rounds=9, P=700),
        "65 x 33, a serpentine of row walls": case(np.ascontiguousarray(serpentine().transpose(0, 2, 1)), [[(0, 0)]], "reached", rounds=2, P=700),
        "33 x 64, random costs, neutral 1": with_goal_near(rs.randint(0, 256, (1, 33, 64)).astype(np.uint8), 16, 32, neutral=1),
        "9 x 130, all 252, neutral 255": case(raw((1, 9, 130), fill=252), [[(4, 0)]], "reached", neutral=255, P=140),
        "blocked_at 100": with_goal_near(scattered(6, (1, 20, 30), 0.03, R=3, scale=0.5), 10, 15, blocked_at=100),
        # a NaN, a point beyond the window and the centre of the wall cell (4, 4)
        "only goals that are skipped": case(walled, None, "none", goals=[[(np.nan, 1.0), (-3.0, 2.0), (2.25, 2.25), (1.0, np.inf)]]),
        # X on the border between the rows 7 and 8 of the window and Y on that between the columns 2 and 3: the cell is (8, 3)
        "a goal on a cell border": case(border, None, "reached", origin=[[-7, 3]], goals=[[((-7 + 8) * 0.5, (3 + 3) * 0.5)]],
                                        extra_starts=[((-7 + 2) * 0.5, (3 + 9) * 0.5)]),
    }
    for name, c in cases.items():
        check(name, c)
    return cases


def check(name, c):
    """The precondition of case `name`, from its own data and tests/nav_ref.py's cell rule alone."""
    from tests import nav_ref
    M, nx, ny = c["cost"].shape
    assert nx * ny <= 1 << 19 and c["goals"].shape[0] == M and c["origin"].shape == (M, 2) and c["starts"].shape[1] == 2, name
    G = c["goals"].shape[1]
    passable = c["cost"] < c["blocked_at"]
    n_used = 0
    for m in range(M):
        n = G if c["n_goals"] is None else int(np.clip(c["n_goals"][m], 0, G))
        cells = nav_ref.window_cells(c["goals"][m, :n], c["origin"][m], c["cell"], nx, ny)
        n_used += int(sum(cl >= 0 and passable[m].reshape(-1)[cl] for cl in cells))
    if c["kind"] == "none":
        assert n_used == 0, name
    else:
        assert n_used >= 1, f"{name}: no goal on a passable cell"


def check_kind(name, c, togo):
    """What the case claims of its result (called with the restatement's togo)."""
    reached = togo != UNREACHED
    passable = c["cost"] < c["blocked_at"]
    share = reached.mean()
    if c["kind"] == "mixed":
        assert 0.1 <= share <= 0.9, (name, share)
    elif c["kind"] == "reached":
        assert reached.any() and np.array_equal(reached, passable), name
    elif c["kind"] == "none":
        assert not reached.any(), name
