"""The named cases of the distance field for tests/test_field_ref_cpu.py (the restatement against brute force) and
tests/test_gpu_field.py (the kernels against the restatement): the smallest shapes at which the kernels can go wrong.

A field case holds 'state' (uint8 [M,nx,ny]), 'R', 'sources' (the mask), 'unknown_cost', 'cell', the 'table' options of
field.tables, and 'kind': 'mixed' (at least 10 % of the cells FAR and at least 10 % not), 'covered' (R reaches over the whole window),
'uniform' (an empty or a full map), 'ties' (some cell has two or more nearest sources) or 'plain' (nothing is asked of it)."""
import numpy as np

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
KINDS = ("mixed", "covered", "uniform", "ties", "plain")


def scatter(seed, shape, share, rows=None):
    """A map of FREE and UNKNOWN cells with OCCUPIED ones on about `share` of them, drawn in the rows [0, rows) only if given."""
    rs = np.random.RandomState(seed)
    state = rs.randint(0, 2, size=shape).astype(np.uint8)
    hit = rs.rand(*shape) < share
    if rows is not None:
        hit[:, rows:] = False
    state[hit] = OCCUPIED
    return state


def placed(shape, cells, fill=FREE):
    state = np.full(shape, fill, np.uint8)
    for c in cells:
        state[c] = OCCUPIED
    return state


def case(state, R, kind, sources=1 << OCCUPIED, unknown_cost=0, cell=0.5, **table):
    assert kind in KINDS and state.dtype == np.uint8 and state.ndim == 3
    return dict(state=state, R=R, kind=kind, sources=sources, unknown_cost=unknown_cost, cell=cell, table=table)


def all_cases():
    checker = np.where(np.add.outer(np.arange(12), np.arange(13)) % 2 == 0, OCCUPIED, FREE).astype(np.uint8)[None]
    digits = (np.arange(10 * 12) % 10).astype(np.uint8).reshape(1, 10, 12)
    return {
        "1 x 1, a source": case(placed((1, 1, 1), [(0, 0, 0)]), 1, "uniform"),
        "1 x 1, no source": case(placed((1, 1, 1), []), 1, "uniform"),
        "a single row of 70": case(placed((1, 1, 70), [(0, 0, 3), (0, 0, 40), (0, 0, 41)]), 5, "mixed"),
        "a single column of 70": case(placed((1, 70, 1), [(0, 8, 0), (0, 9, 0), (0, 66, 0)], fill=UNKNOWN), 5, "mixed", unknown_cost=40),
        "two maps of 13 x 17": case(scatter(1, (2, 13, 17), 0.05), 3, "mixed", inscribed=0.5, scale=2.0),
        "33 x 63": case(scatter(2, (1, 33, 63), 0.01), 8, "mixed"),
        "33 x 64": case(scatter(3, (1, 33, 64), 0.01), 8, "mixed", inscribed=1.0, inflation=3.0, scale=1.0),
        "33 x 65": case(scatter(4, (1, 33, 65), 0.01), 8, "mixed"),
        "9 x 129": case(scatter(5, (1, 9, 129), 0.01), 8, "mixed", cell=0.2),
        "three maps of 40 x 36, R 64": case(scatter(6, (3, 40, 36), 0.003), 64, "covered", scale=0.2),
        "9 x 130, R 200": case(scatter(7, (1, 9, 130), 0.004), 200, "covered", cell=0.1, scale=0.5),
        # about 0.3 % sources, drawn in the upper 60 rows, so that the rows below them are out of reach; the tiles of launch 2 end at rows
        # 32, 64, 96 and 128 here, and most cells have their nearest source in another tile
        "150 x 70, R 40": case(scatter(8, (1, 150, 70), 0.0075, rows=60), 40, "mixed", scale=0.3),
        "300 x 66, R 255": case(placed((1, 300, 66), [(0, 0, 0), (0, 3, 30), (0, 10, 65)]), 255, "mixed", cell=0.2, scale=0.1),
        "20 x 20, empty": case(placed((1, 20, 20), [], fill=UNKNOWN), 4, "uniform", unknown_cost=200),
        "20 x 20, full": case(placed((1, 20, 20), [], fill=OCCUPIED), 4, "uniform"),
        "a checkerboard": case(checker, 3, "ties"),
        # map 0: two sources of one row, the left one wins; map 1: two of one column, the upper one wins; map 2: a diagonal pair
        "placed ties": case(placed((3, 9, 11), [(0, 1, 2), (0, 1, 6), (1, 3, 9), (1, 7, 9), (2, 5, 2), (2, 6, 3)]), 6, "ties"),
        "states 0 .. 9": case(digits, 3, "plain", sources=(1 << 2) | (1 << 5), unknown_cost=7),
    }


def tile_cases():
    """Maps with enough tiles of 64 columns for launch 2 to take higher tiles than the 8 rows of every case above: 16, 32 and 64 rows,
    which it does once 2048 tiles of that height are there (R 5).  Narrow maps, so that 2048 tiles are few cells."""
    return {
        "32768 x 5, tiles of 16 rows": case(scatter(11, (1, 32768, 5), 0.01), 5, "mixed", inscribed=0.5, scale=1.0),
        "two maps of 32768 x 5, tiles of 32 rows": case(scatter(12, (2, 32768, 5), 0.01), 5, "mixed", unknown_cost=9),
        "four maps of 32768 x 5, tiles of 64 rows": case(scatter(13, (4, 32768, 5), 0.01), 5, "mixed", cell=0.2),
    }


# ---- paths --------------------------------------------------------------------------------------------------------------------
# Two maps of 12 x 10 cells of 0.5 m, one with a negative origin.  The columns from 6 on of map 0 hold no source and lie beyond R = 3
# cells of every source: a path that stays there is clear.
PATH_R, PATH_CELL = 3, 0.5
PATH_ORIGIN = np.array([[-7, 3], [100, -50]], np.int64)


def path_map_state():
    state = scatter(21, (2, 12, 10), 0.08)
    state[0, :, 2:] = np.where(state[0, :, 2:] == OCCUPIED, FREE, state[0, :, 2:])          # map 0: sources in columns 0 and 1 only
    state[0, 4, 1] = OCCUPIED
    return state


def _poses(rs, K, P, m):
    """Poses around the window of map m: most inside, some beyond its edges, some exactly on cell borders."""
    ox, oy = PATH_ORIGIN[m]
    xy = np.stack([rs.uniform((ox - 2) * PATH_CELL, (ox + 14) * PATH_CELL, (K, P)), rs.uniform((oy - 2) * PATH_CELL, (oy + 12) * PATH_CELL, (K, P))], -1)
    on_border = rs.rand(K, P) < 0.3
    return np.where(on_border[..., None], np.round(xy / PATH_CELL) * PATH_CELL, xy)


def path_cases():
    """name -> dict(xy fp64 [K,P,2], n_poses int32 [K] or None, path_map int32 [K] or None)."""
    rs = np.random.RandomState(33)
    cases = {}
    cases["1 path of 1 pose"] = dict(xy=np.array([[[(-7 + 4) * PATH_CELL, (3 + 1) * PATH_CELL]]]), n_poses=None, path_map=None)     # on the source (4, 1)
    cases["2 paths of 63"] = dict(xy=_poses(rs, 2, 63, 0), n_poses=np.array([63, 17], np.int32), path_map=None)
    xy = _poses(rs, 3, 64, 1)
    xy[0, 5], xy[1, 0], xy[2, 63] = (np.nan, 1.0), (np.inf, -np.inf), (50.5, -np.inf)
    cases["3 paths of 64 on map 1"] = dict(xy=xy, n_poses=None, path_map=np.array([1, 1, 1], np.int32))
    xy = np.concatenate([_poses(rs, 2, 65, 0), _poses(rs, 2, 65, 1)])
    cases["4 paths of 65, both maps and map 7"] = dict(xy=xy, n_poses=np.array([65, 0, 64, 1], np.int32), path_map=np.array([0, 7, 1, 1], np.int32))
    xy = np.concatenate([_poses(rs, 3, 130, 0), _poses(rs, 2, 130, 1)])
    xy[0] = np.stack([rs.uniform(-3.5, 2.5, 130), rs.uniform(4.5, 6.5, 130)], -1)             # map 0, columns 6 .. 9: clear
    xy[1] = np.stack([rs.uniform(-80.0, -20.0, 130), rs.uniform(4.5, 6.5, 130)], -1)          # all beyond the window
    xy[2, 100:] = np.nan
    cases["5 paths of 130"] = dict(xy=xy, n_poses=np.array([130, 130, 130, 65, -3], np.int32), path_map=np.array([0, 0, 0, 1, -1], np.int32))
    return cases
