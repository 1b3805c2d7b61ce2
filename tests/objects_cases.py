"""The named cases of the map objects for tests/test_objects_ref_cpu.py (the restatement against scipy) and tests/test_gpu_objects.py
(the kernels against the restatement): the smallest shapes at which the kernels can go wrong.

The kernels label tiles of TILE_H = 16 rows x TILE_W = 64 columns and join them along their borders, so the large cases are 130 x 197
(nine tiles down, four across), 96 x 130 (six by three) and 48 x 130 (three by three); 33 x 65 has a last tile of one row and one of
one column.  A case holds 'state' (uint8 [M,nx,ny]), 'origin' (int64 [M,2]), 'cell', 'sources' (the mask), 'connectivity',
'min_cells', 'max_objects' and, where the content fixes it, 'kept': the kept objects of each map."""
import numpy as np

from tests import objects_ref

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
TILE_H, TILE_W = 16, 64


def states(src):
    """bool [..] -> uint8: OCCUPIED where set, FREE and UNKNOWN in stripes elsewhere."""
    src = np.asarray(src, bool)
    rest = (np.indices(src.shape).sum(0) % 3 == 0).astype(np.uint8)
    out = np.where(src, np.uint8(OCCUPIED), rest).astype(np.uint8)
    return out[None] if out.ndim == 2 else out


def random_map(seed, shape, density):
    return np.random.RandomState(seed).rand(*shape) < density


def spiral(nx, ny):
    """One chain of cells, one cell wide, from (0, 0) inwards with one empty cell between its arms."""
    s = np.zeros((nx, ny), bool)
    i = j = d = 0
    s[0, 0] = True
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(a, b):
        return not (0 <= a < nx and 0 <= b < ny) or not s[a, b]

    def can(d):
        di, dj = steps[d]
        a, b = i + di, j + dj
        return 0 <= a < nx and 0 <= b < ny and not s[a, b] and free(a + di, b + dj)

    while True:
        if not can(d):
            d = (d + 1) % 4
            if not can(d):
                return s
        i, j = i + steps[d][0], j + steps[d][1]
        s[i, j] = True


def serpentine(nx, ny):
    """Walls on every second row, joined at alternating ends: one object that a raster scan meets as nx / 2 separate ones."""
    s = np.zeros((nx, ny), bool)
    s[0::2] = True
    s[1::4, ny - 1] = True
    s[3::4, 0] = True
    return s


def comb(nx, ny, down):
    """Teeth on every second column that join only in the last row (down) or in the first (up): the raster-scan equivalence case."""
    s = np.zeros((nx, ny), bool)
    s[:, 0::2] = True
    s[0 if down else nx - 1, :] = False
    s[nx - 1 if down else 0, :] = True
    return s


def corner_blobs():
    """Pairs of 3 x 3 blobs that touch only at a corner: inside a tile, across a horizontal tile border, across a vertical one, and twice
    exactly where four tiles meet, once along each diagonal.  Ten objects with 4-connectivity, five with 8."""
    s = np.zeros((48, 130), bool)
    for (i, j), (a, b) in (((2, 5), (5, 8)),                            # inside tile (0, 0): cells (4, 7) and (5, 8)
                           ((13, 20), (16, 23)),                        # rows 15 | 16
                           ((20, 61), (23, 64)),                        # columns 63 | 64
                           ((13, 61), (16, 64)),                        # (15, 63) and (16, 64): four tiles meet
                           ((29, 64), (32, 61))):                       # (31, 64) and (32, 63): the other diagonal
        s[i:i + 3, j:j + 3] = True
        s[a:a + 3, b:b + 3] = True
    return s


def sizes_2_3_4():
    s = np.zeros((20, 70), bool)
    s[1, 1:3] = True                                                    # 2 cells
    s[5:8, 66] = True                                                   # 3 cells, in the second tile column
    s[15:17, 10:12] = True                                              # 4 cells, rows 15 | 16
    s[18, 63:65] = True                                                 # 2 cells, columns 63 | 64
    return s


def kept_count(src, connectivity, min_cells=1):
    root = objects_ref.first_cells(np.asarray(src, bool), connectivity)
    _, cells = np.unique(root[root >= 0], return_counts=True)
    return int((cells >= min_cells).sum())


def case(state, connectivity, origin=None, cell=0.5, sources=1 << OCCUPIED, min_cells=1, max_objects=256, kept=None):
    assert state.dtype == np.uint8 and state.ndim == 3
    origin = np.zeros((state.shape[0], 2), np.int64) if origin is None else np.asarray(origin, np.int64)
    return dict(state=state, origin=origin, cell=cell, sources=sources, connectivity=connectivity, min_cells=min_cells,
                max_objects=max_objects, kept=kept)


def all_cases():
    cases = {}
    checker = np.add.outer(np.arange(130), np.arange(197)) % 2 == 0
    dense = random_map(5, (96, 130), 0.3)
    three = np.stack([random_map(21, (40, 70), 0.2), np.zeros((40, 70), bool), serpentine(40, 70)])
    digits = (np.arange(33 * 65) % 10).astype(np.uint8).reshape(1, 33, 65)
    digits[0, 10:14, 20:30] = 200
    line = np.zeros(70, bool)
    line[[0, 1, 2, 40, 63, 64, 69]] = True
    for conn in (4, 8):
        def add(name, state, **kw):
            cases[f"{name}, {conn}-connected"] = case(state, conn, **kw)

        add("20 x 70, empty", states(np.zeros((20, 70), bool)), kept=[0])
        add("33 x 65, full", states(np.ones((33, 65), bool)), kept=[1], origin=[[5, -9]])
        add("1 x 1, a source", states(np.ones((1, 1), bool)), kept=[1])
        add("1 x 1, no source", states(np.zeros((1, 1), bool)), kept=[0])
        add("1 x 70", states(line[None, :]), kept=[4])
        add("70 x 1", states(line[:, None]), kept=[4], origin=[[-100, 3]])
        add("33 x 65, random", states(random_map(1, (33, 65), 0.45)), origin=[[-40, 7]], cell=0.2)
        add("130 x 197, random", states(random_map(2, (130, 197), 0.45)), origin=[[1000, -2000]], max_objects=4096)
        add("130 x 197, a spiral", states(spiral(130, 197)), kept=[1])
        add("33 x 65, a serpentine of walls", states(serpentine(33, 65)), kept=[1])
        add("40 x 131, a comb of downward teeth", states(comb(40, 131, True)), kept=[1])
        add("40 x 131, a comb of upward teeth", states(comb(40, 131, False)), kept=[1])
        add("48 x 130, blobs that touch at a corner", states(corner_blobs()), kept=[10 if conn == 4 else 5])
        add("130 x 197, a checkerboard", states(checker), kept=[int(checker.sum()) if conn == 4 else 1])           # 4: the overflow case
        add("96 x 130, density 0.41", states(random_map(3, (96, 130), 0.41)), max_objects=2048)
        add("96 x 130, density 0.59", states(random_map(4, (96, 130), 0.59)), max_objects=2048, origin=[[-3, -4]])
        add("20 x 70, min_cells 3 over objects of 2, 3, 4 and 2 cells", states(sizes_2_3_4()), min_cells=3, kept=[2])
        add("96 x 130, max_objects 1", states(dense), max_objects=1)
        n = kept_count(dense, conn, 2)
        add("96 x 130, max_objects the kept objects", states(dense), min_cells=2, max_objects=n, kept=[n])
        add("96 x 130, max_objects one fewer", states(dense), min_cells=2, max_objects=n - 1, kept=[n])
        add("three maps of 40 x 70", states(three), origin=[[-7, 3], [100, -50], [-(1 << 40), (1 << 40) + 1]], max_objects=300, cell=0.25)
        add("33 x 65, states 0 .. 9 and 200, sources 2 and 5", digits, sources=(1 << 2) | (1 << 5), max_objects=500)
    return cases
