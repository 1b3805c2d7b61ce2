"""NumPy restatement of crd_map_objects (include/camradepth_hip.h): the connected sets of source cells of a state map, numbered in the
order of their first cells, as a label per cell and a table.  A raster scan with a union-find that hangs the larger root under the
smaller, so a root is its object's first cell; everything else is counting.  tests/test_objects_ref_cpu.py holds it to scipy."""
import numpy as np

BACKGROUND, SMALL, OVERFLOW = -1, -2, -3
UNUSED_ROW = (-1, 0, -1, -1, -1, -1, 0, 0)


def source_mask(state, sources):
    """state: uint8 [..]; sources: the bit mask 1 .. 255 -> bool: state < 8 and bit `state` of sources set."""
    state = np.asarray(state)
    return (state < 8) & (((int(sources) >> np.minimum(state, 7).astype(np.int64)) & 1) == 1)


def first_cells(src, connectivity):
    """src: bool [nx][ny] -> int64 [nx][ny]: the first cell (lowest i * ny + j) of every source cell's object, -1 on the others."""
    nx, ny = src.shape
    parent = list(range(nx * ny))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    before = ((0, -1), (-1, -1), (-1, 0), (-1, 1)) if connectivity == 8 else ((0, -1), (-1, 0))
    s = src.tolist()
    for i in range(nx):
        for j in range(ny):
            if not s[i][j]:
                continue
            for di, dj in before:
                a, b = i + di, j + dj
                if a < 0 or b < 0 or b >= ny or not s[a][b]:
                    continue
                p, q = find(i * ny + j), find(a * ny + b)
                if p != q:
                    parent[max(p, q)] = min(p, q)
    root = np.full(nx * ny, -1, np.int64)
    for c in np.flatnonzero(src.reshape(-1)).tolist():
        root[c] = find(c)
    return root.reshape(nx, ny)


def map_objects(state, sources, connectivity, min_cells, max_objects, origin, cell):
    """state: uint8 [M][nx][ny]; origin: int64 [M][2]; cell: float -> dict of label, objects, sums, centre, info as the header gives them."""
    state = np.asarray(state, np.uint8)
    M, nx, ny = state.shape
    N = int(max_objects)
    src = source_mask(state, sources)
    label = np.full((M, nx, ny), BACKGROUND, np.int32)
    objects = np.tile(np.array(UNUSED_ROW, np.int32), (M, N, 1))
    sums = np.zeros((M, N, 2), np.int64)
    centre = np.full((M, N, 2), np.nan, np.float64)
    info = np.zeros((M, 4), np.int32)
    cell = np.float64(cell)
    for m in range(M):
        root = first_cells(src[m], connectivity)
        firsts, cells = np.unique(root[root >= 0], return_counts=True)           # ascending: the objects' order
        number = 0
        for first, n_cells in zip(firsts.tolist(), cells.tolist()):
            ii, jj = np.nonzero(root == first)
            if n_cells < min_cells:
                label[m, ii, jj] = SMALL
                info[m, 2] += 1
                continue
            k, number = number, number + 1
            if k >= N:
                label[m, ii, jj] = OVERFLOW
                info[m, 1] += 1
                continue
            label[m, ii, jj] = k
            edge = ii.min() == 0 or ii.max() == nx - 1 or jj.min() == 0 or jj.max() == ny - 1
            objects[m, k] = (first, n_cells, ii.min(), ii.max(), jj.min(), jj.max(), 1 if edge else 0, 0)
            sums[m, k] = (ii.sum(dtype=np.int64), jj.sum(dtype=np.int64))
            for q in range(2):
                mean = np.float64(sums[m, k, q]) / np.float64(n_cells)
                centre[m, k, q] = ((np.float64(origin[m][q]) + mean) + np.float64(0.5)) * cell
            info[m, 0] += 1
    return {"label": label, "objects": objects, "sums": sums, "centre": centre, "info": info}
