"""CPU: tests/objects_ref.py, the NumPy restatement of crd_map_objects, held to scipy on every case of tests/objects_cases.py --
ndimage.label with the two structures for the partition and its order, find_objects for the boxes, ndimage.sum for counts and sums, a
plain flood-fill loop for the numbering under min_cells and max_objects -- and the host build of the kernels' union-find body
(camradepth_amd/csrc/object_uf.h through tests/objects_uf_host.cpp) in natural and in shuffled order: the same partition."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from tests import objects_cases, objects_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = objects_cases.all_cases()
STRUCTURES = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}
_WANT = {}


def want_of(name):
    """The restatement's outputs of case `name`, computed once and left unchanged."""
    if name not in _WANT:
        c = CASES[name]
        _WANT[name] = objects_ref.map_objects(c["state"], c["sources"], c["connectivity"], c["min_cells"], c["max_objects"], c["origin"], c["cell"])
    return _WANT[name]


def flood_numbers(src, connectivity, min_cells, N):
    """label by a flood fill from every unlabelled source cell in index order: the header's definition, step by step."""
    nx, ny = src.shape
    label = np.full((nx, ny), -1, np.int64)
    seen = np.zeros((nx, ny), bool)
    number = small = 0
    for i0, j0 in zip(*np.nonzero(src)):
        if seen[i0, j0]:
            continue
        seen[i0, j0] = True
        cells, stack = [], [(int(i0), int(j0))]
        while stack:
            i, j = stack.pop()
            cells.append((i, j))
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (di, dj) == (0, 0) or (connectivity == 4 and di and dj):
                        continue
                    a, b = i + di, j + dj
                    if 0 <= a < nx and 0 <= b < ny and src[a, b] and not seen[a, b]:
                        seen[a, b] = True
                        stack.append((a, b))
        ii, jj = np.array(cells).T
        if len(cells) < min_cells:
            label[ii, jj], small = -2, small + 1
        else:
            label[ii, jj] = number if number < N else -3
            number += 1
    return label, number, small


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_agrees_with_scipy(name):
    c, got = CASES[name], want_of(name)
    M, nx, ny = c["state"].shape
    N, conn = c["max_objects"], c["connectivity"]
    src = objects_ref.source_mask(c["state"], c["sources"])
    assert got["label"].dtype == np.int32 and got["objects"].dtype == np.int32 and got["sums"].dtype == np.int64
    assert got["centre"].dtype == np.float64 and got["info"].dtype == np.int32
    assert got["objects"].shape == (M, N, 8) and got["sums"].shape == (M, N, 2) and got["centre"].shape == (M, N, 2) and got["info"].shape == (M, 4)
    for m in range(M):
        lab, n_all = ndimage.label(src[m], structure=STRUCTURES[conn])
        index = np.arange(1, n_all + 1)
        cells = ndimage.sum(src[m], lab, index).astype(np.int64) if n_all else np.zeros(0, np.int64)
        kept = index[cells >= c["min_cells"]]                                       # scipy's numbers of the kept objects, in order
        assert got["info"][m].tolist() == [min(len(kept), N), max(len(kept) - N, 0), n_all - len(kept), 0]
        if c["kept"] is not None:
            assert len(kept) == c["kept"][m]
        want_label = np.full((nx, ny), -1, np.int64)
        want_label[src[m]] = -2
        for k, s in enumerate(kept):
            want_label[lab == s] = k if k < N else -3
        assert np.array_equal(got["label"][m], want_label)
        flood, n_kept, n_small = flood_numbers(src[m], conn, c["min_cells"], N)
        assert np.array_equal(got["label"][m], flood) and (n_kept, n_small) == (len(kept), n_all - len(kept))
        boxes = ndimage.find_objects(lab)
        ii, jj = np.indices((nx, ny))
        rows = min(len(kept), N)
        for k in range(rows):
            s = kept[k]
            si, sj = boxes[s - 1]
            first = int(np.flatnonzero(lab.reshape(-1) == s)[0])
            edge = si.start == 0 or si.stop == nx or sj.start == 0 or sj.stop == ny
            assert got["objects"][m, k].tolist() == [first, cells[s - 1], si.start, si.stop - 1, sj.start, sj.stop - 1, int(edge), 0], (m, k)
            sums = [int(ndimage.sum(ii, lab, s)), int(ndimage.sum(jj, lab, s))]
            assert got["sums"][m, k].tolist() == sums
            ox, oy = (int(v) for v in c["origin"][m])
            exact = [(ox + sums[0] / cells[s - 1] + 0.5) * c["cell"], (oy + sums[1] / cells[s - 1] + 0.5) * c["cell"]]
            assert np.allclose(got["centre"][m, k], exact, rtol=1e-15, atol=0.0)
        assert (got["objects"][m, rows:] == np.array(objects_ref.UNUSED_ROW)).all() and not got["sums"][m, rows:].any()
        assert np.isnan(got["centre"][m, rows:]).all() and not np.isnan(got["centre"][m, :rows]).any()
        if rows:                                                                    # ordered by first cell
            assert (np.diff(got["objects"][m, :rows, 0]) > 0).all()


def test_the_cases_cover_what_they_are_meant_to():
    shapes = {c["state"].shape[1:] for c in CASES.values()}
    assert {(1, 1), (1, 70), (70, 1), (33, 65), (130, 197), (96, 130)} <= shapes
    assert any(nx >= 3 * objects_cases.TILE_H and ny > 3 * objects_cases.TILE_W for nx, ny in shapes)
    over = want_of("130 x 197, a checkerboard, 4-connected")["info"][0]
    assert over.tolist() == [256, 130 * 197 // 2 - 256, 0, 0]
    assert want_of("130 x 197, a checkerboard, 8-connected")["info"][0].tolist() == [1, 0, 0, 0]
    assert want_of("20 x 70, min_cells 3 over objects of 2, 3, 4 and 2 cells, 8-connected")["info"][0].tolist() == [2, 0, 2, 0]
    assert want_of("96 x 130, max_objects one fewer, 4-connected")["info"][0, 1] == 1
    assert want_of("96 x 130, max_objects the kept objects, 4-connected")["info"][0, 1] == 0
    assert want_of("96 x 130, max_objects 1, 8-connected")["info"][0, 0] == 1
    three = CASES["three maps of 40 x 70, 8-connected"]
    assert (three["origin"] < 0).any() and len({want_of("three maps of 40 x 70, 8-connected")["info"][m, 0] for m in range(3)}) == 3
    full = want_of("33 x 65, full, 4-connected")
    assert full["objects"][0, 0].tolist() == [0, 33 * 65, 0, 32, 0, 64, 1, 0]
    spiral = want_of("130 x 197, a spiral, 4-connected")
    assert spiral["objects"][0, 0, 0] == 0 and spiral["objects"][0, 0, 1] > 6000


@pytest.fixture(scope="module")
def host_uf(tmp_path_factory):
    """tests/objects_uf_host.cpp as a shared library: the union-find body of the kernels, compiled for the host."""
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    lib = str(tmp_path_factory.mktemp("objects_uf") / "libobjects_uf_host.so")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(REPO, "camradepth_amd", "csrc"),
                        os.path.join(REPO, "tests", "objects_uf_host.cpp"), "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    fn = ctypes.CDLL(lib).uf_partition
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]
    return fn


def test_the_union_find_body_in_natural_and_in_shuffled_order(host_uf):
    done = set()
    for name, c in CASES.items():
        src_all = objects_ref.source_mask(c["state"], c["sources"])
        for m in range(src_all.shape[0]):
            src = np.ascontiguousarray(src_all[m], np.uint8)
            key = (src.tobytes(), src.shape, c["connectivity"])
            if key in done:
                continue
            done.add(key)
            want = objects_ref.first_cells(src_all[m], c["connectivity"]).astype(np.int32)
            for seed in (0, 1, 0x9E3779B97F4A7C15):
                root = np.full(src.shape, 7, np.int32)
                capped = host_uf(src.ctypes.data, src.shape[0], src.shape[1], c["connectivity"], seed, root.ctypes.data)
                assert capped == 0 and np.array_equal(root, want), (name, m, seed)
