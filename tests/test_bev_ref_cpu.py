"""CPU: tests/bev_ref.py, the NumPy restatement of crd_bev_grid the GPU tests compare the kernels with, against an independent
per-point Python loop that keeps one dictionary entry per cell and compares as include/camradepth_hip.h words it.  Bit for bit: floats
are compared as their int32 views."""
import math

import numpy as np
import pytest

from tests import bev_cases, bev_ref

CASES = bev_cases.all_cases()


def loop(xyz, B, x_min, y_min, cell, nx, ny, frame_offsets=None, rows_per_frame=0, valid=None, label=None, T=None, z_lo=-math.inf,
         z_hi=math.inf, min_points=1, flip_x=False, flip_y=False):
    cells = {}                                                   # (b, i, j) -> [count, (z_max, its row), z_min]
    for p in range(len(xyz)):
        if valid is not None and not valid[p]:
            continue
        if frame_offsets is not None:
            owners = [b for b in range(B) if frame_offsets[b] <= p < frame_offsets[b + 1]]
            if not owners:
                continue
            b = owners[0]
        else:
            b = p // rows_per_frame
            if b >= B:
                continue
        x, y, z = (float(v) for v in xyz[p])
        if T is not None:
            M = [[float(v) for v in row] for row in (T[b] if np.ndim(T) == 3 else T)]
            x, y, z = (M[i][0] * x + M[i][1] * y + M[i][2] * z + M[i][3] for i in range(3))
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        z = z + 0.0
        if not z_lo <= z <= z_hi:
            continue
        qx, qy = (x - x_min) / cell, (y - y_min) / cell
        if math.isinf(qx) or math.isinf(qy):
            continue
        qx, qy = math.floor(qx), math.floor(qy)                  # Python integers: exact
        if not (0 <= qx < nx and 0 <= qy < ny):
            continue
        at = (b, nx - 1 - qx if flip_x else qx, ny - 1 - qy if flip_y else qy)
        if at not in cells:
            cells[at] = [1, (z, p), z]
        else:
            c = cells[at]
            c[0] += 1
            if z > c[1][0] or (z == c[1][0] and p < c[1][1]):
                c[1] = (z, p)
            c[2] = min(c[2], z)
    out = {"count": np.zeros((B, nx, ny), np.int32), "z_max": np.full((B, nx, ny), bev_ref.EMPTY, np.float32),
           "z_min": np.full((B, nx, ny), bev_ref.EMPTY, np.float32), "top_index": np.full((B, nx, ny), -1, np.int32),
           "occupancy": np.zeros((B, nx, ny), np.uint8)}
    if label is not None:
        out["top_label"] = np.full((B, nx, ny), 255, np.uint8)
    with np.errstate(over="ignore"):
        for at, (n, (top, row), low) in cells.items():
            out["count"][at], out["z_max"][at], out["z_min"][at], out["top_index"][at] = n, np.float32(top), np.float32(low), row
            out["occupancy"][at] = n >= min_points
            if label is not None:
                out["top_label"][at] = label[row]
    return out


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_per_point_loop(name):
    case = CASES[name]
    got, want = bev_ref.bev_grid(**case), loop(**case)
    assert set(got) == set(want) == {"count", "z_max", "z_min", "top_index", "occupancy"} | ({"top_label"} if case["label"] is not None else set())
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        assert np.array_equal(bits(got[k]), bits(want[k])), (name, k, np.argwhere(bits(got[k]) != bits(want[k]))[:5])


def test_the_planted_rows_land_where_the_header_says():
    """The loop and the restatement could agree on a wrong reading; these values are worked out by hand from the header."""
    g = bev_ref.bev_grid(**bev_cases.planted())
    n = len(bev_cases.planted()["xyz"])
    assert g["count"][0, 0, 0] == 4 and g["top_index"][0, 0, 0] == 1 and g["z_max"][0, 0, 0] == 1.5        # row 2 is masked, row 12 is the corner
    assert g["z_min"][0, 0, 0] == 0.5
    assert g["top_index"][0, 1, 1] == 4 and g["z_max"][0, 1, 1].view(np.int32) == 0 and g["z_min"][0, 1, 1] == -2.0       # +0.0, not -0.0
    assert g["count"][0, 2, 2] == 4 and g["top_index"][0, 2, 2] == 8 and g["z_max"][0, 2, 2] == -0.5 and g["z_min"][0, 2, 2] == -3.0
    assert g["top_index"][0, 2, 0] == 11 and g["count"][0, 2, 0] == 1                                       # x = 0.0 and y = 2.0: lower edges
    assert g["top_index"][0, 4, 6] == 16 and g["count"][0, 4, 6] == 1                                       # just below both upper edges
    assert g["count"][0].sum() == 4 + 3 + 4 + 1 + 1 + 1 + 2                                                 # rows 14, 15, 17 .. 23 are left out
    assert g["z_max"][0, 4, 0] == np.float32(3.4028235e38) and g["z_min"][0, 4, 0] == np.float32(-3.4028235e38)
    assert g["count"][1].sum() == 0 and (g["z_max"][1].view(np.uint32) == 0x7fc00000).all() and (g["top_index"][1] == -1).all()
    assert (g["top_label"][1] == 255).all() and (g["occupancy"][1] == 0).all()
    assert g["count"][2, 0, 0] == 2 and g["top_index"][2, 0, 0] == 26 and g["z_max"][2, 0, 0] == 4.0         # row 27 (7.0) is masked
    assert g["top_index"][2, 3, 6] == 29 and g["z_max"][2, 3, 6].view(np.int32) == 0                        # -0.0 against -1e-30
    assert g["count"][2, 4, 0] == 3 and g["top_index"][2, 4, 0] == 31
    assert g["count"].sum() == 16 + 7 and g["top_index"].max() < n - 5                                       # nothing from beyond the last frame
    assert g["top_label"][0, 0, 0] == 7 and (g["occupancy"] == (g["count"] >= 1)).all()
    f = bev_ref.bev_grid(**bev_cases.planted(flip_x=True, flip_y=True, min_points=3))
    for k in g:
        if k != "occupancy":
            assert np.array_equal(bits(f[k]), bits(g[k][:, ::-1, ::-1])), k
    assert np.array_equal(f["occupancy"], (f["count"] >= 3).astype(np.uint8)) and f["occupancy"].sum() == 4
    band = bev_ref.bev_grid(**bev_cases.planted(z_lo=0.0, z_hi=0.0))
    assert band["count"].sum() == 3 and band["top_index"][0, 1, 1] == 4 and band["top_index"][2, 3, 6] == 29


def test_workspace_formula():
    assert bev_ref.workspace_bytes(1, 1, 1) == 48 and bev_ref.workspace_bytes(2, 160, 160) == 20 * 51200
    assert bev_ref.workspace_bytes(1, 3, 1) == 32 + 32 + 16
