"""CPU: the lidar front end's restatement (tests/lidar_ref.py) against the fixture the reference's own ground-truth stage produced
(tests/golden/lidar_gt.npz, tests/golden/make_lidar_golden.py) and against plain sequential loops, the conditions the GPU test's inputs
have to meet, and the C ABI of the two entry points without a GPU.  test_gpu_lidar.py ties the kernels to the restatement and to the
same fixture."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import lidar_cases as cases
from tests import lidar_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crd_lidar_project", "crd_lidar_ground_truth")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return cases.load_fixture(golden_dir)


@pytest.mark.parametrize("stage", ["raster", "box", "flow"])
def test_restatement_equals_the_reference_in_fp64_after_every_stage(fixture, stage):
    c = fixture
    assert (c["size"], c["s"], c["cut"], c["shape"]) == ((900, 1600), 2, 34, (416, 800))
    got = ref.ground_truth64(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"], **c["stages"][stage])[:, 1:]
    want = c["f"]["entries_" + stage]
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (stage, got.shape, want.shape)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), stage          # bit for bit: row, col, depth, u, v, msk_lh


def test_fixture_holds_the_cases_it_was_built_for(fixture):
    """Ties, exact halves, the cutoff row, borders; boxes with a subset, none and all of their corners in view, a d_max from an
    out-of-view corner, bounds on exact halves, overlap; depth == d_max and the next double; in-box and seg-clear winners inside a
    rectangle; a flow error of exactly 3 and the next double; a pixel the box filter clears whose msk_lh was set."""
    c, f = fixture, fixture["f"]
    n, s, cut, (h, w) = len(f["x1"]), c["s"], c["cut"], c["shape"]
    xa, ya = ref.scaled(f["x1"], s, 799), ref.scaled(f["y1"], s, 449)
    pix = {}
    for i in range(n):
        pix.setdefault((int(round(ya[i])), int(round(xa[i]))), []).append(i)
    shared = [v for v in pix.values() if len(v) > 1]
    assert len(shared) >= 100 and sum(1 for v in shared if len({f["depth1"][i] for i in v}) < len(v)) >= 40
    assert sum(1 for a in (xa, ya) for v in a if v % 1 == 0.5) >= 18 and {int(v) % 2 for v in xa if v % 1 == 0.5} == {0, 1}
    assert (34, 350) in pix and (32, 351) in pix and sum(1 for (r, _) in pix if r < 34) >= 30
    assert (f["x1"] < 0).any() and (f["x1"] > 1599).any() and (f["y1"] < 0).any() and (f["y1"] > 899).any()
    view = f["corners"][..., 3] != 0
    per_box = view.sum(axis=1)
    assert (per_box == 0).any() and (per_box == 8).any() and ((per_box > 0) & (per_box < 8)).any()
    assert any((~v).any() and v.any() and k[:, 2].argmax() in np.nonzero(~v)[0] for k, v in zip(f["corners"], view))
    rects = ref.rectangles(f["corners"], s, cut, h, w)
    halves = [v for k, m in zip(f["corners"], view) for v in ((k[m, 0] + 0.5) / s - 0.5) if v % 1 == 0.5]
    assert {int(v) % 2 for v in halves} == {0, 1}
    inside = lambda q, r_, c_: q[0] <= c_ <= q[1] and q[2] <= r_ <= q[3]          # noqa: E731
    stage = {k: {(int(e[0]), int(e[1])): e for e in f["entries_" + k]} for k in ("raster", "box", "flow")}
    assert any(sum(inside(q, r_, c_) for q in rects) >= 2 for (r_, c_) in stage["raster"])                    # overlapping rectangles
    d_maxes = {q[4] for q in rects}
    assert any(e[2] in d_maxes and k in stage["box"] for k, e in stage["raster"].items())                     # depth == d_max stays
    assert any(np.nextafter(e[2], 0.0) in d_maxes and k not in stage["box"] for k, e in stage["raster"].items())
    win = {}
    b, r, c_, i = ref.winners(c["proj"], c["off"], c["size"], s, cut)
    for r1, c1, i1 in zip(r, c_, i):
        win[(int(r1), int(c1))] = int(i1)
    covered = [k for k in stage["raster"] if any(inside(q, *k) and stage["raster"][k][2] > q[4] for q in rects)]
    assert sum(1 for k in covered if f["in_box"][win[k]] and f["seg"][k] and k in stage["box"]) >= 5          # in_box winners stay
    assert sum(1 for k in covered if not f["in_box"][win[k]] and not f["seg"][k] and k in stage["box"]) >= 5  # seg clear: they stay
    gone = [k for k in stage["raster"] if k not in stage["box"]]
    assert len(gone) >= 80 and sum(1 for k in gone if stage["raster"][k][5] == 1.0) >= 20                     # msk_lh was set
    fl = c["stages"]["flow"]["flow_im"][0].astype(np.float64)
    errs = {}
    for k in stage["box"]:
        j = win[k]
        e = np.array([ref.scaled(f["x2"][j], s, 799) - xa[j], ref.scaled(f["y2"][j], s, 449) - ya[j]]) - fl[k]
        errs[k] = np.sqrt(e[0] * e[0] + e[1] * e[1])
    assert any(v == 3.0 and k in stage["flow"] for k, v in errs.items())
    assert any(v == np.nextafter(3.0, 4.0) and k not in stage["flow"] for k, v in errs.items())
    assert len(stage["flow"]) < len(stage["box"]) < len(stage["raster"]) < n


def loop_ground_truth(proj, off, K, size, s, cut, seg=None, corners=None, corner_offsets=None, flow_im=None, thres=3.0):
    """The same contract as one sequential pass per stage, written as plainly as possible: points in order with 'replace on a strictly
    smaller depth', boxes in order with in-place clearing."""
    h_new, w_new = size[0] // s, size[1] // s
    h = h_new - cut
    B = len(off) - 1
    best = {}
    for b in range(B):
        for i in range(off[b], off[b + 1]):
            vals = [proj[k][i] for k in ref.PROJ_KEYS]
            if ("valid" in proj and not proj["valid"][i]) or not np.isfinite(vals).all() or not vals[2] > 0:
                continue
            r, c = int(round(float(ref.scaled(vals[1], s, h_new - 1)))) - cut, int(round(float(ref.scaled(vals[0], s, w_new - 1))))
            if r >= 0 and ((b, r, c) not in best or vals[2] < proj["depth1"][best[(b, r, c)]]):
                best[(b, r, c)] = i
    if seg is not None:
        for b in range(B):
            for j in range(corner_offsets[b], corner_offsets[b + 1]):
                k = corners[j]
                m = k[:, 3] != 0
                if not m.any():
                    continue
                xs, ys = np.clip((k[m, 0] + 0.5) / s - 0.5, 0, w_new - 1), np.clip((k[m, 1] + 0.5) / s - 0.5 - cut, 0, h - 1)
                for r in range(int(round(ys.min())), int(round(ys.max())) + 1):
                    for c in range(int(round(xs.min())), int(round(xs.max())) + 1):
                        i = best.get((b, r, c))
                        if i is not None and seg[b, r, c] and not proj["in_box"][i] and proj["depth1"][i] > k[:, 2].max():
                            del best[(b, r, c)]
    out = {}
    for (b, r, c), i in best.items():
        fx = float(ref.scaled(proj["x2"][i], s, w_new - 1) - ref.scaled(proj["x1"][i], s, w_new - 1))
        fy = float(ref.scaled(proj["y2"][i], s, h_new - 1) - ref.scaled(proj["y1"][i], s, h_new - 1))
        if flow_im is not None:
            ex, ey = fx - float(flow_im[b, r, c, 0]), fy - float(flow_im[b, r, c, 1])
            if (ex * ex + ey * ey) ** 0.5 > thres:
                continue
        out[(b, r, c)] = (i, fx, fy)
    return out


@pytest.mark.parametrize("name", list(cases.RAGGED))
def test_restatement_equals_a_sequential_loop(name):
    """'The first of equal depths' and 'the union over boxes equals the reference's sequential clearing', on the small ragged cases."""
    c = cases.ragged_case(name)
    for filt in ({}, {k: c["filters"][k] for k in ("seg", "corners", "corner_offsets")}, c["filters"]):
        for proj in (c["proj"], {k: v for k, v in c["proj"].items() if k != "valid"}):
            want = loop_ground_truth(proj, c["off"], c["K"], c["size"], c["s"], c["cut"], **filt)
            got = ref.ground_truth64(proj, c["off"], c["K"], c["size"], c["s"], c["cut"], **filt)
            assert {(int(e[0]), int(e[1]), int(e[2])) for e in got} == set(want), (name, sorted(filt))
            for e in got:
                i = want[(int(e[0]), int(e[1]), int(e[2]))][0]
                assert e[3] == proj["depth1"][i] and e[6] == proj["low_h"][i]
    full = ref.ground_truth64(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"])
    box = ref.ground_truth64(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"],
                             **{k: c["filters"][k] for k in ("seg", "corners", "corner_offsets")})
    both = ref.ground_truth64(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"], **c["filters"])
    assert len(both) + 5 <= len(box) and len(box) + 5 <= len(full), (len(full), len(box), len(both))          # both filters do work
    gt, depth, msk = ref.ground_truth(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"], **c["filters"])
    assert gt.shape == (c["B"], c["size"][0] // c["s"] - c["cut"], c["size"][1] // c["s"], 3) and depth.flags.c_contiguous
    assert (depth != 0).sum() == len(both) and not msk[depth == 0].any() and msk.any()
    plain = ref.ground_truth(c["proj"], c["off"], c["K"], c["size"], c["s"], c["cut"])[1]
    assert all(((plain[b] != 0).any()) == (m > 0) for b, m in enumerate(c["counts"]))


def loop_project(c, min_distance=2.5, min_z=2.0, h_min=0.3, h_max=2.0):
    """Per point: the entries of its sweep in order, the first box that holds it."""
    n = len(c["pts"])
    hit, box = np.full(n, -1), np.zeros(n, dtype=np.uint8)
    for p in range(int(c["off"][0]), int(c["off"][-1])):
        s = int(c["sw"][p])
        for e in range(c["sweep_boxes"][s], c["sweep_boxes"][s + 1]):
            q = c["entries"][e][:12].reshape(3, 4) @ np.append(c["pts"][p], 1.0)
            if (np.abs(q) < c["entries"][e][12:]).all():
                hit[p], box[p] = e, c["vehicle"][c["box_id"][e]]
                break
    return hit, box


def test_projection_case_meets_its_margin_and_the_first_box_wins():
    """The condition of the GPU test: on the restatement's own fp64 values every point of a frame is at least 1e-6 (100 times the GPU
    test's bound) away from every box face, both height thresholds, the min_distance square, min_z and the image borders."""
    c = cases.projection_case()
    want = cases.project_ref(c)
    n_in = int(c["off"][-1])
    assert np.isfinite(want["margin"][:n_in]).all() and want["margin"][:n_in].min() >= 1e-6, want["margin"][:n_in].min()
    assert not np.isfinite(want["margin"][n_in:]).any() and not want["valid"][n_in:].any() and (want["box_entry"][n_in:] == -1).all()
    hit, box = loop_project(c)
    assert np.array_equal(hit, want["box_entry"]) and np.array_equal(box, want["in_box"])
    counts = np.bincount(hit[hit >= 0], minlength=6)
    assert counts[3] == 0 and (np.delete(counts, 3) >= 10).all(), counts          # entry 3 lies inside entry 2, which comes first
    # nested boxes: points inside both of a pair went to the first of the pair
    for first, second in ((2, 3), (4, 5)):
        both = 0
        for p in np.nonzero(hit == first)[0]:
            q = c["entries"][second][:12].reshape(3, 4) @ np.append(c["pts"][p], 1.0)
            both += bool((np.abs(q) < c["entries"][second][12:]).all())
        assert both >= 5, (first, second, both)
    v, lo = want["valid"][:n_in], want["low_h"][:n_in]
    assert 0.1 < v.mean() < 0.9 and 0.05 < lo.mean() < 0.9 and 0 < want["in_box"].sum() < (hit >= 0).sum()
    x, y = np.abs(c["pts"][:n_in, 0]), np.abs(c["pts"][:n_in, 1])
    assert ((x < 2.5) & (y < 2.5)).any() and ((x < 2.5) & (y >= 2.5)).any() and ((x >= 2.5) & (y < 2.5)).any()
    Z, px, py = want["depth1"][:n_in], want["x1"][:n_in], want["y1"][:n_in]
    assert (Z < 2).any() and (px[Z >= 2] <= 0).any() and (px[Z >= 2] >= 1600).any() and (py[Z >= 2] <= 0).any() and (py[Z >= 2] >= 900).any()
    assert np.abs(np.stack([want[k] for k in ref.PROJ_KEYS])).max() < 1e6       # an ulp of 1.2e-10: room under the bound of 1e-8
    # other thresholds: the margin holds there too
    other = cases.project_ref(c, min_distance=1.0, min_z=10.0, h_min=-0.5, h_max=1.0)
    assert other["margin"][:n_in].min() >= 1e-6 and (other["valid"] != want["valid"]).any() and (other["low_h"] != want["low_h"]).any()


def test_boundary_case_is_exact_on_the_restatement():
    c, expected = cases.boundary_case()
    got = cases.project_ref(c)
    for j, (what, valid, low, in_box, entry) in enumerate(expected):
        assert (got["valid"][j], got["low_h"][j], got["in_box"][j], got["box_entry"][j]) == (valid, low, in_box, entry), what
    assert got["depth1"][11] == 2.0 and got["x1"][13] == 0.0 and got["x1"][15] == 1600.0 and got["x1"][14] == 0.25


def test_new_symbols_are_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in built._SIGS and getattr(L, name).argtypes is not None, f"{name} is not bound"
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, h, flags=re.S).group(1)
        assert not [a for a in args.split(",") if "double" in a and "*" not in a], name       # fp64 through memory or as bit patterns


def test_invalid_sizes_are_reported_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    bits = built.f64_bits

    def project(**kw):
        v = dict(B=1, n=4, n_sweeps=1, n_entries=1, n_boxes=1, k_stride=0, im_h=900, im_w=1600, min_distance=2.5, min_z=2.0, h_min=0.3,
                 points=a, entries=a)
        v.update(kw)
        return L.crd_lidar_project(v["points"], a, a, v["B"], v["n"], a, a, a, a, v["n_sweeps"], v["entries"], a, v["n_entries"], a, a, a,
                                   v["n_boxes"], a, v["k_stride"], v["im_h"], v["im_w"], v["min_distance"], v["min_z"], bits(v["h_min"]),
                                   bits(2.0), a, a, a, a, a, a, a, a, a, None)

    def ground_truth(**kw):
        v = dict(B=1, n=4, k_stride=0, im_h=900, im_w=1600, s=2, cut=34, seg=None, corner_offsets=None, n_boxes=0, flow=None, thres=3.0,
                 ws=a, ws_bytes=1 << 40, gt=a, msk=a)
        v.update(kw)
        return L.crd_lidar_ground_truth(a, a, a, a, a, a, a, None, a, v["B"], v["n"], a, v["k_stride"], v["im_h"], v["im_w"], v["s"],
                                        v["cut"], v["seg"], a, v["corner_offsets"], v["n_boxes"], v["flow"], bits(v["thres"]), v["ws"],
                                        v["ws_bytes"], v["gt"], a, v["msk"], None)

    def refused(rc, name, word):
        msg = L.crd_last_error()
        assert rc == -1 and name in msg and word in msg, (rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, name.decode())

    for kw, word in ((dict(B=0), b"bad argument"), (dict(n=-1), b"bad argument"), (dict(im_h=0), b"bad argument"),
                     (dict(n_sweeps=-1), b"bad argument"), (dict(n_entries=-1), b"bad argument"), (dict(n_boxes=-1), b"bad argument"),
                     (dict(k_stride=3), b"k_stride"), (dict(min_distance=-1.0), b"min_distance"), (dict(min_z=float("nan")), b"min_z"),
                     (dict(h_min=float("nan")), b"h_min"), (dict(points=None), b"null"), (dict(entries=None), b"box tables")):
        refused(project(**kw), b"crd_lidar_project", word)
    n_pix = 416 * 800
    for kw, word in ((dict(B=0), b"bad argument"), (dict(n=-1), b"bad argument"), (dict(n_boxes=-1), b"bad argument"),
                     (dict(s=0), b"downsample_scale"), (dict(s=901), b"downsample_scale"), (dict(cut=-1), b"y_cutoff"),
                     (dict(cut=450), b"y_cutoff"), (dict(k_stride=1), b"k_stride"), (dict(ws=None), b"null"),
                     (dict(ws_bytes=12 * n_pix - 1), b"workspace"), (dict(seg=a, corner_offsets=a, n_boxes=3, ws_bytes=12 * n_pix + 95), b"workspace"),
                     (dict(seg=a), b"together"), (dict(corner_offsets=a), b"together"), (dict(flow=a, thres=float("nan")), b"thres"),
                     (dict(ws=a + 4), b"aligned"), (dict(gt=a + 8), b"aligned"), (dict(msk=a + 2), b"aligned")):
        refused(ground_truth(**kw), b"crd_lidar_ground_truth", word)
    assert project(n=0, points=None) == 0                 # no points: nothing to launch


def test_python_interface_refuses_host_tensors_without_a_gpu(built):
    import torch
    from camradepth_amd import lidar
    z, u = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.uint8)
    proj = dict({k: z for k in lidar.PROJ_KEYS}, low_h=u, in_box=u)
    with pytest.raises(built.CrdError, match="cuda"):
        lidar.lidar_ground_truth(proj, torch.tensor([0, 4], dtype=torch.int32), torch.eye(3, dtype=torch.float64))
    with pytest.raises(built.CrdError, match="cuda") as refusal:
        lidar.project_lidar(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32),
                            torch.zeros(1, 3, 4, dtype=torch.float64), torch.zeros(1, 3, 4, dtype=torch.float64),
                            torch.zeros(1, 4, dtype=torch.float64), torch.eye(3, dtype=torch.float64))
    assert "radar" not in str(refusal.value)
    with pytest.raises(built.CrdError, match="leave no pixel") as refusal:              # a bad map size
        lidar.lidar_ground_truth(proj, torch.tensor([0, 4], dtype=torch.int32), torch.eye(3, dtype=torch.float64), y_cutoff=450)
    assert "radar" not in str(refusal.value)
    assert lidar.map_shape((900, 1600), 2, 34) == (416, 800)
    assert lidar.workspace_bytes(3) == 16 + 24 + 8 and lidar.workspace_bytes(4, 2) == 16 + 32 + 64
