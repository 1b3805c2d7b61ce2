#!/usr/bin/env python3
"""Generate tests/golden/lidar_gt.npz by running the REAL reference ground-truth stage on CPU.

Runs only in the build container (needs /root/reference).  lib/fuse_lidar.py is imported read-only with in-process stand-ins for
the packages it imports at module level and that are absent here (nuscenes, nuscenes.nuscenes, pyquaternion, skimage; matplotlib
and mpl_toolkits if missing); only its four pure-NumPy functions are called, in the order scripts/cal_gt.py:125-132 applies them:
cal_depthMap_flow, filter_occlusion_by_bbox, filter_occlusion and lidarFlow2uv, at the 900 x 1600 image the reference hard-codes,
downsample_scale 2, y_cutoff 34, thres 3.  Nothing of the reference is copied: the fixture holds the seeded inputs, the non-zero
output entries (row, col, depth, u, v, msk_lh) in float64 after each of the three stages, and the NumPy version.  The fixture
follows NumPy 2.x, where lidarFlow2uv's float32 map plus a float64 flow is float64.

    python tests/golden/make_lidar_golden.py
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SCALE, CUTOFF, H, W, THRES = 2, 34, 900, 1600, 3.0
K = np.array([[1266.4172, 0.0, 816.267], [0.0, 1270.5031, 491.507], [0.0, 0.0, 1.0]])        # fy != fx: the reference uses fx for v


def install_shims():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    nothing = lambda *a, **k: None                                  # noqa: E731
    mod("nuscenes"), mod("nuscenes.nuscenes", NuScenes=object), mod("nuscenes.utils")
    mod("nuscenes.utils.data_classes", LidarPointCloud=type("LidarPointCloud", (), {}))
    mod("nuscenes.utils.geometry_utils", view_points=nothing, transform_matrix=nothing)
    mod("pyquaternion", Quaternion=type("Quaternion", (), {}))
    sk = mod("skimage")
    sk.io = mod("skimage.io", imread=nothing)
    sk.transform = mod("skimage.transform", resize=nothing)
    for name in ("matplotlib.pyplot", "mpl_toolkits.axes_grid1"):
        try:
            importlib.import_module(name)
        except ImportError:
            parts = name.split(".")
            for i in range(1, len(parts) + 1):
                if ".".join(parts[:i]) not in sys.modules:
                    mod(".".join(parts[:i]), make_axes_locatable=nothing)


def load_reference():
    install_shims()
    spec = importlib.util.spec_from_file_location("ref_fuse_lidar", os.path.join(REF, "lib", "fuse_lidar.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def half_pixel(k):
    """The full-resolution coordinate whose scaled value is exactly k + 0.5."""
    return 2.0 * k + 1.5


def whole_pixel(k):
    """The full-resolution coordinate whose scaled value is exactly k."""
    return 2.0 * k + 0.5


# The flow-threshold pixels (column, map row): a flow error of exactly (3, 0) and of (nextafter(3, 4), 0), on points nearer than all others
EXACT3, ABOVE3 = (2, 300), (0, 304)
# The d_max pixels of box F: a depth equal to d_max and the next double above it
AT_DMAX, OVER_DMAX, F_DMAX = (116, 60), (118, 60), 1.25


def make_points(seed=20261019):
    """Seeded points (x1, y1, depth1, x2, y2, low_h, in_box) with every case the rasteriser can get wrong; the comments name them."""
    rs = np.random.RandomState(seed)
    rows = []

    def add(x1, y1, d, x2=None, y2=None, low=None, box=None):
        rows.append((x1, y1, d, x1 + rs.normal(0, 6) if x2 is None else x2, y1 + rs.normal(0, 2) if y2 is None else y2,
                     float(rs.uniform() < 0.5) if low is None else low, float(rs.uniform() < 0.2) if box is None else box))
        return len(rows) - 1

    for _ in range(300):                                             # the bulk: anywhere in the image
        add(rs.uniform(0, W), rs.uniform(0, H), rs.uniform(2, 100))
    for _ in range(900):                                             # dense where the boxes are, in front of and behind them
        add(rs.uniform(500, 1000), rs.uniform(250, 560), rs.uniform(2, 60))
    for _ in range(100):                                             # pixel collisions: an earlier point's pixel, another depth
        j = rs.randint(len(rows))
        add(rows[j][0] + rs.uniform(-0.2, 0.2), rows[j][1], rs.uniform(2, 100))
    for _ in range(50):                                              # exact fp64 depth ties: the earlier point keeps the pixel
        j = rs.randint(len(rows))
        add(rows[j][0], rows[j][1], rows[j][2], low=1.0 - rows[j][5], box=1.0 - rows[j][6])
    for _ in range(10):                                              # a tie of two behind a later, nearer third
        x, y, d = rs.uniform(0, W), rs.uniform(100, H), rs.uniform(10, 50)
        add(x, y, d), add(x, y, d), add(x, y, d - 1.0), add(x, y, d - 1.0)
    for _ in range(20):                                              # depths one fp64 ulp apart: equal as fp32
        x, y, d = rs.uniform(0, W), rs.uniform(100, H), rs.uniform(2, 100)
        add(x, y, d), add(x, y, np.nextafter(d, 0.0))                # the later one is nearer and takes the pixel
        x, y, d = rs.uniform(0, W), rs.uniform(100, H), rs.uniform(2, 100)
        add(x, y, d), add(x, y, np.nextafter(d, 1000.0))             # the later one is farther and does not
    for k in (100, 101, 254, 255, 0, 798):                           # scaled coordinate exactly k + .5: half to even, both parities
        add(half_pixel(k), rs.uniform(100, H), rs.uniform(2, 100))
        add(rs.uniform(0, W), half_pixel(k % 300 + 60), rs.uniform(2, 100))
        add(half_pixel(k), half_pixel(k % 300 + 61), rs.uniform(2, 100))
    add(700.0, half_pixel(33), 20.0), add(702.0, half_pixel(32), 20.0)    # 33.5 -> map row 34 = output row 0; 32.5 -> 32, cut off
    for _ in range(8):                                               # clipped at the four borders (point and flow target)
        add(rs.uniform(-9, 0), rs.uniform(100, 800), rs.uniform(2, 100))
        add(rs.uniform(1599.2, 1610), rs.uniform(100, 800), rs.uniform(2, 100))
        add(rs.uniform(0, W), rs.uniform(-9, 0), rs.uniform(2, 100))
        add(rs.uniform(0, W), rs.uniform(899.2, 910), rs.uniform(2, 100))
        add(rs.uniform(0, 30), rs.uniform(100, 800), rs.uniform(2, 100), x2=rs.uniform(-40, -1))
        add(rs.uniform(1570, W), rs.uniform(100, 800), rs.uniform(2, 100), x2=rs.uniform(1601, 1650))
        add(rs.uniform(0, W), rs.uniform(70, 90), rs.uniform(2, 100), y2=rs.uniform(-20, -1))
        add(rs.uniform(0, W), rs.uniform(880, H), rs.uniform(2, 100), y2=rs.uniform(901, 930))
    for _ in range(30):                                              # winners above the cutoff row
        add(rs.uniform(0, W), rs.uniform(0, 2 * CUTOFF), rs.uniform(2, 100))
    # the flow threshold: xa = column and xb - xa = 1.25 are exact, so with flow_im = (-1.75, 0.5) the error is exactly (3, 0); one with
    # xb two ulps of 1.25 farther, so that the error is nextafter(3, 4)
    c, r = EXACT3
    add(whole_pixel(c), whole_pixel(r), 1.5, x2=whole_pixel(c + 1.25), y2=whole_pixel(r + 0.5), low=1.0, box=0.0)
    c, r = ABOVE3
    add(whole_pixel(c), whole_pixel(r), 1.5, x2=3.0 + 2 * np.spacing(3.0), y2=whole_pixel(r + 0.5), low=1.0, box=0.0)
    # box F: a winner at exactly d_max stays, the next double above it goes; both low, neither in a box
    (c, r), (c2, r2) = AT_DMAX, OVER_DMAX
    add(whole_pixel(c), whole_pixel(r + CUTOFF), F_DMAX, low=1.0, box=0.0)
    add(whole_pixel(c2), whole_pixel(r2 + CUTOFF), np.nextafter(F_DMAX, 2.0), low=1.0, box=0.0)
    return np.array(rows, dtype=np.float64)


def make_corners():
    """Eight projected corners (x, y, depth, in_view) per box, in full-resolution pixels; the comments name the cases."""
    def box(x0, x1, y0, y1, d0, d1, view=None, depths=None):
        xs, ys = [x0, x1, x0, x1, x0 + 8, x1 - 8, x0 + 8, x1 - 8], [y0, y0, y1, y1, y0 + 6, y0 + 6, y1 - 6, y1 - 6]
        ds = [d0, d0, d0, d0, d1, d1, d1, d1] if depths is None else depths
        return [[x, y, d, 1.0 if view is None or view[i] else 0.0] for i, (x, y, d) in enumerate(zip(xs, ys, ds))]

    boxes = [
        box(560.0, 760.0, 300.0, 420.0, 20.0, 24.0),                                                  # A: all eight in view
        box(700.0, 900.0, 380.0, 500.0, 30.0, 35.0),                                                  # B: overlaps A, another d_max
        box(-120.0, 620.0, 430.0, 540.0, 15.0, 18.0, view=[0, 1, 0, 1, 0, 1, 0, 1]),                  # C: a strict subset in view
        box(1700.0, 1900.0, 300.0, 400.0, 5.0, 6.0, view=[0] * 8),                                    # D: none in view: does nothing
        box(820.0, 990.0, 260.0, 370.0, 12.0, 14.0, view=[1, 1, 1, 1, 1, 1, 1, 0],
            depths=[12.0, 12.0, 12.0, 12.0, 14.0, 14.0, 14.0, 40.0]),                                 # E: d_max from an out-of-view corner
        box(whole_pixel(112), whole_pixel(124), whole_pixel(56 + CUTOFF), whole_pixel(64 + CUTOFF), 1.0, F_DMAX),      # F: d_max = 1.25
        box(half_pixel(250), half_pixel(301), half_pixel(100 + CUTOFF), half_pixel(131 + CUTOFF), 22.0, 26.0),  # G: bounds on exact halves,
        box(half_pixel(255), half_pixel(300), half_pixel(103 + CUTOFF), half_pixel(130 + CUTOFF), 8.0, 9.0),    # H: ... of both parities
        box(400.0, 520.0, -200.0, 60.0, 3.0, 4.0),                                                    # I: above the cutoff, clipped to row 0
    ]
    return np.array(boxes, dtype=np.float64)


def make_seg(h, w):
    """A blocky vehicle mask: 16 x 16 blocks, two of three set."""
    r, c = np.mgrid[0:h, 0:w]
    return ((r // 16 + c // 16) % 3 != 0)


def entries(depth_map, uv, msk_lh):
    hit = depth_map != 0
    assert not (uv[~hit] != 0).any() and not msk_lh[~hit].any()
    r, c = np.nonzero(hit)
    return np.stack([r.astype(np.float64), c.astype(np.float64), depth_map[hit], uv[..., 0][hit], uv[..., 1][hit],
                     msk_lh[hit].astype(np.float64)], axis=1)


def main():
    ref = load_reference()
    pts = make_points()
    n = len(pts)
    x1, y1, d1, x2, y2, low, box = (pts[:, i].copy() for i in range(7))
    low, box = low.astype(bool), box.astype(bool)
    corners = make_corners()
    x_cn, y_cn, d_cn, m_cn = (corners[..., i].reshape(-1).copy() for i in range(4))
    m_cn = m_cn.astype(bool)
    depth_map, flow, msk_lh, msk_in = ref.cal_depthMap_flow(x1.copy(), y1.copy(), d1.copy(), x2.copy(), y2.copy(), d1.copy(), low, box,
                                                            SCALE, CUTOFF)
    h, w = depth_map.shape
    assert (h, w) == (H // SCALE - CUTOFF, W // SCALE) and depth_map.dtype == np.float64
    seg = make_seg(h, w)
    # the image flow, at rasterised pixels only (the filter reads it nowhere else): the lidar flow plus noise, so that some errors pass 3
    rs = np.random.RandomState(11)
    fr, fc = np.nonzero(depth_map > 0)
    fv = (flow[fr, fc] + rs.normal(0, 1.7, size=(len(fr), 2))).astype(np.float32)
    for (c, r) in (EXACT3, ABOVE3):
        fv[(fr == r - CUTOFF) & (fc == c)] = (-1.75, 0.5)
    flow_im = np.zeros((h, w, 2), dtype=np.float32)
    flow_im[fr, fc] = fv
    stages = {}
    uv = ref.lidarFlow2uv(flow.copy(), K, depth_map.copy(), SCALE, CUTOFF)
    assert uv.dtype == np.float64
    stages["raster"] = entries(depth_map, uv, msk_lh)
    # scripts/cal_gt.py:127-132
    depth_b, msk_d1 = ref.filter_occlusion_by_bbox(depth_map.copy(), seg, msk_in, x_cn, y_cn, d_cn, m_cn, SCALE, CUTOFF)
    flow_b, lh_b = flow * msk_d1[..., None], msk_lh * msk_d1
    stages["box"] = entries(depth_b, ref.lidarFlow2uv(flow_b.copy(), K, depth_b.copy(), SCALE, CUTOFF), lh_b)
    depth_f, lh_f, _, flow_f = ref.filter_occlusion(depth_b.copy(), lh_b.copy(), msk_in.copy(), flow_b.copy(), flow_im, thres=THRES)
    stages["flow"] = entries(depth_f, ref.lidarFlow2uv(flow_f.copy(), K, depth_f.copy(), SCALE, CUTOFF), lh_f)
    # the designed cases did what their comments say
    (c3, r3), (c4, r4) = EXACT3, ABOVE3
    assert depth_b[r3 - CUTOFF, c3] == 1.5 and depth_f[r3 - CUTOFF, c3] == 1.5                 # an error of exactly 3 stays
    assert depth_b[r4 - CUTOFF, c4] == 1.5 and depth_f[r4 - CUTOFF, c4] == 0                   # the next double above 3 goes
    assert depth_map[AT_DMAX[1], AT_DMAX[0]] == F_DMAX == depth_b[AT_DMAX[1], AT_DMAX[0]] and seg[AT_DMAX[1], AT_DMAX[0]]
    assert depth_map[OVER_DMAX[1], OVER_DMAX[0]] == np.nextafter(F_DMAX, 2.0) and depth_b[OVER_DMAX[1], OVER_DMAX[0]] == 0
    assert msk_lh[OVER_DMAX[1], OVER_DMAX[0]] and seg[OVER_DMAX[1], OVER_DMAX[0]]              # cleared by the box filter, msk_lh was set
    gone_b, gone_f = (depth_map > 0) & (depth_b == 0), (depth_b > 0) & (depth_f == 0)
    assert gone_b.sum() >= 100 and gone_f.sum() >= 100 and (gone_b & msk_lh).sum() >= 20 and (gone_f & lh_b).sum() >= 20
    path = os.path.join(HERE, "lidar_gt.npz")
    np.savez_compressed(path, x1=x1, y1=y1, depth1=d1, x2=x2, y2=y2, low_h=low.astype(np.uint8), in_box=box.astype(np.uint8),
                        corners=corners, seg=seg.astype(np.uint8), flow_rows=fr.astype(np.int16), flow_cols=fc.astype(np.int16),
                        flow_values=fv, K=K, image_size=np.array([H, W]), downsample_scale=np.array(SCALE), y_cutoff=np.array(CUTOFF),
                        thres=np.array(THRES), entries_raster=stages["raster"], entries_box=stages["box"], entries_flow=stages["flow"],
                        numpy_version=np.array(np.__version__))
    print(f"{path}: {n} points, {len(corners)} boxes, non-zero pixels {[len(v) for v in stages.values()]}, "
          f"{os.path.getsize(path)} bytes, numpy {np.__version__}")


if __name__ == "__main__":
    main()
