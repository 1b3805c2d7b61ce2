#!/usr/bin/env python3
"""Generate tests/golden/radar_raster.npz by running the REAL reference rasteriser on CPU.

Runs only in the build container (needs /root/reference).  lib/fuse_radar.py is imported read-only with in-process stand-ins for
the packages it imports at module level and that are absent here (nuscenes, pyquaternion, skimage; matplotlib if missing); only its
two pure-NumPy functions are called: cal_depthMap_flow and radarFlow2uv, at the 900 x 1600 image the reference hard-codes,
downsample_scale 2, y_cutoff 34.  Nothing of the reference is copied: the fixture holds the seeded inputs, the non-zero output
entries (row, col, depth, u, v, rad_vel) in float64 and the NumPy version.

    python tests/golden/make_radar_golden.py
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SCALE, CUTOFF, H, W = 2, 34, 900, 1600
K = np.array([[1266.4172, 0.0, 816.267], [0.0, 1270.5031, 491.507], [0.0, 0.0, 1.0]])        # fy != fx: the reference uses fx for v


def install_shims():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    nothing = lambda *a, **k: None                                  # noqa: E731
    mod("nuscenes"), mod("nuscenes.utils")
    mod("nuscenes.utils.data_classes", RadarPointCloud=type("RadarPointCloud", (), {}))
    mod("nuscenes.utils.geometry_utils", view_points=nothing, transform_matrix=nothing)
    mod("pyquaternion", Quaternion=type("Quaternion", (), {}))
    sk = mod("skimage")
    sk.io = mod("skimage.io", imread=nothing)
    sk.transform = mod("skimage.transform", resize=nothing)
    try:
        importlib.import_module("matplotlib.pyplot")
    except ImportError:
        mp = mod("matplotlib")
        mp.pyplot = mod("matplotlib.pyplot")


def load_reference():
    install_shims()
    spec = importlib.util.spec_from_file_location("ref_fuse_radar", os.path.join(REF, "lib", "fuse_radar.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def half_pixel(k):
    """The full-resolution coordinate whose scaled value is exactly k + 0.5."""
    return 2.0 * k + 1.5


def make_points(seed=20261018):
    """Seeded points (x1, y1, depth1, x2, y2, v_comp) with every case the rasteriser can get wrong; the comments name them."""
    rs = np.random.RandomState(seed)
    rows = []

    def add(x1, y1, d, x2=None, y2=None, v=None):
        rows.append((x1, y1, d, x1 + rs.normal(0, 6) if x2 is None else x2, y1 + rs.normal(0, 2) if y2 is None else y2,
                     rs.uniform(0, 2) if v is None else v))
        return len(rows) - 1

    for _ in range(300):                                             # the bulk: anywhere in the image
        add(rs.uniform(0, W), rs.uniform(0, H), rs.uniform(2, 100))
    for _ in range(100):                                             # pixel collisions: an earlier point's pixel, another depth
        j = rs.randint(len(rows))
        add(rows[j][0] + rs.uniform(-0.2, 0.2), rows[j][1], rs.uniform(2, 100))
    for _ in range(50):                                              # exact fp64 depth ties: the earlier point keeps the pixel
        j = rs.randint(len(rows))
        add(rows[j][0], rows[j][1], rows[j][2])
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
    for _ in range(6):                                               # v_comp at the threshold: 0.5 is not moving, the next double is
        add(rs.uniform(0, W), rs.uniform(100, H), 1.5, v=0.5)
        add(rs.uniform(0, W), rs.uniform(100, H), 1.5, v=np.nextafter(0.5, 1.0))
    return np.array(rows, dtype=np.float64)


def main():
    ref = load_reference()
    pts = make_points()
    n = len(pts)
    rs = np.random.RandomState(7)
    times1, times2, rcs = rs.uniform(0, 0.5, n), rs.uniform(0, 0.5, n), rs.uniform(-5, 30, n)
    x1, y1, d1, x2, y2, vc = (pts[:, i].copy() for i in range(6))
    depth2 = d1 + rs.normal(0, 0.5, n)
    depth_map, flow, _, _, vel_map = ref.cal_depthMap_flow(x1.copy(), y1.copy(), d1.copy(), times1, x2.copy(), y2.copy(), depth2, times2,
                                                           rcs.copy(), vc.copy(), SCALE, CUTOFF)       # rcs: the reference adds to it
    uv = ref.radarFlow2uv(flow, K, depth_map, SCALE, CUTOFF)
    assert depth_map.shape == (H // SCALE - CUTOFF, W // SCALE) and depth_map.dtype == np.float64 and uv.dtype == np.float64
    hit = depth_map != 0
    assert not (uv[~hit] != 0).any() and not (vel_map[~hit] != 0).any()
    r, c = np.nonzero(hit)
    out = np.stack([r.astype(np.float64), c.astype(np.float64), depth_map[hit], uv[..., 0][hit], uv[..., 1][hit], vel_map[hit]], axis=1)
    path = os.path.join(HERE, "radar_raster.npz")
    np.savez_compressed(path, x1=x1, y1=y1, depth1=d1, x2=x2, y2=y2, v_comp=vc, K=K, image_size=np.array([H, W]),
                        downsample_scale=np.array(SCALE), y_cutoff=np.array(CUTOFF), entries=out, numpy_version=np.array(np.__version__))
    print(f"{path}: {n} points, {len(out)} non-zero pixels, {os.path.getsize(path)} bytes, numpy {np.__version__}")


if __name__ == "__main__":
    main()
