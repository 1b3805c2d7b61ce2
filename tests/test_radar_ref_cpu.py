"""CPU: the radar front end's restatement (tests/radar_ref.py) against the fixture the reference's own rasteriser produced
(tests/golden/radar_raster.npz, tests/golden/make_radar_golden.py), and the C ABI of the two entry points without a GPU.
test_gpu_radar.py ties the kernels to the restatement and to the same fixture."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import radar_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crd_radar_project", "crd_radar_rasterize")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "radar_raster.npz")))


def test_restatement_equals_the_reference_rasteriser_in_fp64(fixture):
    f = fixture
    size, s, cut = tuple(int(v) for v in f["image_size"]), int(f["downsample_scale"]), int(f["y_cutoff"])
    assert (size, s, cut) == ((900, 1600), 2, 34)
    proj = {k: f[k] for k in ref.PROJ_KEYS}
    n = len(proj["x1"])
    got = np.array([row[1:] for row in ref.rasterize64(proj, [0, n], f["K"], size, s, cut)], dtype=np.float64)
    want = f["entries"]
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    assert np.array_equal(got.view(np.int64), want.view(np.int64))              # bit for bit: row, col, depth, u, v, rad_vel


def test_fixture_holds_the_cases_it_was_built_for(fixture):
    """Collisions, exact ties, sub-fp32 depth differences, exact halves of both parities, all four borders, rows above the cutoff and
    v_comp at its threshold are in the inputs -- so equality with the reference above covers them."""
    f = fixture
    x1, y1, d1, x2, y2, vc = (f[k] for k in ref.PROJ_KEYS)
    n = len(x1)
    xa, ya = ref.scaled(x1, 2, 799), ref.scaled(y1, 2, 449)
    pix = {}
    for i in range(n):
        pix.setdefault((int(round(ya[i])), int(round(xa[i]))), []).append(i)
    shared = [v for v in pix.values() if len(v) > 1]
    assert sum(len(v) - 1 for v in shared) >= 100                                                   # points that met a taken pixel
    assert sum(len(v) - len({d1[i] for i in v}) for v in shared) >= 50                              # ... at exactly its fp64 depth
    sub32 = [v for v in shared if len({np.float32(d1[i]) for i in v}) < len({d1[i] for i in v})]
    assert len(sub32) >= 40                                                                         # differ below fp32 resolution
    assert any(d1[v[-1]] < d1[v[0]] for v in sub32) and any(d1[v[-1]] > d1[v[0]] for v in sub32)
    for a in (xa, ya):
        halves = a[(a % 1.0) == 0.5]
        assert {int(h) % 2 for h in halves} == {0, 1}
    assert (x1 < 0).any() and (x1 > 1599).any() and (y1 < 0).any() and (y1 > 899).any()
    assert (x2 < 0).any() and (x2 > 1600).any() and (y2 < 0).any() and (y2 > 900).any()
    assert sum(1 for (r, c) in pix if r < 34) >= 30 and (34, 350) in pix and (32, 351) in pix
    assert (vc == 0.5).any() and (vc == np.nextafter(0.5, 1.0)).any()
    won = {(int(r) + 34, int(c)): m for r, c, _, _, _, m in f["entries"]}
    for i in range(n):
        if vc[i] in (0.5, np.nextafter(0.5, 1.0)):
            assert won[(int(round(ya[i])), int(round(xa[i])))] == float(vc[i] > 0.5)
    assert all(r >= 0 for r, *_ in f["entries"]) and len(f["entries"]) < n


def test_restatement_skips_what_the_reference_raises_on():
    base = dict(x1=[10.0, 10.0, 10.0, 10.0], y1=[10.0] * 4, depth1=[5.0, 0.0, -1.0, 4.0], x2=[11.0, 11.0, 11.0, np.nan], y2=[10.0] * 4,
                v_comp=[1.0] * 4)
    K = np.array([[100.0, 0, 50.0], [0, 100.0, 40.0], [0, 0, 1.0]])
    assert [w[-1] for w in ref.winners(base, [0, 4], (80, 100), 2, 0)] == [0]
    base["valid"] = [0, 1, 1, 1]
    assert ref.winners(base, [0, 4], (80, 100), 2, 0) == []
    radar, vel = ref.rasterize(base, [0, 2, 2, 4], K, (80, 100), 2, 0)
    assert radar.shape == (3, 40, 50, 3) and vel.shape == (3, 40, 50) and not radar.any() and not vel.any()


def test_new_symbols_are_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    assert built.ABI_VERSION == 13 == int(re.search(r"#define\s+CRD_ABI_VERSION\s+(\d+)", h).group(1))
    L = built.load()
    assert L.crd_version() == 13
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in built._SIGS and getattr(L, name).argtypes is not None, f"{name} is not bound"
    # every fp64 quantity travels through device memory: no double parameter in either signature
    for name in NEW:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, h, flags=re.S).group(1)
        assert not [a for a in args.split(",") if "double" in a and "*" not in a], name


def test_invalid_sizes_are_reported_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15

    def project(**kw):
        v = dict(B=1, n=4, n_sweeps=1, k_stride=0, im_h=900, im_w=1600, min_distance=1.0, min_z=2.0, points=a)
        v.update(kw)
        return L.crd_radar_project(v["points"], a, a, v["B"], v["n"], a, a, a, v["n_sweeps"], a, v["k_stride"], v["im_h"], v["im_w"],
                                   v["min_distance"], v["min_z"], a, a, a, a, a, a, a, None)

    def rasterize(**kw):
        v = dict(B=1, n=4, k_stride=0, im_h=900, im_w=1600, s=2, cut=34, ws=a, ws_bytes=1 << 40, radar=a)
        v.update(kw)
        return L.crd_radar_rasterize(a, a, a, a, a, a, None, a, v["B"], v["n"], a, v["k_stride"], v["im_h"], v["im_w"], v["s"], v["cut"],
                                     v["ws"], v["ws_bytes"], v["radar"], a, None)

    def refused(rc, name, word):
        msg = L.crd_last_error()
        assert rc == -1 and name in msg and word in msg, (rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, name.decode())

    for kw, word in ((dict(B=0), b"bad argument"), (dict(n=-1), b"bad argument"), (dict(im_h=0), b"bad argument"),
                     (dict(im_w=-5), b"bad argument"), (dict(n_sweeps=-1), b"bad argument"), (dict(k_stride=3), b"k_stride"),
                     (dict(min_distance=-1.0), b"min_distance"), (dict(min_z=float("nan")), b"min_z"), (dict(points=None), b"null")):
        refused(project(**kw), b"crd_radar_project", word)
    for kw, word in ((dict(B=0), b"bad argument"), (dict(n=-1), b"bad argument"), (dict(im_h=0), b"bad argument"),
                     (dict(s=0), b"downsample_scale"), (dict(s=901), b"downsample_scale"), (dict(cut=-1), b"y_cutoff"),
                     (dict(cut=450), b"y_cutoff"), (dict(k_stride=1), b"k_stride"), (dict(ws=None), b"null"),
                     (dict(ws_bytes=12 * 416 * 800 - 1), b"workspace"), (dict(ws=a + 4), b"aligned"), (dict(radar=a + 8), b"aligned")):
        refused(rasterize(**kw), b"crd_radar_rasterize", word)
    assert project(n=0, points=None) == 0                 # no points: nothing to launch


def test_python_interface_refuses_host_tensors_without_a_gpu(built):
    import torch
    from camradepth_amd import radar
    z = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(built.CrdError, match="cuda"):
        radar.rasterize_radar({k: z for k in radar.PROJ_KEYS}, torch.tensor([0, 4], dtype=torch.int32), torch.eye(3, dtype=torch.float64))
    with pytest.raises(built.CrdError, match="cuda"):
        radar.project_radar(torch.zeros(4, 5, dtype=torch.float64), torch.zeros(4, dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32),
                            torch.zeros(1, 3, 4, dtype=torch.float64), torch.zeros(1, 3, 4, dtype=torch.float64),
                            torch.zeros(1, 2, dtype=torch.float64), torch.eye(3, dtype=torch.float64))
    assert radar.map_shape((900, 1600), 2, 34) == (416, 800) and radar.map_shape((101, 150), 2, 0) == (50, 75)
    assert radar.workspace_bytes(3) == 16 + 24
    with pytest.raises(built.CrdError):
        radar.map_shape((900, 1600), 2, 450)
