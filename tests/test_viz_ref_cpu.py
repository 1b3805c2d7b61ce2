"""CPU: tests/viz_ref.py, the NumPy restatement the visualisation kernels are held to, against what it restates: matplotlib's
plt.imsave -> PNG -> RGB for float maps and labels, matplotlib's jet and rainbow tables and their published construction for the
literal tables in the package, scipy's grey dilation, and np.argmax / torch.max for the label map."""
import io

import numpy as np
import pytest
import torch

from tests import viz_ref as ref

F = np.float32


def builtin(name):
    from camradepth_amd._viz_tables import TABLES
    t = np.frombuffer(TABLES[name], dtype=np.uint8).reshape(256, 3)
    return t


def imsave_rgb(a, cmap, **kw):
    """plt.imsave -> PNG bytes -> uint8 RGB, alpha dropped."""
    plt = pytest.importorskip("matplotlib.pyplot")
    buf = io.BytesIO()
    plt.imsave(buf, a, cmap=cmap, format="png", **kw)
    buf.seek(0)
    img = plt.imread(buf, format="png")                       # float32 [h,w,4] in k / 255
    rgb = np.rint(img[..., :3] * 255).astype(np.uint8)
    assert np.array_equal(rgb.astype(F) / F(255), img[..., :3])
    return rgb


def test_builtin_tables_are_matplotlibs_and_their_published_construction():
    # jet: linear segments (matplotlib's _jet_data), rainbow: |2x - 0.5|, sin(pi x), cos(pi x / 2) (gnuplot palette 33, 13, 10)
    x = np.linspace(0, 1, 256)
    seg = {"red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
           "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
           "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0))}
    jet = np.stack([np.interp(x, *zip(*seg[c])) for c in ("red", "green", "blue")], axis=1)
    rainbow = np.stack([np.abs(2 * x - 0.5), np.sin(np.pi * x), np.cos(np.pi * x / 2)], axis=1)
    for name, lut in (("jet", jet), ("rainbow", rainbow)):
        t = builtin(name)
        assert t.shape == (256, 3) and t.dtype == np.uint8
        built = (np.clip(lut, 0, 1) * 255).astype(np.uint8)
        assert np.array_equal(t, built), (name, np.argwhere(t != built)[:4])
    mpl = pytest.importorskip("matplotlib")
    for name in ("jet", "rainbow"):
        cm = mpl.colormaps[name]
        cm._init()
        assert np.array_equal(builtin(name), (cm._lut[:256, :3] * 255).astype(np.uint8)), name


def float_maps():
    rs = np.random.RandomState(5)
    maps = {}
    for i in range(12):
        m = rs.standard_normal(size=(13, 21)).astype(F)
        if i % 3 == 1:
            m[rs.uniform(size=m.shape) < 0.7] = 0
        if i % 4 == 2:
            m *= F(100)
        maps[f"random {i}"] = m
    maps["uniform 0..1"] = rs.uniform(size=(9, 30)).astype(F)
    maps["constant"] = np.full((4, 6), 3.25, dtype=F)
    maps["zeros"] = np.zeros((4, 6), dtype=F)
    for lo, hi in ((0.0, 1.0), (-3.0, 5.0), (0.1, 0.7), (2.5, 80.0)):
        maps[f"bin boundaries {lo} .. {hi}"] = (F(lo) + np.arange(257, dtype=F) / F(256) * F(hi - lo)).astype(F).reshape(1, 257)
    for i in range(8):                                        # ranges that are no short binary fractions: the quotient rounds near the boundary
        lo, span = F(rs.uniform(-5, 5)), F(rs.uniform(0.01, 100))
        maps[f"bin boundaries, random range {i}"] = (lo + np.arange(257, dtype=F) / F(256) * span).astype(F).reshape(1, 257)
    maps["negative and -0.0"] = np.array([[-0.0, 0.0, -1.0, 1.0, 1e-30, -1e-30]], dtype=F)
    maps["subnormals"] = np.array([[0.0, 1e-45, 3e-39, 1e-38, -2e-40]], dtype=F)
    return maps


def test_float_maps_equal_imsave():
    jet = builtin("jet")
    for name, m in float_maps().items():
        got = ref.colorize(m[None], jet)[0]
        want = imsave_rgb(m, "jet")
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
    # fixed ranges: values below, at and above the ends
    m = np.array([[-2.0, -1.0, -0.999, 0.0, 0.5, 2.999, 3.0, 3.001, 7.0]], dtype=F)
    for lo, hi in ((-1.0, 3.0), (0.0, 0.5), (-5.0, 10.0), (0.25, 0.25)):
        got = ref.colorize(m[None], jet, lo, hi)[0]
        want = imsave_rgb(m, "jet", vmin=lo, vmax=hi)
        assert np.array_equal(got, want), ((lo, hi), got[0, :, 0], want[0, :, 0])
    # x == vmax takes the last row, below vmin the first
    got = ref.colorize(m[None], jet, -1.0, 3.0)[0, 0]
    assert np.array_equal(got[6], jet[255]) and np.array_equal(got[0], jet[0]) and np.array_equal(got[8], jet[255])
    # ranges per frame, as a [B, 2] array
    both = np.stack([m, m])
    got = ref.colorize(both, jet, np.array([-1.0, 0.0], dtype=F), np.array([3.0, 0.5], dtype=F))
    assert np.array_equal(got[0], imsave_rgb(m, "jet", vmin=-1.0, vmax=3.0)) and np.array_equal(got[1], imsave_rgb(m, "jet", vmin=0.0, vmax=0.5))


def test_labels_equal_imsave():
    rainbow = builtin("rainbow")
    rs = np.random.RandomState(6)
    cases = {"0..20": rs.randint(0, 21, size=(12, 17)), "one value": np.full((3, 5), 7), "all 256": np.arange(256).reshape(8, 32)}
    with_ignore = rs.randint(0, 21, size=(12, 17))
    with_ignore[rs.uniform(size=with_ignore.shape) < 0.05] = 255
    cases["0..20 and 255"] = with_ignore
    cases["two values"] = np.array([[3, 9, 9, 3]])
    for name, lab in cases.items():
        got = ref.colorize(lab.astype(np.uint8)[None], rainbow)[0]
        for dtype in (np.uint8, np.int64):                   # the reference saves int64 labels; uint8 gives the same picture
            want = imsave_rgb(lab.astype(dtype), "rainbow")
            assert np.array_equal(got, want), (name, dtype, np.argwhere(got != want)[:4])
    got = ref.colorize(with_ignore.astype(np.uint8)[None], rainbow, 0, 20)[0]
    assert np.array_equal(got, imsave_rgb(with_ignore, "rainbow", vmin=0, vmax=20))


def test_non_finite_pixels_are_left_out_of_the_range():
    jet = builtin("jet")
    m = np.array([[0.0, 1.0, np.nan, 4.0, np.inf, -np.inf, 2.0]], dtype=F)
    got = ref.colorize(m[None], jet, bad_colour=(9, 8, 7))[0, 0]
    finite = np.isfinite(m[0])
    assert np.array_equal(got[finite], ref.colorize(m[:, finite][None], jet)[0, 0])
    assert (got[~finite] == np.array([9, 8, 7])).all()
    assert ref.frame_range(m[None]).tolist() == [[0.0, 4.0]]
    allnan = np.full((1, 2, 3), np.nan, dtype=F)
    assert ref.frame_range(allnan).tolist() == [[0.0, 0.0]] and (ref.colorize(allnan, jet, bad_colour=(1, 2, 3)) == np.array([1, 2, 3])).all()


def test_dilation_equals_scipys_grey_dilation():
    ndimage = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(7)
    r = rs.uniform(0.0, 1.3, size=(2, 14, 19)).astype(F)
    r[rs.uniform(size=r.shape) < 0.9] = 0
    r[0, 0, 0], r[0, -1, -1], r[1, 0, -1], r[1, 5, 5], r[1, 6, 6] = 0.5, 0.25, 1.0, np.nan, np.inf
    t = ref.radar_transform(r)
    assert t[1, 0, -1] == 0 and t[1, 5, 5] == 0 and t[1, 6, 6] == 0 and t[0, 0, 0] == F(0.5) and (t[np.isfinite(r) & (r > 1)] < 0).all()
    for k in (1, 3, 5, 9):
        want = np.stack([ndimage.grey_dilation(f, size=(k, k), mode="constant", cval=-np.inf) for f in t])
        assert np.array_equal(ref.dilate(t, k), want), k
    assert np.array_equal(ref.dilate(t, 1), t)


def test_argmax_equals_numpy_and_torch():
    rs = np.random.RandomState(8)
    for C in (1, 2, 21, 256):
        x = rs.standard_normal(size=(2, C, 5, 7)).astype(F)
        x = np.round(x * 2) / 2                               # ties
        if C > 1:
            x[0, :, 0, 0] = 1.0
            x[0, 1, 1, 1] = np.nan
            x[1, C - 1, 2, 2] = np.nan
            x[1, 0, 2, 2] = np.inf
            x[0, :, 3, 3] = np.nan
            x[1, :, 4, 4] = -np.inf
        got = ref.seg_labels(x)
        assert got.dtype == np.uint8
        assert np.array_equal(got, np.argmax(x, axis=1).astype(np.uint8)), C
        assert np.array_equal(got, torch.max(torch.from_numpy(x), dim=1)[1].numpy().astype(np.uint8)), C


def test_blend_grey_and_paste_by_hand():
    img = np.array([[[10, 20, 30], [255, 255, 255], [0, 0, 0], [2, 2, 2]]], dtype=np.uint8)[None]                # B, G, R
    assert np.array_equal(ref.to_rgb(img, "bgr")[0, 0, 0], [30, 20, 10]) and ref.to_rgb(img, "rgb") is img
    colour = np.array([[[2, 4, 6], [255, 0, 1], [1, 3, 255], [2, 2, 2]]], dtype=np.uint8)[None]
    got = ref.blend(img, colour, 0.5, 0.25)[0, 0]             # 5 + 0.5 = 5.5 -> 6 (even), 10 + 1 = 11, 15 + 1.5 = 16.5 -> 16
    assert got[0].tolist() == [6, 11, 16] and got[1].tolist() == [191, 128, 128] and got[3].tolist() == [2, 2, 2]          # 1.5 -> 2
    assert ref.blend(img, colour, 0.8, 0.75)[0, 0, 1].tolist() == [255, 204, 205]                                    # beyond 255 clamps
    assert ref.blend(img, colour, -1.0, 0.0)[0, 0, 0].tolist() == [0, 0, 0]
    g = ref.grey(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [30, 20, 10]]], dtype=np.uint8))
    assert g[0, :, 0].tolist() == [255, 0, 76, 150, 29, 22] and (g[..., 0] == g[..., 1]).all() and (g[..., 1] == g[..., 2]).all()
    x = np.array([[[0.0, 2.0, -1.0, np.nan]]], dtype=F)
    assert ref.paste(img, x, colour)[0, 0].tolist() == [img[0, 0, 0].tolist(), colour[0, 0, 1].tolist(), img[0, 0, 2].tolist(), img[0, 0, 3].tolist()]


def test_radar_overlay_by_hand():
    jet = builtin("jet")
    img = np.full((1, 5, 7, 3), 100, dtype=np.uint8)
    img[..., 0] = 50                                          # B, G, R = 50, 100, 100
    r = np.zeros((1, 5, 7), dtype=F)
    r[0, 2, 3] = 0.25
    got = ref.radar_overlay(img, r, jet, k=3)
    grey = (100 * 9798 + 100 * 19235 + 50 * 3735 + 16384) >> 15
    assert (got[0, 0] == grey).all() and (got[0, :, 0] == grey).all()
    assert (got[0, 1:4, 2:5] == jet[255]).all()               # the 3 x 3 block holds the frame's maximum
    r[0, 2, 3] = 1.0                                          # 1 - r = 0: the return vanishes
    assert (ref.radar_overlay(img, r, jet, k=3) == grey).all()
    r[0, 2, 3] = 1.5                                          # 1 - r < 0: the block is the frame's minimum and never > 0
    assert (ref.radar_overlay(img, r, jet, k=3) == grey).all()


def test_collage_tiles_the_panels():
    a, b = np.full((2, 3, 4, 3), 7, dtype=np.uint8), np.full((2, 3, 4, 3), 9, dtype=np.uint8)
    c = ref.collage({(0, 0): a, (1, 2): b}, 2, 3, 4)
    assert c.shape == (2, 6, 12, 3) and (c[:, :3, :4] == 7).all() and (c[:, 3:, 8:] == 9).all() and c.sum() == 7 * a.size + 9 * b.size
