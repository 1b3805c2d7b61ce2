"""CPU: the camera front end without a GPU.  The NumPy restatement (tests/camera_ref.py) equals scipy.ndimage.zoom(order=1,
grid_mode=True) -- what scikit-image 0.19.3's resize(order=1, anti_aliasing=False) calls -- truncated to uint8 and cut, for every
factor the entry accepts; the new symbol is declared, exported and bound at the same ABI version; crd_camera_frontend refuses every
documented bad argument before any GPU call; the Python interface refuses what it can judge without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import camera_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "crd_camera_frontend"


def zoomed(im, s, cut, mode):
    from scipy import ndimage
    H, W, _ = im.shape
    h_new, w_new = H // s, W // s
    return ndimage.zoom(im.astype(np.float64), (h_new / H, w_new / W, 1), order=1, mode=mode, grid_mode=True).astype("uint8")[cut:]


def cases():
    out = [(size, s) for size in ((24, 36), (20, 28)) for s in (1, 2, 3, 4) if size[0] % s == 0 and size[1] % s == 0]
    assert ((20, 28), 3) not in out and len(out) == 7
    return out + [((900, 1600), 2)]


@pytest.mark.parametrize("size,s", cases(), ids=lambda v: str(v).replace(" ", ""))
def test_restatement_equals_scipy_zoom(size, s):
    rs = np.random.RandomState(7 + s)
    H, W = size
    im = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    im[:4, :4] = 255                                     # sums of four that would overflow a byte
    im[4:8, :4] = np.array([1, 2, 3], dtype=np.uint8)
    for cut in (0, 3) if H < 100 else (34,):
        got = ref.downsample(im[None], s, cut)[0]
        assert got.shape == (H // s - cut, W // s, 3) and got.dtype == np.uint8
        for mode in ("mirror", "reflect"):
            assert np.array_equal(got, zoomed(im, s, cut, mode)), (size, s, cut, mode)
    # the swap is a swap of the stored channels; a fourth byte and pitches change nothing
    assert np.array_equal(ref.downsample(im[None], s, 0, swap_rb=True), ref.downsample(im[None], s, 0)[..., ::-1])
    if H < 100:
        row, frame = W * 4 + 5, (W * 4 + 5) * H + 11
        buf = rs.randint(0, 256, size=7 + 2 * frame).astype(np.uint8)
        view = ref.frames_of(buf, 2, H, W, 4, row, frame, offset=7)
        dense = np.ascontiguousarray(view[..., :3])
        assert np.array_equal(ref.downsample(view, s, 1), ref.downsample(dense, s, 1))


def test_normalisation_is_fp32_operation_by_operation():
    image = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    x = ref.normalise(image)
    assert x.dtype == np.float32 and x.shape == (1, 3, 16, 16)
    for k in range(3):
        for v in (0, 1, 127, 254, 255):
            want = np.float32(np.float32(np.float32(v) / np.float32(255)) - ref.MEAN[k]) / ref.STD[k]
            assert x[0, k, v // 16, v % 16] == want and type(want) is np.float32
    got = ref.camera_inputs(np.zeros((2, 8, 12, 3), np.uint8), 2, 1)
    assert got["image"].shape == (2, 3, 6, 3) and got["x"].shape == (2, 3, 3, 6)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_new_symbol_is_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, h), f"{NAME} is not declared"
    assert hasattr(raw, NAME), f"{NAME} is not exported"
    assert NAME in built._SIGS and getattr(L, NAME).argtypes is not None, f"{NAME} is not bound"
    assert L.crd_version() == 13 and int(re.search(r"#define\s+CRD_ABI_VERSION\s+(\d+)", h).group(1)) == 13      # no struct, no changed signature
    from camradepth_amd import camera, radar
    assert camera.map_shape is radar.map_shape and camera.map_shape((900, 1600), 2, 34) == (416, 800)


def test_invalid_arguments_are_reported_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    base = dict(frames=a, B=2, im_h=900, im_w=1600, ch=3, row=4800, frame=900 * 4800, swap=1, s=2, cut=34, image=a, x=a, xc=7)

    def call(**kw):
        v = dict(base)
        v.update(kw)
        return L.crd_camera_frontend(v["frames"], v["B"], v["im_h"], v["im_w"], v["ch"], v["row"], v["frame"], v["swap"], v["s"], v["cut"],
                                     v["image"], v["x"], v["xc"], None)

    def refused(rc, status, word):
        msg = L.crd_last_error()
        assert rc == status and NAME.encode() in msg and word in msg, (rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, NAME)

    invalid = ((dict(frames=None), b"null"), (dict(image=None, x=None), b"null"), (dict(B=0), b"bad argument"), (dict(B=-1), b"bad argument"),
               (dict(im_h=0), b"bad argument"), (dict(im_w=-5), b"bad argument"), (dict(ch=2), b"channels"), (dict(ch=5), b"channels"),
               (dict(row=4799), b"row_pitch"), (dict(ch=4), b"row_pitch"), (dict(frame=900 * 4800 - 1), b"frame_pitch"),
               (dict(row=4816), b"frame_pitch"), (dict(s=0), b"downsample_scale"), (dict(s=5), b"downsample_scale"),
               (dict(s=-2), b"downsample_scale"), (dict(cut=-1), b"y_cutoff"), (dict(cut=450), b"y_cutoff"), (dict(s=4, cut=225), b"y_cutoff"),
               (dict(xc=2), b"x_channels"), (dict(xc=0), b"x_channels"), (dict(x=a + 2), b"aligned"))
    for kw, word in invalid:
        refused(call(**kw), -1, word)
    unsupported = ((dict(im_h=901, frame=901 * 4800), b"does not divide"), (dict(im_w=1599), b"does not divide"),
                   (dict(s=3), b"does not divide"), (dict(s=4, im_h=902, frame=902 * 4800), b"does not divide"),
                   (dict(B=1 << 15, im_h=1 << 10, im_w=1 << 10, row=3 << 10, frame=3 << 20, s=1, cut=0), b"32-bit"),
                   (dict(B=1000, xc=8), b"32-bit"))
    for kw, word in unsupported:
        refused(call(**kw), -2, word)


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import camera
    frames = torch.zeros(1, 900, 1600, 3, dtype=torch.uint8)
    with pytest.raises(built.CrdError, match="cuda"):
        camera.camera_inputs(frames)
    for kw in (dict(order_in="grb"), dict(order_out="RGB"), dict(downsample_scale=5), dict(downsample_scale=0), dict(downsample_scale=1.5)):
        with pytest.raises(built.CrdError, match="order|downsample_scale"):
            camera.camera_inputs(frames, **kw)
