"""CPU: what the augmentation's restatement (tests/augment_ref.py) promises, and what the library refuses without a GPU.
test_gpu_augment.py ties the kernels to that restatement bit for bit, so what holds here holds for the batches training sees."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import augment_ref as ref
from tests import dropout_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_pyramid_of_the_flipped_map_is_not_the_flipped_pyramid():
    """Why the levels are rebuilt from the augmented full map: with an even width the window of output column ox covers source
    columns 2ox-1 .. 2ox+1, which is not mirror-symmetric.  A fixed sparse 8 x 12 map shows it."""
    full = np.zeros((1, 1, 8, 12), dtype=np.float32)
    for (y, x, v) in ((0, 0, 0.5), (1, 11, 0.25), (3, 4, 0.75), (4, 5, 0.125), (6, 2, 0.625), (7, 9, 0.375)):
        full[0, 0, y, x] = v
    flipped = np.ascontiguousarray(full[..., ::-1])
    a, b = ref.pyramid(flipped, 3), [np.ascontiguousarray(m[..., ::-1]) for m in ref.pyramid(full, 3)]
    assert [m.shape for m in a] == [(1, 1, 4, 6), (1, 1, 2, 3), (1, 1, 1, 2)]
    assert not np.array_equal(a[0], b[0])
    # the point at (3, 4): an even column lies in one window (ox = 2), its mirror image, column 7, in two (ox = 3 and 4)
    pooled, pooled_f = ref.min_pool(full), ref.min_pool(flipped)
    assert list(pooled[0, 0, 1, 1:4]) == [0.0, 0.75, 0.0]
    assert list(pooled_f[0, 0, 1, 2:5]) == [0.0, 0.75, 0.75] and list(b[0][0, 0, 1, 2:5]) == [0.0, 0.75, 0.0]
    # the host min-pool written out here is the project's (torch) one
    import torch
    from camradepth_amd import synth
    assert np.array_equal(synth.min_pool_ignore_zero(torch.from_numpy(full)).numpy(), ref.min_pool(full))
    odd = np.zeros((2, 1, 7, 9), dtype=np.float32)
    odd[0, 0, ::3, ::2], odd[1, 0, 6, 8] = 0.5, 0.25
    assert np.array_equal(synth.min_pool_ignore_zero(torch.from_numpy(odd)).numpy(), ref.min_pool(odd))


def test_crop_offsets_cover_their_range_and_the_flip_rate_is_p():
    H, W, h, w = 96, 128, 64, 96                       # H - h = W - w = 32
    rows = np.concatenate([ref.draw(64, H, W, h, w, p=0.5, seed=11, counter=c) for c in range(64)])
    assert rows.shape == (4096, 8)
    y0, x0, flip = rows[:, 0], rows[:, 1], rows[:, 2]
    assert y0.min() == 0 and y0.max() == H - h and x0.min() == 0 and x0.max() == W - w
    assert set(np.unique(flip)) == {0, 1}
    assert abs(flip.mean() - 0.5) < 0.04               # five standard deviations of 4096 fair coins are 0.039
    # nothing to crop, nothing to flip
    ident = ref.draw(64, H, W, H, W, p=0.0, seed=11, counter=3)
    assert not ident[:, :3].any() and (ref.floats(ident) == 1.0).all()
    assert ref.draw(64, H, W, h, w, p=1.0, seed=11)[:, 2].all()


def test_scalar_and_array_hash_agree():
    rows = ref.draw(3, 70, 101, 32, 64, p=0.5, seed=5, rank=2, counter=9)
    for b in range(3):
        assert rows[b, 0] == (ref.top24(b * 8, 5, 2, 9) * 39) >> 24 and rows[b, 1] == (ref.top24(b * 8 + 1, 5, 2, 9) * 38) >> 24


def test_slots_are_fixed():
    """Switching one photometric transform off leaves every other word as it was (and writes 1.0 in its own)."""
    full = dict(gamma=(0.9, 1.1), brightness=(0.75, 1.25), colour=(0.9, 1.1))
    base = ref.draw(16, 96, 128, 64, 96, p=0.5, seed=3, counter=2, **full)
    cols = {"gamma": [3], "brightness": [4], "colour": [5, 6, 7]}
    assert (ref.floats(base) != 1.0).all()
    for off, own in cols.items():
        got = ref.draw(16, 96, 128, 64, 96, p=0.5, seed=3, counter=2, **{k: v for k, v in full.items() if k != off})
        others = [c for c in range(8) if c not in own]
        assert np.array_equal(got[:, others], base[:, others]) and (ref.floats(got)[:, [c - 3 for c in own]] == 1.0).all()
    lo = ref.floats(base)
    assert (lo[:, 0] >= np.float32(0.9)).all() and (lo[:, 0] <= np.float32(1.1)).all()
    assert (lo[:, 1] >= np.float32(0.75)).all() and (lo[:, 1] <= np.float32(1.25)).all()
    # no crop and no flip either: the photometric words do not move
    assert np.array_equal(ref.draw(16, 96, 128, 96, 128, p=0.0, seed=3, counter=2, **full)[:, 3:], base[:, 3:])


def test_augmentation_stream_is_not_a_dropout_stream():
    """Equal seed and counter: the engine's DropPath draw uses (s, c), its Dropout2d draw (s + 1, c + 1); augmentation must match neither."""
    n = 256
    for seed in (0, 7, dropout_ref.M64):
        for counter in (0, 1, 12):
            s = dropout_ref.rank_seed(seed, 0)
            aug = dropout_ref.uniforms(n, ref.stream_seed(seed, 0), counter)
            for other in (dropout_ref.uniforms(n, s, counter), dropout_ref.uniforms(n, (s + 1) & dropout_ref.M64, counter + 1),
                          dropout_ref.uniforms(n, (s + 1) & dropout_ref.M64, counter)):
                assert (aug == other).mean() < 0.05
    assert ref.stream_seed(0, 1) != ref.stream_seed(0, 0)


def test_stream_constant_is_stated_once_per_layer(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    assert int(re.search(r"#define\s+CRD_AUGMENT_STREAM\s+(0x[0-9A-Fa-f]+)", h).group(1), 16) == ref.AUG_STREAM == built.AUGMENT_STREAM
    assert int(re.search(r"#define\s+CRD_AUGMENT_WORDS\s+(\d+)", h).group(1)) == ref.WORDS == built.AUGMENT_WORDS


def test_identity_table_is_the_plain_normalisation():
    """With nothing enabled the table is ((float)v / 255 - mean) / std."""
    ident = ref.draw(2, 64, 96, 64, 96)
    t = ref.lut(ident, gamma=False, brightness=False, colour=False)
    v = np.arange(256, dtype=np.float32)
    for c in range(3):
        want = (v / np.float32(255) - ref.MEAN[c]) / ref.STD[c]
        assert np.abs(t[0, c] - want).max() <= 2.4e-7          # float64 against the fp32 chain: one rounding of values below 2.7


def test_bad_arguments_are_refused_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(64)              # any non-NULL host address: a refused call launches nothing and reads none of it
    a = ctypes.addressof(buf)

    def refused(fn, args, word):
        rc = fn(*args)
        msg = L.crd_last_error()
        assert rc == -1 and fn.__name__.encode() in msg and word in msg, (fn.__name__, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, fn.__name__)

    def draw(params=a, B=2, H=64, W=96, h=32, w=64, p=0.5, g=(1, 1), br=(1, 1), co=(1, 1), enable=0):
        return (params, None, B, H, W, h, w, p, g[0], g[1], br[0], br[1], co[0], co[1], enable, 0, 0, None)

    refused(L.crd_augment_draw, draw(params=None), b"null")
    refused(L.crd_augment_draw, draw(h=96), b"larger than the frame")
    refused(L.crd_augment_draw, draw(w=128), b"larger than the frame")
    refused(L.crd_augment_draw, draw(h=48), b"multiple of 32")
    refused(L.crd_augment_draw, draw(w=40), b"multiple of 32")
    refused(L.crd_augment_draw, draw(p=-0.1), b"probability")
    refused(L.crd_augment_draw, draw(p=1.5), b"probability")
    refused(L.crd_augment_draw, draw(p=float("nan")), b"probability")
    refused(L.crd_augment_draw, draw(g=(1.1, 0.9), enable=built.AUGMENT_GAMMA), b"gamma")
    refused(L.crd_augment_draw, draw(br=(1.25, 0.75), enable=built.AUGMENT_BRIGHTNESS), b"brightness")
    refused(L.crd_augment_draw, draw(co=(1.1, 0.9), enable=built.AUGMENT_COLOUR), b"colour")
    refused(L.crd_augment_draw, draw(B=0), b"bad argument")
    refused(L.crd_augment_lut, (None, 2, 0, a, None), b"null")
    refused(L.crd_augment_lut, (a, 2, 0, None, None), b"null")

    def assemble(img=a, params=a, lut=a, out=a, H=64, W=96, h=32, w=64, seg=None, fseg=None):
        return (img, a, None, a, seg, params, lut, 2, H, W, h, w, 100.0, out, a, fseg, None, None)

    refused(L.crd_augment_assemble, assemble(img=None), b"null")
    refused(L.crd_augment_assemble, assemble(params=None), b"null")
    refused(L.crd_augment_assemble, assemble(lut=None), b"null")
    refused(L.crd_augment_assemble, assemble(out=None), b"null")
    refused(L.crd_augment_assemble, assemble(seg=a), b"null final_seg")
    refused(L.crd_augment_assemble, assemble(h=96), b"larger than the frame")
    refused(L.crd_augment_assemble, assemble(w=48), b"multiple of 32")

    def gather(image=a, params=a, C=7, h=32, w=64, seg=None, seg_out=None):
        return (image, a, seg, params, 2, C, 64, 96, h, w, a, a, seg_out, None, None)

    refused(L.crd_augment_gather, gather(image=None), b"null")
    refused(L.crd_augment_gather, gather(params=None), b"null")
    refused(L.crd_augment_gather, gather(seg=a), b"null seg_out")
    refused(L.crd_augment_gather, gather(C=0), b"channels")
    refused(L.crd_augment_gather, gather(h=128), b"larger than the frame")
    refused(L.crd_augment_gather, gather(h=16), b"multiple of 32")
    refused(L.crd_gt_pyramid_from_full, (None, 2, 32, 64, a, None, None, None), b"bad argument")
    refused(L.crd_gt_pyramid_from_full, (a, 2, 32, 64, a, None, a, None), b"needs the one above")


def test_augment_object_validates_and_carries_its_counter(built):
    from camradepth_amd.batch import Augment
    for bad in (dict(crop=(48, 64)), dict(crop=(0, 64)), dict(hflip=1.5), dict(hflip=-0.5), dict(gamma=(1.1, 0.9)),
                dict(gamma=(0.0, 1.0)), dict(brightness=(1.25, 0.75)), dict(colour=(1.1, 0.9))):
        with pytest.raises(built.CrdError):
            Augment(**bad)
    off = Augment()
    assert off.crop is None and off.hflip == 0.0 and off.enable == 0 and off.out_shape(64, 96) == (64, 96)
    aug = Augment(crop=(32, 64), hflip=0.5, gamma=(0.9, 1.1), colour=(0.9, 1.1), seed=7, rank=1)
    assert aug.enable == built.AUGMENT_GAMMA | built.AUGMENT_COLOUR and aug.out_shape(64, 96) == (32, 64)
    aug.counter = 41
    other = Augment(crop=(32, 64))
    other.load_state_dict(aug.state_dict())
    assert other.counter == 41 and aug.state_dict() == {"counter": 41}
