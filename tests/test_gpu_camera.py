"""GPU: the camera front end (camradepth_amd.camera.camera_inputs, crd_camera_frontend) against the NumPy restatement in
tests/camera_ref.py on the host copy of the same frames.  Every comparison is torch.equal, the fp32 planes as their bit patterns: the
image is integer arithmetic and the normalisation is specified operation by operation, and tests/test_camera_ref_cpu.py holds the
restatement to scipy.ndimage.zoom, so a result either has the restatement's bits or is wrong."""
import numpy as np
import pytest
import torch

from tests import camera_ref as ref

pytestmark = pytest.mark.gpu

B = 2
SENTINEL = 77


@pytest.fixture(scope="module")
def camera():
    from camradepth_amd import camera as module
    return module


def raw(seed, H, W, channels=3, row_pitch=None, offset=0):
    """B random frames on the device as a [B,H,W,channels] view of a flat buffer with the row pitch given (dense without) that begins
    `offset` bytes into the allocation; a few blocks of 255 so that the sum of four overflows a byte."""
    rs = np.random.RandomState(seed)
    row = W * channels if row_pitch is None else row_pitch
    frame = H * row + (0 if row_pitch is None else row)
    buf = torch.from_numpy(rs.randint(0, 256, size=offset + B * frame).astype(np.uint8)).cuda()
    view = torch.as_strided(buf, (B, H, W, channels), (frame, row, channels, 1), offset)
    view[:, :4, :6] = 255
    return view


def assert_bits(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} values differ; first at {i}: {got[i].item()!r} against {want[i].item()!r}")


def check(camera, frames, what, scales=(1, 2, 3, 4)):
    """Every dividing scale, y_cutoff 0 and 3, both orders: image and planes against the restatement -> the number of cases compared."""
    host = frames.cpu().numpy()
    H, W = frames.shape[1:3]
    n = 0
    for s in scales:
        if H % s or W % s:
            continue
        for cut in (0, 3):
            for order_in in ("rgb", "bgr"):
                got = camera.camera_inputs(frames, s, cut, order_in, "bgr", normalised=True)
                want = ref.camera_inputs(host, s, cut, swap_rb=order_in == "rgb")
                assert set(got) == {"image", "x"} and got["image"].shape == (B, H // s - cut, W // s, 3)
                assert_bits(got["image"], want["image"], f"{what}, s {s}, cut {cut}, {order_in}: image")
                assert_bits(got["x"], want["x"], f"{what}, s {s}, cut {cut}, {order_in}: x")
                n += 1
    return n


@pytest.mark.parametrize("size,n", [((24, 36), 16), ((20, 28), 12)], ids=["24x36", "20x28"])
def test_small_frames_against_the_restatement(camera, size, n):
    """w = 36, 18, 12, 9 and 28, 14, 7: whole groups of eight with and without a row tail, and rows shorter than one group.  The dense
    pitches of these frames are no multiples of 16, so every scale takes the per-pixel path."""
    assert check(camera, raw(1, *size), f"{size}") == n


def test_wide_path_and_its_fallback_on_the_same_frames(camera):
    """36 x 64 dense from an aligned base: row pitch 192 and frame pitch 6912 are multiples of 16, so s = 2 runs the 16-byte loads
    (w = 32: four whole groups per row).  The same pixels through a view with 4 channels and an odd row pitch, and through a dense view
    one byte into its allocation, run the per-pixel path and must give the same bytes."""
    dense = raw(2, 36, 64)
    assert dense.data_ptr() % 16 == 0 and dense.stride(1) % 16 == 0 and dense.stride(0) % 16 == 0
    assert check(camera, dense, "dense, aligned") == 12
    padded = raw(3, 36, 64, channels=4, row_pitch=64 * 4 + 5, offset=3)
    padded[..., :3] = dense
    assert padded.stride(1) % 2 == 1 and not padded.is_contiguous()
    assert check(camera, padded, "4 channels, odd pitch") == 12
    shifted = raw(4, 36, 64, offset=1)
    shifted.copy_(dense)
    assert shifted.data_ptr() % 16 == 1
    assert check(camera, shifted, "dense, misaligned base", scales=(2,)) == 4
    for order_in in ("rgb", "bgr"):
        a, b, c = (camera.camera_inputs(f, 2, 1, order_in, normalised=True) for f in (dense, padded, shifted))
        for k in ("image", "x"):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (order_in, k)


def test_wide_path_with_a_row_tail_and_odd_store_addresses(camera):
    """36 x 72 in rows of 224 bytes: the wide path with w = 36, four whole groups and a tail of four pixels per row; the image rows
    begin at odd multiples of four bytes, so whole groups take the byte stores there and the 8-byte stores elsewhere."""
    frames = raw(5, 36, 72, row_pitch=224)
    assert frames.data_ptr() % 16 == 0 and frames.stride(0) % 16 == 0
    assert check(camera, frames, "36 x 72, pitch 224", scales=(2, 4)) == 8


def test_planes_equal_the_batch_assembler(camera):
    from camradepth_amd.batch import assemble_batch
    frames = raw(6, 36, 64)
    for order_in in ("rgb", "bgr"):
        got = camera.camera_inputs(frames, 2, 2, order_in, normalised=True)
        h, w = got["image"].shape[1:3]
        zeros = torch.zeros(B, h, w, device="cuda")
        x = assemble_batch(got["image"], torch.zeros(B, h, w, 3, device="cuda"), zeros, zeros)["image"]
        assert x.shape == (B, 7, h, w)
        assert torch.equal(got["x"].view(torch.int32), x[:, :3].contiguous().view(torch.int32)), order_in


def test_out_no_allocation_and_capture(camera):
    """With out= the call is one launch: nothing is allocated, channels >= 3 of out['x'] are not touched, and a captured call replays
    onto new frame contents."""
    frames = raw(7, 36, 64)
    h, w = camera.map_shape((36, 64), 2, 2)
    out = {"image": torch.full((B, h, w, 3), SENTINEL, dtype=torch.uint8, device="cuda"),
           "x": torch.full((B, 7, h, w), float(SENTINEL), device="cuda")}

    def call():
        return camera.camera_inputs(frames, 2, 2, out=out)

    def verify(what):
        torch.cuda.synchronize()
        want = ref.camera_inputs(frames.cpu().numpy(), 2, 2, swap_rb=True)
        assert_bits(out["image"], want["image"], f"{what}: image")
        assert_bits(out["x"][:, :3].contiguous(), want["x"], f"{what}: x")
        assert (out["x"][:, 3:] == SENTINEL).all(), what

    res = call()                                                 # eager once: the code object is loaded before the capture
    assert set(res) == {"image", "x"} and all(res[k].data_ptr() == out[k].data_ptr() for k in out)
    verify("out=")
    only_x = camera.camera_inputs(frames, 2, 2, out={"x": out["x"]})
    assert set(only_x) == {"x"}
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    first = out["image"].clone()
    for seed in (8, 9):
        frames.copy_(raw(seed, 36, 64))
        out["image"].fill_(SENTINEL), out["x"][:, :3].fill_(float(SENTINEL))
        g.replay()
        verify(f"replay, frames of seed {seed}")
    assert not torch.equal(first, out["image"])


def test_wrong_inputs_are_refused(camera):
    from camradepth_amd import lib as L
    frames = raw(10, 36, 64)
    for bad in (frames.cpu(), frames.float(), frames[..., :2], frames[:, :, ::2], frames[0]):
        with pytest.raises(L.CrdError):
            camera.camera_inputs(bad, 2, 0)
    for kw in (dict(downsample_scale=3), dict(downsample_scale=5), dict(y_cutoff=18), dict(y_cutoff=-1), dict(order_in="gbr"),
               dict(order_out="argb"), dict(out={}), dict(out={"image": torch.empty(B, 18, 32, 3, device="cuda")}),
               dict(out={"x": torch.empty(B, 2, 18, 32, device="cuda")}), dict(normalised=True, out={"image": frames})):
        with pytest.raises(L.CrdError):
            camera.camera_inputs(frames, **dict(dict(downsample_scale=2, y_cutoff=0), **kw))
    with pytest.raises(L.CrdError):                              # 35 rows: 2 does not divide them
        camera.camera_inputs(frames[:, :35], 2, 0)
