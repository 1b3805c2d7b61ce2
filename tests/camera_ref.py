"""NumPy restatement of the camera front end (include/camradepth_hip.h, crd_camera_frontend): raw uint8 frames with byte pitches -> the
uint8 image [B,h,w,3] and the normalised fp32 planes [B,3,h,w].  Integer arithmetic up to the byte; the normalisation is
crd_assemble_input's expression, operation by operation in fp32.  tests/test_camera_ref_cpu.py holds it to scipy.ndimage.zoom."""
import numpy as np

F = np.float32
MEAN = np.array([0.485, 0.456, 0.406], dtype=F)
STD = np.array([0.229, 0.224, 0.225], dtype=F)


def frames_of(buf, B, H, W, channels, row_pitch, frame_pitch, offset=0):
    """The [B,H,W,channels] view of a flat uint8 buffer whose pixel (b, y, x) begins at offset + b * frame_pitch + y * row_pitch +
    x * channels -- the addressing of the C entry."""
    assert row_pitch >= W * channels and frame_pitch >= H * row_pitch
    return np.lib.stride_tricks.as_strided(buf[offset:], (B, H, W, channels), (frame_pitch, row_pitch, channels, 1), writeable=False)


def downsample(frames, s=2, y_cutoff=34, swap_rb=False):
    """frames uint8 [B,H,W,3 or 4] (any strides) -> uint8 [B,h,w,3], h = H / s - y_cutoff, w = W / s; s in 1 .. 4 divides H and W."""
    B, H, W, ch = frames.shape
    assert ch in (3, 4) and 1 <= s <= 4 and H % s == 0 and W % s == 0 and 0 <= y_cutoff < H // s
    p = frames[..., :3].astype(np.uint32)
    if swap_rb:
        p = p[..., ::-1]
    if s % 2:
        v = p[:, s // 2::s, s // 2::s]
    else:
        o = s // 2 - 1
        v = (p[:, o::s, o::s] + p[:, o::s, o + 1::s] + p[:, o + 1::s, o::s] + p[:, o + 1::s, o + 1::s]) >> 2
    return np.ascontiguousarray(v[:, y_cutoff:].astype(np.uint8))


def normalise(image):
    """uint8 [B,h,w,3] -> fp32 [B,3,h,w]: (v / 255 - mean[k]) / std[k] per stored channel k, every operation rounded to fp32."""
    v = image.astype(F) / F(255.0)
    return np.ascontiguousarray((((v - MEAN) / STD).astype(F)).transpose(0, 3, 1, 2))


def camera_inputs(frames, s=2, y_cutoff=34, swap_rb=False):
    image = downsample(frames, s, y_cutoff, swap_rb)
    return {"image": image, "x": normalise(image)}
