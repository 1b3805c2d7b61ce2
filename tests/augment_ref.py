"""numpy restatement of the batch augmentation (include/camradepth_hip.h, "Batch augmentation on the device"): the draw of
crd_augment_draw, the image table of crd_augment_lut and the gather of crd_augment_assemble / crd_augment_gather, shared by
test_augment_ref_cpu.py and test_gpu_augment.py.

The draw uses the generator of crd_dropout_masks (tests/dropout_ref.py) on a stream of its own: the seed is
rank_seed(seed, rank) ^ AUG_STREAM.  Element i = b * 8 + k of the draw (seed, counter) has t = hash >> 40 and u = t * 2^-24;
    k = 0, 1   y0 = (t * (H - h + 1)) >> 24,  x0 = (t * (W - w + 1)) >> 24          integers only
    k = 2      flip = u < p                                                          p as float32
    k = 3..7   gamma, brightness, colour[0..2] = lo + u * (hi - lo)                  fp32, each operation rounded; 1.0 when switched off
so the integer words can be compared exactly and the float words to the last bit on a device that does not contract the sum.
The table is computed in float64 and rounded to fp32 once: it is the yardstick for the device's fp32 chain, not its copy."""
import numpy as np

from tests.dropout_ref import EPOCH_MUL, M64, mix_int, rank_seed, uniforms

AUG_STREAM = 0xA0761D6478BD642F         # include/camradepth_hip.h: CRD_AUGMENT_STREAM
WORDS = 8
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)          # the constants of k_assemble_input, as fp32
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def stream_seed(seed, rank=0):
    return rank_seed(seed, rank) ^ AUG_STREAM


def top24(i, seed, rank, counter):
    """t of element i, one Python integer at a time: the scalar restatement of what `uniforms` does on arrays."""
    base = mix_int(stream_seed(seed, rank) ^ ((int(counter) * EPOCH_MUL) & M64))
    return mix_int((base + i) & M64) >> 40


def draw(B, H, W, h, w, p=0.0, gamma=None, brightness=None, colour=None, seed=0, rank=0, counter=0):
    """-> int32 [B, 8]: words 3..7 hold fp32 bit patterns (view them with floats())."""
    u = uniforms(B * WORDS, stream_seed(seed, rank), counter).reshape(B, WORDS)
    t = (u * np.float32(2.0 ** 24)).astype(np.int64)                       # exact: u is a multiple of 2^-24 below 1
    out = np.empty((B, WORDS), dtype=np.int32)
    out[:, 0] = (t[:, 0] * (H - h + 1)) >> 24
    out[:, 1] = (t[:, 1] * (W - w + 1)) >> 24
    out[:, 2] = u[:, 2] < np.float32(p)
    f = np.ones((B, 5), dtype=np.float32)
    for cols, rng in ((slice(0, 1), gamma), (slice(1, 2), brightness), (slice(2, 5), colour)):
        if rng is not None:
            lo, hi = np.float32(rng[0]), np.float32(rng[1])
            f[:, cols] = lo + u[:, 3:][:, cols] * (hi - lo)                # float32 throughout
    out[:, 3:] = f.view(np.int32)
    return out


def floats(params):
    """Words 3..7 of a table as float32 [B, 5]."""
    return np.ascontiguousarray(params[:, 3:]).view(np.float32)


def lut(params, gamma=True, brightness=True, colour=True):
    """float32 [B, 3, 256] from a table (the device's or the restatement's); the flags say which transforms are enabled."""
    f = floats(params).astype(np.float64)
    v = np.arange(256, dtype=np.float64) / 255.0
    out = np.empty((params.shape[0], 3, 256), dtype=np.float64)
    for b in range(params.shape[0]):
        t = v.copy()
        if gamma:
            t = np.power(t, f[b, 0])
        if brightness:
            t = t * f[b, 1]
        for c in range(3):
            tc = t * f[b, 2 + c] if colour else t
            out[b, c] = (np.clip(tc, 0.0, 1.0) - np.float64(MEAN[c])) / np.float64(STD[c])
    return out.astype(np.float32)


def gather(src, params, h, w):
    """src [B, ..., H, W] -> [B, ..., h, w]: out[b, ..., y, x] = src[b, ..., y0 + y, x0 + (flip ? w - 1 - x : x)]."""
    out = np.empty(src.shape[:-2] + (h, w), dtype=src.dtype)
    for b in range(src.shape[0]):
        y0, x0, flip = (int(v) for v in params[b, :3])
        win = src[b, ..., y0:y0 + h, x0:x0 + w]
        out[b] = win[..., ::-1] if flip else win
    return out


def mirror_u(image, params):
    """Channel 4 of flipped samples: v == 0 ? 0 : -v (in place on a gathered [B, C >= 6, h, w] image)."""
    for b in range(image.shape[0]):
        if params[b, 2]:
            v = image[b, 4]
            image[b, 4] = np.where(v == 0, np.float32(0.0), -v)
    return image


def inverse_depth(depth, max_depth):
    """dataloader.py:241-247 in float32, as k_gt_inverse writes it: g = clip(d, 0, max); g > 0 -> (max - g) * (1 / max)."""
    md = np.float32(max_depth)
    g = np.clip(depth.astype(np.float32), np.float32(0), md)
    return np.where(g > 0, (md - g) * (np.float32(1.0) / md), g).astype(np.float32)


def assemble(img_u8, radar, rad_vel, depth, seg_u8, params, table, h, w, max_depth=100.0):
    """The fused assembly given the image table -> dict(image, gt_full[, final_seg, intermediate_seg]) of numpy arrays.
    img_u8 [B,H,W,3] uint8, radar [B,H,W,3], rad_vel [B,H,W] or None, depth [B,H,W] metres, seg_u8 [B,H,W] uint8 or None."""
    B = img_u8.shape[0]
    md = np.float32(max_depth)
    byte = gather(np.ascontiguousarray(img_u8.transpose(0, 3, 1, 2)), params, h, w)                 # [B,3,h,w]
    planes = [np.take_along_axis(table, byte.reshape(B, 3, -1).astype(np.int64), axis=2).reshape(B, 3, h, w)]
    rad = gather(np.ascontiguousarray(radar.transpose(0, 3, 1, 2)).astype(np.float32), params, h, w)
    planes.append(np.clip(rad[:, 0:1], np.float32(0), md) / md)
    planes.append(rad[:, 1:3])
    if rad_vel is not None:
        planes.append(gather(rad_vel[:, None].astype(np.float32), params, h, w))
    out = {"image": mirror_u(np.concatenate(planes, axis=1).astype(np.float32), params),
           "gt_full": gather(inverse_depth(depth, max_depth)[:, None], params, h, w)}
    if seg_u8 is not None:
        out["final_seg"] = gather(seg_u8.astype(np.int64), params, h, w)
        out["intermediate_seg"] = intermediate_seg(out["final_seg"])
    return out


def intermediate_seg(final):
    """seg_targets' rule at a halving: skimage order 0 reads source index 2 o + 1."""
    return np.ascontiguousarray(final[:, 1::2, 1::2][:, :final.shape[1] // 2, :final.shape[2] // 2])


def min_pool(t):
    """Zero-ignoring 3x3 / stride 2 / pad 1 min-pool of a float32 [B,1,H,W] array (dataloader.py:213-222), written out."""
    B, _, H, W = t.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    big = np.where(t == 0, np.float32(255), t).astype(np.float32)
    pad = np.full((B, 1, H + 2, W + 2), np.float32(255))
    pad[:, :, 1:-1, 1:-1] = big
    out = np.full((B, 1, OH, OW), np.float32(255))
    for ky in range(3):
        for kx in range(3):
            out = np.minimum(out, pad[:, :, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2][:, :, :OH, :OW])
    return np.where(out == 255, np.float32(0), out).astype(np.float32)


def pyramid(full, levels=3):
    out, cur = [], full
    for _ in range(levels):
        cur = min_pool(cur)
        out.append(cur)
    return out
