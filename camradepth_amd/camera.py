"""GPU camera front end: raw camera frames -> the `image [B,h,w,3]` uint8 tensor assemble_batch takes, and optionally the normalised
image planes of the network input.

The reference makes its `_im` image offline, on the host in float64 (scripts/prepare_flow_im.py:18-26, downsample_im:
skimage.transform.resize(order=1, anti_aliasing=False) to half the size, astype('uint8'), the row cutoff).  Here one launch does it on
the device, bit for bit where downsample_scale divides the frame: INTEGRATION.md, "Camera front end".  Decoding the camera's JPEG stays
with the caller.  Nothing calls this module unless asked."""
import torch

from . import lib as L
from ._frontend import _dev, map_shape  # noqa: F401  (map_shape: the shape of the maps, re-exported)

ORDERS = ("rgb", "bgr")
SCALES = (1, 2, 3, 4)    # include/camradepth_hip.h, crd_camera_frontend: the factors for which the rule is skimage's


def _frames_arg(frames):
    """The raw frames, checked -> (B, H, W, channels, row pitch, frame pitch), pitches in bytes."""
    if not (torch.is_tensor(frames) and frames.is_cuda):
        raise L.CrdError("frames must be a cuda tensor (no CPU fallback)")
    if frames.dtype != torch.uint8:
        raise L.CrdError(f"frames must be torch.uint8, not {frames.dtype}")
    if frames.dim() != 4 or frames.shape[3] not in (3, 4) or frames.numel() == 0:
        raise L.CrdError(f"frames must have shape [B,H,W,3] or [B,H,W,4] with at least one pixel, not {list(frames.shape)}")
    B, H, W, ch = frames.shape
    sb, sr, sc, s1 = frames.stride()
    row = sr if H > 1 else W * ch
    frame = sb if B > 1 else H * row
    if s1 != 1 or (W > 1 and sc != ch) or row < W * ch or frame < H * row:
        raise L.CrdError(f"frames has strides {frames.stride()}: the channels and pixels of a row must be dense, rows and frames must "
                         "not overlap")
    return B, H, W, ch, row, frame


def camera_inputs(frames, downsample_scale=2, y_cutoff=34, order_in="rgb", order_out="bgr", normalised=False, out=None):
    """Raw frames -> {'image': uint8 [B,h,w,3]} with (h, w) = map_shape((H, W), downsample_scale, y_cutoff) (crd_camera_frontend).

    frames: uint8 cuda tensor [B,H,W,3] or [B,H,W,4] (a fourth byte is ignored) whose innermost two strides are dense; the row and
    frame strides are taken from the tensor, so a cropped or padded view needs no .contiguous().  downsample_scale 1 .. 4 must divide H
    and W.  order_in: the channel order of frames, 'rgb' (skimage.io.imread, most decoders) or 'bgr'; order_out: that of the result,
    'bgr' being what the network was trained on (cv2.imread).  normalised=True also returns 'x', fp32 [B,3,h,w]: the image planes of
    the network input, the bits assemble_batch makes from 'image'.  out: a dictionary with 'image', 'x' or both to write into -- 'x'
    fp32 [B,C,h,w] with C >= 3, of which channels 0 .. 2 are written (a plan's input buffer); exactly the tensors given are made and
    returned, nothing is allocated and nothing waits for the device, so the call can be captured in a graph on one stream."""
    fn = "camera_inputs"
    if order_in not in ORDERS or order_out not in ORDERS:
        raise L.CrdError(f"{fn}: order_in and order_out are 'rgb' or 'bgr', not {order_in!r} and {order_out!r}")
    if isinstance(downsample_scale, bool) or int(downsample_scale) != downsample_scale or int(downsample_scale) not in SCALES:
        raise L.CrdError(f"{fn}: downsample_scale is one of {SCALES}, not {downsample_scale}")
    s = int(downsample_scale)
    B, H, W, ch, row, frame = _frames_arg(frames)
    h, w = map_shape((H, W), s, y_cutoff)
    if H % s or W % s:
        raise L.CrdError(f"{fn}: downsample_scale {s} does not divide the frame {H} x {W} (the resize is then no plain average)")
    dev = frames.device
    if out is None:
        out = {"image": torch.empty(B, h, w, 3, dtype=torch.uint8, device=dev)}
        if normalised:
            out["x"] = torch.empty(B, 3, h, w, device=dev)
    else:
        if not isinstance(out, dict) or not set(out) <= {"image", "x"} or not out:
            raise L.CrdError(f"{fn}: out= is a dictionary that holds 'image', 'x' or both")
        if normalised and "x" not in out:
            raise L.CrdError(f"{fn}: normalised=True without out['x']")
        out = dict(out)
        if "image" in out:
            out["image"] = _dev(out["image"], torch.uint8, (B, h, w, 3), "out['image']")
        if "x" in out:
            out["x"] = _dev(out["x"], torch.float32, (B, None, h, w), "out['x']")
            if out["x"].shape[1] < 3:
                raise L.CrdError(f"{fn}: out['x'] has {out['x'].shape[1]} channels, the image takes three")
    x = out.get("x")
    L.check(L.load().crd_camera_frontend(L.ptr(frames), B, H, W, ch, row, frame, 1 if order_in != order_out else 0, s, int(y_cutoff),
                                         L.ptr(out.get("image")), L.ptr(x), x.shape[1] if x is not None else 0, L.stream()),
            "crd_camera_frontend")
    return out
