"""GPU point-cloud back end: a depth map -> 3-D points in metres in the caller's frame.

The other end of the network from the radar and lidar front ends: `final_depth` of CamRaDepth.forward / InferenceGraph.run (normalised
inverse depth, `encoding="inverse"`) or a metres map of the front ends (`encoding="metres"`) goes in, an organised cloud
(`unproject_depth`) or a compact one in (b, r, c) order (`point_cloud`) comes out.  The pixel-centre convention, K, the row cutoff and
the `frame_offsets` layout are the rasterisers', so a cloud can be fed straight back into project_radar / project_lidar.  All
arithmetic is fp64 on the device, specified operation by operation in include/camradepth_hip.h: INTEGRATION.md, "Point-cloud back
end".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from ._frontend import _dev, _intrinsics, _size, map_shape

TILE = 1024              # include/camradepth_hip.h: CRD_CLOUD_TILE, candidates per workgroup of the compact path
ENCODINGS = {"inverse": 0, "metres": 1}
OPTIONAL = ("rgb", "label", "pixel")


def candidates(h, w, stride=1):
    """Candidate pixels of one frame: those with r % stride == 0 and c % stride == 0."""
    return -(-h // stride) * -(-w // stride)


def workspace_bytes(B, h, w, stride=1):
    """include/camradepth_hip.h, crd_point_cloud: one int32 per tile of TILE candidates; tiles do not straddle frames."""
    return 4 * B * -(-candidates(h, w, stride) // TILE)


def keep_table(ids, device="cuda"):
    """The uint8 [256] table of point_cloud(keep=) from a collection of the class ids to keep.  It allocates and copies: build it
    once, outside a captured region."""
    ids = sorted({int(i) for i in ids})
    if ids and not 0 <= ids[0] <= ids[-1] <= 255:
        raise L.CrdError(f"keep: class ids are 0 .. 255, not {ids[0]} .. {ids[-1]}")
    table = torch.zeros(256, dtype=torch.uint8)
    table[ids] = 1
    return table.to(device)


def _stride(stride):
    if int(stride) != stride or int(stride) < 1:
        raise L.CrdError(f"stride must be an integer >= 1, not {stride}")
    return int(stride)


class CloudWorkspace:
    """The scratch memory of point_cloud and its preallocated outputs for batches of B frames, sized for the y_cutoff and stride given
    (a larger y_cutoff or stride fits too).  `out` is the dictionary point_cloud(out=) takes for a call without image, labels and
    with_pixel; `outputs(rgb=, label=, pixel=)` adds the buffers of those.  With workspace= and out= a call allocates nothing, so it
    can be captured in a graph on one stream."""

    def __init__(self, B, image_size=(900, 1600), downsample_scale=2, y_cutoff=0, stride=1, device="cuda"):
        h, w = map_shape(image_size, downsample_scale, y_cutoff)
        if int(B) <= 0:
            raise L.CrdError(f"CloudWorkspace: B = {B}")
        self.B, self.image_size, self.downsample_scale, self.stride = int(B), _size(image_size), int(downsample_scale), _stride(stride)
        self.cap = self.B * candidates(h, w, self.stride)
        self.tiles = torch.empty(workspace_bytes(self.B, h, w, self.stride), dtype=torch.uint8, device=device)
        self.xyz = torch.empty(self.cap, 3, device=device)
        self.frame_offsets = torch.empty(self.B + 1, dtype=torch.int32, device=device)
        self.rgb = torch.empty(self.cap, 3, dtype=torch.uint8, device=device)
        self.label = torch.empty(self.cap, dtype=torch.uint8, device=device)
        self.pixel = torch.empty(self.cap, dtype=torch.int32, device=device)

    def outputs(self, rgb=False, label=False, pixel=False):
        out = {"xyz": self.xyz, "frame_offsets": self.frame_offsets}
        out.update({k: getattr(self, k) for k, on in zip(OPTIONAL, (rgb, label, pixel)) if on})
        return out

    @property
    def out(self):
        return self.outputs()


def _given(out, keys, fn):
    """The tensors of out= under `keys`, or CrdError when it is no dictionary that holds them all."""
    if not isinstance(out, dict) or any(k not in out for k in keys):
        raise L.CrdError(f"{fn}: out= is a dictionary that holds {list(keys)}")
    return [out[k] for k in keys]


def _common(fn, depth, K, image_size, downsample_scale, y_cutoff, max_depth, encoding, out_from_cam, min_range, max_range, skip_empty,
            mask, labels, keep):
    """The checked tensors and the leading arguments crd_depth_unproject and crd_point_cloud share."""
    if encoding not in ENCODINGS:
        raise L.CrdError(f"{fn}: encoding is 'inverse' or 'metres', not {encoding!r}")
    h, w = map_shape(image_size, downsample_scale, y_cutoff)
    if torch.is_tensor(depth) and depth.dim() == 4:
        depth = _dev(depth, torch.float32, (None, 1, h, w), "depth")
        depth = depth.view(depth.shape[0], h, w)
    depth = _dev(depth, torch.float32, (None, h, w), "depth")
    B = depth.shape[0]
    if B == 0:
        raise L.CrdError(f"{fn}: depth holds no frame")
    K, k_stride = _intrinsics(K, B)
    T, t_stride = None, 0
    if out_from_cam is not None:
        per_frame = torch.is_tensor(out_from_cam) and out_from_cam.dim() == 3
        T = _dev(out_from_cam, torch.float64, (B, 3, 4) if per_frame else (3, 4), "out_from_cam")
        t_stride = 12 if per_frame else 0
    if not float(max_depth) > 0.0 or math.isinf(float(max_depth)) or math.isnan(float(min_range)) or math.isnan(float(max_range)):
        raise L.CrdError(f"{fn}: max_depth {max_depth}, min_range {min_range}, max_range {max_range}")
    if mask is not None:
        mask = _dev(mask, torch.uint8, (B, h, w), "mask")
    if labels is not None:
        if keep is None:
            raise L.CrdError(f"{fn}: labels without keep (the classes to keep: a uint8 [256] cuda table or a collection of ids)")
        labels = _dev(labels, torch.uint8, (B, h, w), "labels")
        keep = _dev(keep, torch.uint8, (256,), "keep") if torch.is_tensor(keep) else keep_table(keep, depth.device)
    elif keep is not None:
        raise L.CrdError(f"{fn}: keep without labels")
    im_h, im_w = _size(image_size)
    lead = (L.ptr(depth), B, im_h, im_w, int(downsample_scale), int(y_cutoff), L.ptr(K), k_stride, L.ptr(T), t_stride, ENCODINGS[encoding],
            L.f64_bits(max_depth), L.f64_bits(min_range), L.f64_bits(max_range), 1 if skip_empty else 0, L.ptr(mask), L.ptr(labels),
            L.ptr(keep))
    return lead, (depth, K, T, mask, labels, keep), B, h, w


def unproject_depth(depth, K, image_size=(900, 1600), downsample_scale=2, y_cutoff=34, max_depth=100.0, encoding="inverse",
                    out_from_cam=None, min_range=0.0, max_range=math.inf, skip_empty=False, mask=None, labels=None, keep=None, out=None):
    """The organised cloud (crd_depth_unproject): every pixel of a depth map to its 3-D point.

    depth [B,h,w] or [B,1,h,w] fp32 with (h, w) = map_shape(image_size, downsample_scale, y_cutoff); encoding 'inverse': normalised
    inverse depth, d = max_depth * (1 - p) -- the network's output, where p = 0 is max_depth metres, and gt_full, where 0 is "no ground
    truth" (skip_empty=True drops it); 'metres': d = p.  K [3,3] or [B,3,3] fp64; out_from_cam [3,4] or [B,3,4] fp64 moves the camera-
    frame point (X, Y, Z = d) into the caller's frame.  A pixel is valid when p is finite, d > 0, min_range <= d <= max_range, mask
    ([B,h,w] uint8) is non-zero and keep (a uint8 [256] cuda table, or a collection of class ids) holds its labels ([B,h,w] uint8)
    value.  Returns {'points': [B,h,w,3] fp32, 'valid': [B,h,w] uint8}; an invalid pixel is (0, 0, 0) and 0.  out: a dictionary of the
    two tensors to write into."""
    lead, held, B, h, w = _common("unproject_depth", depth, K, image_size, downsample_scale, y_cutoff, max_depth, encoding, out_from_cam,
                                  min_range, max_range, skip_empty, mask, labels, keep)
    dev = held[0].device
    if out is None:
        out = {"points": torch.empty(B, h, w, 3, device=dev), "valid": torch.empty(B, h, w, dtype=torch.uint8, device=dev)}
    else:
        points, valid = _given(out, ("points", "valid"), "unproject_depth")
        out = {"points": _dev(points, torch.float32, (B, h, w, 3), "out['points']"), "valid": _dev(valid, torch.uint8, (B, h, w), "out['valid']")}
    L.check(L.load().crd_depth_unproject(*lead, L.ptr(out["points"]), L.ptr(out["valid"]), L.stream()), "crd_depth_unproject")
    return out


def point_cloud(depth, K, image_size=(900, 1600), downsample_scale=2, y_cutoff=34, max_depth=100.0, encoding="inverse", out_from_cam=None,
                min_range=0.0, max_range=math.inf, skip_empty=False, mask=None, labels=None, keep=None, stride=1, image=None,
                with_pixel=False, workspace=None, out=None):
    """The compact cloud (crd_point_cloud): the valid pixels of unproject_depth among those with r % stride == 0 and c % stride == 0,
    written densely in (b, r, c) order, the same bits every run.

    Returns {'xyz': [cap,3] fp32, 'frame_offsets': [B+1] int32} with cap = B * ceil(h / stride) * ceil(w / stride); frame b owns the rows
    frame_offsets[b] .. frame_offsets[b+1] - 1 and frame_offsets[B] is the number of points -- the tensor project_radar and
    project_lidar take.  Rows from frame_offsets[B] on are left untouched.  With image ([B,h,w,3] uint8, as assemble_batch takes it)
    also 'rgb' [cap,3] uint8, with labels 'label' [cap] uint8, with with_pixel 'pixel' [cap] int32 = r * w + c.  workspace: a
    CloudWorkspace; out: a dictionary of exactly the tensors the call returns, each with at least cap rows (CloudWorkspace.out /
    .outputs(...)): then nothing is allocated and nothing waits for the device."""
    fn = "point_cloud"
    stride = _stride(stride)
    lead, held, B, h, w = _common(fn, depth, K, image_size, downsample_scale, y_cutoff, max_depth, encoding, out_from_cam, min_range,
                                  max_range, skip_empty, mask, labels, keep)
    dev = held[0].device
    if image is not None:
        image = _dev(image, torch.uint8, (B, h, w, 3), "image")
    cap = B * candidates(h, w, stride)
    need = workspace_bytes(B, h, w, stride)
    if workspace is None:
        tiles = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        tiles = workspace.tiles
        if tiles.numel() < need:
            raise L.CrdError(f"{fn}: the workspace holds {tiles.numel()} bytes, {need} are needed (B {B}, map {h} x {w}, stride {stride})")
    wanted = {"rgb": image is not None, "label": labels is not None, "pixel": bool(with_pixel)}
    shapes = {"xyz": (torch.float32, (None, 3)), "frame_offsets": (torch.int32, (B + 1,)), "rgb": (torch.uint8, (None, 3)),
              "label": (torch.uint8, (None,)), "pixel": (torch.int32, (None,))}
    if out is None:
        out = {"xyz": torch.empty(cap, 3, device=dev), "frame_offsets": torch.empty(B + 1, dtype=torch.int32, device=dev)}
        out.update({k: torch.empty((cap,) + shapes[k][1][1:], dtype=shapes[k][0], device=dev) for k in OPTIONAL if wanted[k]})
    else:
        _given(out, ("xyz", "frame_offsets"), fn)
        for k, what in (("rgb", "image"), ("label", "labels"), ("pixel", "with_pixel")):
            if (k in out) != wanted[k]:
                raise L.CrdError(f"{fn}: out['{k}'] without {what}" if k in out else f"{fn}: {what} without out['{k}']")
        out = {k: _dev(out[k], *shapes[k], f"out['{k}']") for k in ("xyz", "frame_offsets") + tuple(k for k in OPTIONAL if wanted[k])}
        for k in out:
            if k != "frame_offsets" and out[k].shape[0] < cap:
                raise L.CrdError(f"{fn}: out['{k}'] holds {out[k].shape[0]} rows, {cap} are needed")
    L.check(L.load().crd_point_cloud(*lead, stride, L.ptr(image), L.ptr(tiles), tiles.numel(), L.ptr(out["xyz"]), L.ptr(out.get("rgb")),
                                     L.ptr(out.get("label")), L.ptr(out.get("pixel")), L.ptr(out["frame_offsets"]), L.stream()),
            "crd_point_cloud")
    return out
