"""GPU visualisation back end: depth maps, label maps and the radar channel -> uint8 RGB pictures on the device.

What the reference's src/visualization/visualization.py:102-151 writes per sample through plt.imsave, cv2.imread, cv2.dilate and
cv2.addWeighted -- the jet-coloured depth (`colorize`), that depth blended over the camera image and the lidar ground truth pasted on
it (`overlay`), the segmentation in `rainbow` (`seg_labels`, `colorize_labels`), the dilated radar returns over the grey image
(`radar_overlay`) -- and a 2 x 3 collage of them (`Visualizer`), from buffers that are already on the device.  The arithmetic is
specified in include/camradepth_hip.h and restated by tests/viz_ref.py, bit for bit: INTEGRATION.md, "Visualisation back end".
Every output is RGB; writing a PNG stays with the caller.  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from ._frontend import _dev
from ._viz_tables import TABLES

TILE = 1024              # include/camradepth_hip.h: CRD_VIZ_TILE, pixels of one frame per workgroup of the range pass
FLOAT, LABELS = 0, 1     # CRD_VIZ_FLOAT, CRD_VIZ_LABELS
MODES = {None: 0, "paste": 1, "blend": 2, "image": 3}      # CRD_VIZ_NONE, _PASTE, _BLEND, _IMAGE
ORDERS = {"bgr": 1, "rgb": 0}
PANELS = ("depth_pred", "depth_on_rgb", "lidar_gt", "seg", "pred_seg", "radar", "unsup", "collage")

_tables = {}


def workspace_bytes(B, h, w):
    """include/camradepth_hip.h, crd_viz_range: one (min, max) pair of 8 bytes per tile of TILE pixels; tiles do not straddle frames."""
    return 8 * B * -(-(h * w) // TILE)


def table(cmap, device="cuda"):
    """The uint8 [256,3] colour table on `device`: 'jet' or 'rainbow' (copied there once and kept), or the caller's own cuda tensor.
    The first use of a built-in name on a device allocates and copies: VizWorkspace does it, outside a captured region."""
    if torch.is_tensor(cmap):
        return _dev(cmap, torch.uint8, (256, 3), "cmap")
    if not isinstance(cmap, str) or cmap not in TABLES:
        raise L.CrdError(f"cmap is one of {sorted(TABLES)} or a uint8 [256,3] cuda tensor, not {cmap!r}")
    key = (cmap, torch.device(device))
    if key not in _tables:
        _tables[key] = torch.frombuffer(bytearray(TABLES[cmap]), dtype=torch.uint8).view(256, 3).to(device)
    return _tables[key]


class VizWorkspace:
    """The scratch memory of this module for maps of up to B frames of h x w pixels: `partials` (workspace_bytes(B, h, w) bytes),
    `range` (fp32 [B,2]) and `dilated` (fp32 [B,h,w], the radar panel's map); the built-in tables are put on the device.  With
    workspace= and out= a call allocates nothing and does not wait for the device, so it can be captured in a graph on one stream."""

    def __init__(self, B, h, w, device="cuda"):
        if int(B) <= 0 or int(h) <= 0 or int(w) <= 0:
            raise L.CrdError(f"VizWorkspace: B {B}, map {h} x {w}")
        self.B, self.h, self.w = int(B), int(h), int(w)
        self.partials = torch.empty(workspace_bytes(self.B, self.h, self.w), dtype=torch.uint8, device=device)
        self.range = torch.empty(self.B, 2, device=device)
        self.dilated = torch.empty(self.B, self.h, self.w, device=device)
        for name in TABLES:
            table(name, self.partials.device)


def _map(x, what, labels=None):
    """A float map [B,h,w] or [B,1,h,w] (fp32) or a label map [B,h,w] (uint8) -> (tensor [B,h,w], kind).  labels: True / False insists
    on one kind, None takes either.  Type and shape are judged before the device, so a host tensor is told all that is wrong with it."""
    if not torch.is_tensor(x):
        raise L.CrdError(f"{what} must be a cuda tensor (no CPU fallback)")
    kinds = {torch.float32: FLOAT, torch.uint8: LABELS}
    if x.dtype not in kinds or (labels is not None and kinds[x.dtype] != (LABELS if labels else FLOAT)):
        wanted = "torch.float32 or torch.uint8" if labels is None else "torch.uint8" if labels else "torch.float32"
        raise L.CrdError(f"{what} must be {wanted}, not {x.dtype}")
    kind = kinds[x.dtype]
    if not (x.dim() == 3 or (kind == FLOAT and x.dim() == 4 and x.shape[1] == 1)) or x.numel() == 0:
        raise L.CrdError(f"{what} must have shape [B,h,w]{' or [B,1,h,w]' if kind == FLOAT else ''} with at least one pixel, not {list(x.shape)}")
    x = _dev(x, x.dtype, tuple(x.shape), what)
    return (x.view(x.shape[0], x.shape[2], x.shape[3]) if x.dim() == 4 else x), kind


def _scratch(fn, workspace, B, h, w, dev, dilated=False):
    """(partials, range, dilated or None) from the workspace, checked, or freshly allocated."""
    need = workspace_bytes(B, h, w)
    if workspace is None:
        return (torch.empty(need, dtype=torch.uint8, device=dev), torch.empty(B, 2, device=dev),
                torch.empty(B, h, w, device=dev) if dilated else None)
    if workspace.partials.numel() < need or workspace.range.shape[0] < B or (dilated and workspace.dilated.numel() < B * h * w):
        raise L.CrdError(f"{fn}: the workspace is sized for B {workspace.B}, map {workspace.h} x {workspace.w}; B {B}, map {h} x {w} needs "
                         f"{need} bytes of partials")
    return workspace.partials, workspace.range[:B], workspace.dilated.view(-1)[:B * h * w].view(B, h, w) if dilated else None


def _picture(fn, out, B, h, w, dev):
    """out=, or a new picture: uint8 [B,h,w,3] whose last two dimensions are dense; rows and frames may have any pitch that keeps them
    apart (a panel of a larger canvas)."""
    if out is None:
        return torch.empty(B, h, w, 3, dtype=torch.uint8, device=dev)
    if not (torch.is_tensor(out) and out.is_cuda):
        raise L.CrdError(f"{fn}: out must be a cuda tensor (no CPU fallback)")
    if out.dtype != torch.uint8 or tuple(out.shape) != (B, h, w, 3):
        raise L.CrdError(f"{fn}: out must be torch.uint8 {[B, h, w, 3]}, not {out.dtype} {list(out.shape)}")
    sb, sr, sc, s3 = out.stride()
    if s3 != 1 or (w > 1 and sc != 3) or (h > 1 and sr < 3 * w) or (B > 1 and sb < (h - 1) * sr + 3 * w):
        raise L.CrdError(f"{fn}: out has strides {out.stride()}: pixels must be dense within a row, rows and frames must not overlap")
    return out


def _pitches(out):
    B, h, w, _ = out.shape
    row = out.stride(1) if h > 1 else 3 * w
    return row, (out.stride(0) if B > 1 else h * row)


def _fixed(fn, vmin, vmax):
    """vmin / vmax of a call, checked -> (range tensor or None, vmin, vmax as floats or None): both None (the frames' own range), two
    finite numbers, or vmin an fp32 [B,2] cuda tensor of (vmin, vmax) rows with vmax None."""
    if torch.is_tensor(vmin) and vmax is None:
        return vmin, 0.0, 0.0
    if (vmin is None) != (vmax is None):
        raise L.CrdError(f"{fn}: pass both vmin and vmax or neither (vmin {vmin}, vmax {vmax})")
    if vmin is None:
        return None, None, None
    if torch.is_tensor(vmin) or torch.is_tensor(vmax):
        raise L.CrdError(f"{fn}: a range on the device is one fp32 [B,2] tensor passed as vmin=, with vmax=None")
    vmin, vmax = float(vmin), float(vmax)
    if not (math.isfinite(vmin) and math.isfinite(vmax)) or vmax < vmin:
        raise L.CrdError(f"{fn}: vmin {vmin}, vmax {vmax}: finite numbers with vmin <= vmax")
    return None, vmin, vmax


def _bad(fn, bad_colour):
    try:
        r, g, b = (int(v) for v in bad_colour)
    except (TypeError, ValueError):
        raise L.CrdError(f"{fn}: bad_colour is three integers 0 .. 255, not {bad_colour!r}") from None
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise L.CrdError(f"{fn}: bad_colour is three integers 0 .. 255, not {bad_colour!r}")
    return r | g << 8 | b << 16


def _range_into(fn, x, kind, dilate, workspace):
    """crd_viz_range -> (range [B,2], the dilated map or None)."""
    B, h, w = x.shape
    partials, rng, dilated = _scratch(fn, workspace, B, h, w, x.device, dilated=dilate != 0)
    L.check(L.load().crd_viz_range(L.ptr(x), kind, B, h, w, dilate, L.ptr(dilated), L.ptr(partials), partials.numel(), L.ptr(rng), L.stream()),
            "crd_viz_range")
    return rng, dilated


def _image(image, shape):
    if not (torch.is_tensor(image) and image.is_cuda):
        raise L.CrdError("image must be a cuda tensor (no CPU fallback)")
    return _dev(image, torch.uint8, tuple(shape) + (3,), "image")


def _draw(fn, x, kind, cmap, rng, vmin, vmax, bad, image, order, mode, alpha, beta, grey, out, shape=None):
    B, h, w = x.shape if x is not None else shape
    dev = x.device if x is not None else image.device
    if image is not None:
        image = _image(image, (B, h, w))
    tab = None if mode == "image" else table(cmap, dev)
    out = _picture(fn, out, B, h, w, dev)
    row, frame = _pitches(out)
    L.check(L.load().crd_viz_draw(L.ptr(x), kind, B, h, w, L.ptr(tab), L.ptr(rng), vmin or 0.0, vmax or 0.0, bad, L.ptr(image), ORDERS[order],
                                  MODES[mode], float(alpha), float(beta), 1 if grey else 0, L.ptr(out), row, frame, L.stream()), "crd_viz_draw")
    return out


def _colour(fn, x, labels, cmap, vmin, vmax, bad_colour, image, order, mode, alpha, beta, out, workspace):
    """What colorize, colorize_labels and overlay share: the arguments that are not tensors are judged first, then the map."""
    bad = _bad(fn, bad_colour)
    rng, vmin, vmax = _fixed(fn, vmin, vmax)
    if mode == "blend" and not (abs(float(alpha)) <= 1e30 and abs(float(beta)) <= 1e30):
        raise L.CrdError(f"{fn}: alpha {alpha}, beta {beta}")
    if order not in ORDERS:
        raise L.CrdError(f"{fn}: image_order is 'bgr' or 'rgb', not {order!r}")
    x, kind = _map(x, "labels" if labels else "x", labels)
    table(cmap, x.device)                                        # a wrong cmap, image or out is refused before anything is launched
    if image is not None:
        image = _image(image, x.shape)
    out = _picture(fn, out, *x.shape, x.device)
    if rng is not None:
        rng = _dev(rng, torch.float32, (x.shape[0], 2), "the range")
    elif vmin is None:
        rng, _ = _range_into(fn, x, kind, 0, workspace)
    return _draw(fn, x, kind, cmap, rng, vmin, vmax, bad, image, order, mode, alpha, beta, False, out)


def frame_range(x, out=None, workspace=None):
    """fp32 [B,2] on the device: (vmin, vmax) of every frame of a float map (its finite values; (0, 0) without one) or a label map --
    the reduction `colorize` runs, on its own, so that a caller can smooth a range over time and pass it back as vmin=.  out: the
    [B,2] tensor to write into."""
    x, kind = _map(x, "x")
    B, h, w = x.shape
    partials, rng, _ = _scratch("frame_range", workspace, B, h, w, x.device)
    if out is not None:
        rng = _dev(out, torch.float32, (B, 2), "out")
    L.check(L.load().crd_viz_range(L.ptr(x), kind, B, h, w, 0, None, L.ptr(partials), partials.numel(), L.ptr(rng), L.stream()), "crd_viz_range")
    return rng


def colorize(x, cmap="jet", vmin=None, vmax=None, bad_colour=(0, 0, 0), out=None, workspace=None):
    """A float map, fp32 [B,h,w] or [B,1,h,w], in the colours of cmap -> uint8 RGB [B,h,w,3]: plt.imsave(..., cmap=cmap) without the
    file (visualization.py:104,126).

    The range is each FRAME's own minimum and maximum unless it is fixed: vmin and vmax as two numbers, or vmin an fp32 [B,2] cuda
    tensor (frame_range's layout) -- for video a fixed range avoids flicker and needs no reduction.  A non-finite pixel is left out of
    the range and drawn in bad_colour; vmin == vmax paints table row 0.  cmap: 'jet', 'rainbow' or a uint8 [256,3] cuda tensor.  out:
    the picture to write into, possibly a view into a larger canvas (pixels dense within a row, any row and frame pitch).  With
    workspace= (a VizWorkspace) and out= nothing is allocated and nothing waits for the device."""
    return _colour("colorize", x, False, cmap, vmin, vmax, bad_colour, None, "rgb", None, 0.0, 0.0, out, workspace)


def colorize_labels(labels, cmap="rainbow", vmin=None, vmax=None, out=None, workspace=None):
    """A label map, uint8 [B,h,w] (seg_labels' output, or batch['seg'].to(torch.uint8)), in the colours of cmap -> uint8 RGB
    [B,h,w,3]: plt.imsave(..., cmap='rainbow') of integer labels (visualization.py:113,121), normalised in fp64 as matplotlib does for
    integers.  Range, cmap, out and workspace as for colorize."""
    return _colour("colorize_labels", labels, True, cmap, vmin, vmax, (0, 0, 0), None, "rgb", None, 0.0, 0.0, out, workspace)


def seg_labels(logits, out=None):
    """uint8 [B,h,w]: the first index of the maximum over the C <= 256 channels of logits (fp32 [B,C,h,w], `final_seg`); a NaN counts
    as larger than everything -- torch.max(logits, dim=1)[1] (visualization.py:120).  What colorize_labels and
    cloud.point_cloud(labels=) take."""
    logits = _dev(logits, torch.float32, (None, None, None, None), "logits")
    B, C, h, w = logits.shape
    if not 1 <= C <= 256 or logits.numel() == 0:
        raise L.CrdError(f"seg_labels: logits {list(logits.shape)}: 1 .. 256 classes and at least one pixel")
    out = torch.empty(B, h, w, dtype=torch.uint8, device=logits.device) if out is None else _dev(out, torch.uint8, (B, h, w), "out")
    L.check(L.load().crd_seg_labels(L.ptr(logits), B, C, h, w, L.ptr(out), L.stream()), "crd_seg_labels")
    return out


def overlay(image_u8, x, mode="paste", alpha=0.8, beta=0.75, cmap="jet", vmin=None, vmax=None, image_order="bgr", bad_colour=(0, 0, 0),
            out=None, workspace=None):
    """The colours of map x (a float map as for colorize, or a uint8 label map) over the camera image -> uint8 RGB [B,h,w,3].

    image_u8: uint8 [B,h,w,3] as assemble_batch takes it, in image_order 'bgr' ("as cv2 reads it") or 'rgb'.  mode 'paste': the
    colour where x > 0 and the image elsewhere, the range taken over the WHOLE map, zeros included -- the reference's lidar_gt
    picture (visualization.py:103-108).  mode 'blend': clamp(rint(image * alpha + colour * beta)) per channel in fp32 -- its
    depth_on_rgb (visualization.py:150, cv2.addWeighted(img, 0.8, colour, 0.75, 0)).  The rest as for colorize."""
    if mode not in ("paste", "blend"):
        raise L.CrdError(f"overlay: mode is 'paste' or 'blend', not {mode!r}")
    return _colour("overlay", x, None, cmap, vmin, vmax, bad_colour, image_u8, image_order, mode, alpha, beta, out, workspace)


def _dilate(fn, dilate):
    if isinstance(dilate, bool) or int(dilate) != dilate or not 1 <= int(dilate) <= 9 or int(dilate) % 2 == 0:
        raise L.CrdError(f"{fn}: dilate is an odd integer 1 .. 9, not {dilate}")
    return int(dilate)


def radar_overlay(image_u8, radar_depth, dilate=5, cmap="jet", image_order="bgr", out=None, workspace=None):
    """The reference's radar picture (visualization.py:130-141) -> uint8 RGB [B,h,w,3]: radar_depth (the network input's channel 3,
    fp32 [B,h,w] contiguous: x[:, 3].contiguous(), or radar_inputs' own map) becomes 1 - r at its returns, is dilated by a dilate x
    dilate maximum (odd, 1 .. 9), coloured over the per-frame range of the DILATED map and pasted where that is > 0 onto the grey
    image.  A return at r == 1 vanishes, as in the reference."""
    fn = "radar_overlay"
    dilate = _dilate(fn, dilate)
    r, _ = _map(radar_depth, "radar_depth", labels=False)
    table(cmap, r.device)
    if image_order not in ORDERS:
        raise L.CrdError(f"{fn}: image_order is 'bgr' or 'rgb', not {image_order!r}")
    B, h, w = r.shape
    image_u8 = _image(image_u8, (B, h, w))
    out = _picture(fn, out, B, h, w, r.device)
    rng, dilated = _range_into(fn, r, FLOAT, dilate, workspace)
    return _draw(fn, dilated, FLOAT, cmap, rng, None, None, 0, image_u8, image_order, "paste", 0.0, 0.0, True, out)


def image_rgb(image_u8, image_order="bgr", grey=False, out=None):
    """The camera image in R, G, B order (grey: its grey value in all three channels), written into out= -- a collage's first panel."""
    image_u8 = _image(image_u8, (None, None, None))
    return _draw("image_rgb", None, FLOAT, None, None, None, None, 0, image_u8, image_order, "image", 0.0, 0.0, grey, out,
                 shape=tuple(image_u8.shape[:3]))


class Visualizer:
    """The reference's pictures of a batch of B frames of h x w pixels, drawn into preallocated buffers: render() allocates nothing
    and does not wait for the device, so it can be captured in a graph behind InferenceGraph.run.

    `collage` is uint8 [B,2h,3w,3], a plain 2 x 3 tiling in the reference's panel order -- top: image, seg, pred_seg; bottom:
    depth_pred, lidar_gt, then unsup if the model has it, else depth_on_rgb -- and those pictures are VIEWS of it (missing ones stay
    black); 'radar', and 'depth_on_rgb' beside 'unsup', have buffers of their own.  The reference's collage is a matplotlib figure
    with axes and margins, which this does not reproduce."""

    def __init__(self, B, h, w, image_order="bgr", cmap_depth="jet", cmap_seg="rainbow", cmap_unsup="jet", dilate=5, alpha=0.8, beta=0.75,
                 device="cuda"):
        if image_order not in ORDERS:
            raise L.CrdError(f"Visualizer: image_order is 'bgr' or 'rgb', not {image_order!r}")
        self.ws = VizWorkspace(B, h, w, device)
        self.B, self.h, self.w, self.image_order = self.ws.B, self.ws.h, self.ws.w, image_order
        self.dilate, self.alpha, self.beta = _dilate("Visualizer", dilate), float(alpha), float(beta)
        dev = self.ws.partials.device
        self.cmaps = {k: table(v, dev) for k, v in (("depth", cmap_depth), ("seg", cmap_seg), ("unsup", cmap_unsup))}
        self.collage = torch.zeros(self.B, 2 * self.h, 3 * self.w, 3, dtype=torch.uint8, device=dev)
        self.radar = torch.empty(self.B, self.h, self.w, 3, dtype=torch.uint8, device=dev)
        self.blend = torch.empty(self.B, self.h, self.w, 3, dtype=torch.uint8, device=dev)
        self.radar_depth = torch.empty(self.B, self.h, self.w, device=dev)
        self.labels = torch.empty(self.B, self.h, self.w, dtype=torch.uint8, device=dev)

    def panel(self, i, j):
        """The view of the collage's panel in row i, column j."""
        return self.collage[:, i * self.h:(i + 1) * self.h, j * self.w:(j + 1) * self.w]

    def render(self, image_u8, x, pred, gt_full=None, seg=None):
        """image_u8: uint8 [B,h,w,3]; x: the network input [B,7,h,w] (channel 3 is the radar depth) or None for an RGB-only model;
        pred: the output dictionary of the model or of InferenceGraph.run; gt_full: the lidar ground truth, fp32 [B,h,w] or
        [B,1,h,w]; seg: the ground-truth labels, uint8 [B,h,w].  Returns the pictures, uint8 RGB, under the names of the reference's
        files: 'depth_pred', 'depth_on_rgb', 'lidar_gt' (with gt_full), 'seg' (with seg), 'pred_seg' and 'unsup' (if the model has
        those heads), 'radar' (with x), 'collage'.  They are this object's buffers: the next render() overwrites them."""
        ws, order = self.ws, self.image_order
        depth = pred["depth"]["final_depth"]
        logits, unsup = pred["seg"]["final_seg"], pred["seg"]["unsup_map"]
        out = {}
        image_rgb(image_u8, order, out=self.panel(0, 0))
        out["depth_pred"] = colorize(depth, self.cmaps["depth"], out=self.panel(1, 0), workspace=ws)
        # the range is still in the workspace: the blend colours the same map
        out["depth_on_rgb"] = overlay(image_u8, depth, "blend", self.alpha, self.beta, self.cmaps["depth"], vmin=ws.range, image_order=order,
                                      out=self.blend if unsup is not None else self.panel(1, 2), workspace=ws)
        if gt_full is not None:
            out["lidar_gt"] = overlay(image_u8, gt_full, "paste", cmap=self.cmaps["depth"], image_order=order, out=self.panel(1, 1), workspace=ws)
        if seg is not None:
            out["seg"] = colorize_labels(seg, self.cmaps["seg"], out=self.panel(0, 1), workspace=ws)
        if logits is not None:
            out["pred_seg"] = colorize_labels(seg_labels(logits, out=self.labels), self.cmaps["seg"], out=self.panel(0, 2), workspace=ws)
        if unsup is not None:
            out["unsup"] = colorize(unsup, self.cmaps["unsup"], out=self.panel(1, 2), workspace=ws)
        if x is not None:
            if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.shape[1] > 3):
                raise L.CrdError("Visualizer.render: x is the network input, a cuda tensor [B,C,h,w] with the radar depth in channel 3")
            self.radar_depth.copy_(x[:, 3])
            out["radar"] = radar_overlay(image_u8, self.radar_depth, self.dilate, self.cmaps["depth"], order, out=self.radar, workspace=ws)
        out["collage"] = self.collage
        return out
