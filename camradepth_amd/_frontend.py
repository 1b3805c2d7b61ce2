"""What the radar and lidar front ends and the point-cloud back end share on the Python side: the argument checks, the geometry of the
maps, the workspace of the z-buffer rasteriser and the checks of a rasterising call (radar.py, lidar.py, cloud.py), and the three forms
of a point cloud that the back ends behind it take (bev.py, occupancy.py)."""
import torch

from . import lib as L


def _dev(t, dtype, shape, what):
    """A contiguous cuda tensor of the dtype and shape given (None in `shape`: any extent), or CrdError."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.CrdError(f"{what} must be a cuda tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise L.CrdError(f"{what} must be {dtype}, not {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and s != n for s, n in zip(shape, t.shape)):
        raise L.CrdError(f"{what} must have shape {list(shape)}, not {list(t.shape)}")
    if not t.is_contiguous():
        raise L.CrdError(f"{what} must be contiguous")
    return t


def _frames(frame_offsets):
    off = _dev(frame_offsets, torch.int32, (None,), "frame_offsets")
    if off.shape[0] < 2:
        raise L.CrdError("frame_offsets must hold B + 1 >= 2 entries")
    return off, off.shape[0] - 1


def _rows(fn, cloud, frame_offsets, valid, labels):
    """-> (xyz [n,3], valid, labels, frame_offsets or None, rows_per_frame, B) from one of the three forms of the first argument."""
    if isinstance(cloud, dict):
        if frame_offsets is not None:
            raise L.CrdError(f"{fn}: a cloud dictionary brings its own frames; frame_offsets= goes with a bare [n,3] tensor")
        if "xyz" in cloud and "frame_offsets" in cloud:                       # point_cloud's
            xyz = _dev(cloud["xyz"], torch.float32, (None, 3), "cloud['xyz']")
            off, B = _frames(cloud["frame_offsets"])
            labels = cloud.get("label") if labels is None else labels
            return xyz, valid, labels, off, 0, B
        if "points" in cloud and "valid" in cloud:                            # unproject_depth's
            pts = _dev(cloud["points"], torch.float32, (None, None, None, 3), "cloud['points']")
            B, h, w, _ = pts.shape
            if B * h * w == 0:
                raise L.CrdError(f"{fn}: cloud['points'] holds no pixel")
            if valid is not None:
                raise L.CrdError(f"{fn}: an organised cloud brings its own valid")
            own = _dev(cloud["valid"], torch.uint8, (B, h, w), "cloud['valid']")
            if labels is not None:
                labels = _dev(labels, torch.uint8, (B, h, w), "labels").view(-1)          # the label map the cloud was made with
            return pts.view(-1, 3), own.view(-1), labels, None, h * w, B
        raise L.CrdError(f"{fn}: a cloud dictionary holds 'xyz' and 'frame_offsets' (point_cloud) or 'points' and 'valid' (unproject_depth)")
    xyz = _dev(cloud, torch.float32, (None, 3), "xyz")
    if frame_offsets is None:
        raise L.CrdError(f"{fn}: a bare xyz tensor needs frame_offsets (int32 [B+1] on the device)")
    off, B = _frames(frame_offsets)
    return xyz, valid, labels, off, 0, B


def _intrinsics(K, B):
    """-> (K, k_stride): one 3x3 matrix for every frame, or one per frame."""
    if torch.is_tensor(K) and K.dim() == 3:
        return _dev(K, torch.float64, (B, 3, 3), "K"), 9
    return _dev(K, torch.float64, (3, 3), "K"), 0


def _size(image_size):
    h, w = (int(v) for v in image_size)
    return h, w


def map_shape(image_size=(900, 1600), downsample_scale=2, y_cutoff=34):
    """(rows, columns) of the maps the rasterisers write and the point-cloud back end reads."""
    h, w = _size(image_size)
    s = int(downsample_scale)
    if s <= 0 or h // s <= 0 or w // s <= 0 or not 0 <= int(y_cutoff) < h // s:
        raise L.CrdError(f"maps: image {h} x {w}, downsample_scale {downsample_scale}, y_cutoff {y_cutoff} leave no pixel")
    return h // s - int(y_cutoff), w // s


class RasterWorkspace:
    """The scratch memory of a rasterising front end for batches of up to B frames: `keys`, key_bytes(pixels) bytes for the per-pixel key
    images (sized for y_cutoff = 0, so any cutoff fits), and, with max_points given, the projection's outputs for up to that many
    points.  A subclass names them in GROUPS: (attribute, dtype, keys) for a [len(keys), max_points] buffer whose rows proj_out hands out
    under those keys; keys None: one [max_points] buffer under the attribute's own name."""
    GROUPS = ()

    def __init__(self, B, image_size, downsample_scale, max_points, key_bytes, device):
        h, w = map_shape(image_size, downsample_scale, 0)
        if int(B) <= 0:
            raise L.CrdError(f"{type(self).__name__}: B = {B}")
        self.B, self.image_size, self.downsample_scale = int(B), _size(image_size), int(downsample_scale)
        self.keys = torch.empty(key_bytes(self.B * h * w), dtype=torch.uint8, device=device)
        self.max_points = None if max_points is None else int(max_points)
        if self.max_points is not None:
            for attr, dtype, keys in self.GROUPS:
                shape = (self.max_points,) if keys is None else (len(keys), self.max_points)
                setattr(self, attr, torch.empty(shape, dtype=dtype, device=device))

    def proj_out(self, n):
        """The projection buffers for n points, as the projection's out= takes them."""
        if self.max_points is None or n > self.max_points:
            raise L.CrdError(f"{type(self).__name__}: no room for the projection of {n} points (max_points = {self.max_points})")
        out = {}
        for attr, _, keys in self.GROUPS:
            buf = getattr(self, attr)
            out.update({attr: buf[:n]} if keys is None else {k: buf[i, :n] for i, k in enumerate(keys)})
        return out


def raster_args(fn, proj, frame_offsets, K, image_size, downsample_scale, y_cutoff, f64_keys, u8_keys, workspace, need_of, out, out_spec,
                detail=""):
    """The checks rasterize_radar and lidar_ground_truth share, under the caller's name fn.

    proj holds fp64 [N] tensors under f64_keys, uint8 [N] tensors under u8_keys and perhaps 'valid'; need_of(n_pix) is the caller's
    workspace need in bytes (detail: what else it depends on, for the refusal of a workspace too small); out_spec maps each output's
    name to (dtype, trailing shape) behind [B, h, w].  -> (head, keys, out, B, h, w): the leading arguments of crd_radar_rasterize and
    crd_lidar_ground_truth up to y_cutoff, the byte buffer of the key images, the dictionary of outputs and the shape of the maps."""
    h, w = map_shape(image_size, downsample_scale, y_cutoff)
    off, B = _frames(frame_offsets)
    if not all(k in proj for k in f64_keys + u8_keys):
        raise L.CrdError(f"{fn}: proj needs {f64_keys + u8_keys}")
    first = proj[f64_keys[0]]
    N = first.shape[0] if torch.is_tensor(first) and first.dim() == 1 else None
    points = [_dev(proj[k], torch.float64, (N,), f"proj['{k}']") for k in f64_keys] + \
             [_dev(proj[k], torch.uint8, (N,), f"proj['{k}']") for k in u8_keys]
    valid = proj.get("valid")
    if valid is not None:
        valid = _dev(valid, torch.uint8, (N,), "proj['valid']")
    K, k_stride = _intrinsics(K, B)
    im_h, im_w = _size(image_size)
    dev = points[0].device
    need = need_of(B * h * w)
    if workspace is None:
        keys = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        keys = workspace.keys
        if keys.numel() < need:
            raise L.CrdError(f"{fn}: the workspace holds {keys.numel()} bytes, {need} are needed "
                             f"(B {B}, image {im_h} x {im_w}, downsample_scale {downsample_scale}{detail})")
    if out is None:
        out = {k: torch.empty((B, h, w) + tail, dtype=dtype, device=dev) for k, (dtype, tail) in out_spec.items()}
    else:
        out = {k: _dev(out[k], dtype, (B, h, w) + tail, f"out['{k}']") for k, (dtype, tail) in out_spec.items()}
    head = [L.ptr(t) for t in points] + [L.ptr(valid), L.ptr(off), B, N, L.ptr(K), k_stride, im_h, im_w, int(downsample_scale), int(y_cutoff)]
    return head, keys, out, B, h, w
