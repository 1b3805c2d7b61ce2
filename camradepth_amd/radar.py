"""GPU radar front end: accumulated radar sweeps -> the `radar [B,H,W,3]` and `rad_vel [B,H,W]` tensors assemble_batch takes.

The reference makes these maps offline, in a Python loop over points (lib/fuse_radar.py: the projection nested in
merge_selected_radar, then cal_depthMap_flow and radarFlow2uv).  Here both stages run on the device in fp64, the rasteriser bit for
bit as the reference's: INTEGRATION.md, "Radar front end".  The reference's time and RCS maps are not produced -- the network does
not read them.

Points of all frames of a batch lie in one array; `frame_offsets` (int32 cuda tensor [B + 1]) gives frame b the points
frame_offsets[b] .. frame_offsets[b + 1] - 1."""
import torch

from . import lib as L

PROJ_KEYS = ("x1", "y1", "depth1", "x2", "y2", "v_comp")


def _dev(t, dtype, shape, what):
    """A contiguous cuda tensor of the dtype and shape given (None in `shape`: any extent), or CrdError."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.CrdError(f"{what} must be a cuda tensor (the radar front end has no CPU fallback)")
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


def _intrinsics(K, B):
    """-> (K, k_stride): one 3x3 matrix for every frame, or one per frame."""
    if torch.is_tensor(K) and K.dim() == 3:
        return _dev(K, torch.float64, (B, 3, 3), "K"), 9
    return _dev(K, torch.float64, (3, 3), "K"), 0


def _size(image_size):
    h, w = (int(v) for v in image_size)
    return h, w


def map_shape(image_size=(900, 1600), downsample_scale=2, y_cutoff=34):
    """(rows, columns) of the maps rasterize_radar writes."""
    h, w = _size(image_size)
    s = int(downsample_scale)
    if s <= 0 or h // s <= 0 or w // s <= 0 or not 0 <= int(y_cutoff) < h // s:
        raise L.CrdError(f"radar maps: image {h} x {w}, downsample_scale {downsample_scale}, y_cutoff {y_cutoff} leave no pixel")
    return h // s - int(y_cutoff), w // s


def workspace_bytes(n_pix):
    """include/camradepth_hip.h, crd_radar_rasterize: n_pix uint32 winners, then n_pix uint64 depth keys from a 16-byte boundary."""
    return ((4 * n_pix + 15) & ~15) + 8 * n_pix


class RadarWorkspace:
    """The scratch memory of the front end for batches of up to B frames: the per-pixel key images of the rasteriser (sized for
    y_cutoff = 0, so any cutoff fits) and, with max_points given, the projection's outputs for up to that many points.  With
    workspace= and out= a call allocates nothing, so it can be captured in a graph on one stream."""

    def __init__(self, B, image_size=(900, 1600), downsample_scale=2, max_points=None, device="cuda"):
        h, w = map_shape(image_size, downsample_scale, 0)
        if int(B) <= 0:
            raise L.CrdError(f"RadarWorkspace: B = {B}")
        self.B, self.image_size, self.downsample_scale = int(B), _size(image_size), int(downsample_scale)
        self.keys = torch.empty(workspace_bytes(self.B * h * w), dtype=torch.uint8, device=device)
        self.max_points = None if max_points is None else int(max_points)
        if self.max_points is not None:
            self.proj = torch.empty(len(PROJ_KEYS), self.max_points, dtype=torch.float64, device=device)
            self.valid = torch.empty(self.max_points, dtype=torch.uint8, device=device)

    def proj_out(self, n):
        """The projection buffers for n points, as project_radar(out=) takes them."""
        if self.max_points is None or n > self.max_points:
            raise L.CrdError(f"RadarWorkspace: no room for the projection of {n} points (max_points = {self.max_points})")
        out = {k: self.proj[i, :n] for i, k in enumerate(PROJ_KEYS)}
        out["valid"] = self.valid[:n]
        return out


def project_radar(points, sweep_index, frame_offsets, cam1_from_sensor, cam2_from_sensor, lags, K, image_size=(900, 1600),
                  min_distance=1.0, min_z=2.0, out=None):
    """Doppler compensation, pose chain and pinhole projection of every point into two camera frames (crd_radar_project).

    points [N,5] fp64: x, y, z, vx_comp, vy_comp in the radar sensor frame; sweep_index [N] int32: the row of the point's sweep in
    cam1_from_sensor / cam2_from_sensor [S,3,4] fp64 and lags [S,2] fp64 (camera time minus sweep time, signed); K [3,3] or [B,3,3]
    fp64.  Returns {'x1', 'y1', 'depth1', 'x2', 'y2', 'v_comp'} fp64 [N] and 'valid' uint8 [N], in the order of the points.
    out: a dictionary of those seven tensors to write into."""
    off, B = _frames(frame_offsets)
    points = _dev(points, torch.float64, (None, 5), "points")
    N = points.shape[0]
    sweep_index = _dev(sweep_index, torch.int32, (N,), "sweep_index")
    cam1 = _dev(cam1_from_sensor, torch.float64, (None, 3, 4), "cam1_from_sensor")
    S = cam1.shape[0]
    cam2 = _dev(cam2_from_sensor, torch.float64, (S, 3, 4), "cam2_from_sensor")
    lags = _dev(lags, torch.float64, (S, 2), "lags")
    K, k_stride = _intrinsics(K, B)
    h, w = _size(image_size)
    if out is None:
        buf = torch.empty(len(PROJ_KEYS), N, dtype=torch.float64, device=points.device)
        out = {k: buf[i] for i, k in enumerate(PROJ_KEYS)}
        out["valid"] = torch.empty(N, dtype=torch.uint8, device=points.device)
    else:
        out = {k: _dev(out[k], torch.float64, (N,), f"out['{k}']") for k in PROJ_KEYS} | \
              {"valid": _dev(out["valid"], torch.uint8, (N,), "out['valid']")}
    L.check(L.load().crd_radar_project(L.ptr(points), L.ptr(sweep_index), L.ptr(off), B, N, L.ptr(cam1), L.ptr(cam2), L.ptr(lags), S,
                                       L.ptr(K), k_stride, h, w, float(min_distance), float(min_z),
                                       *(L.ptr(out[k]) for k in PROJ_KEYS), L.ptr(out["valid"]), L.stream()), "crd_radar_project")
    return out


def rasterize_radar(proj, frame_offsets, K, image_size=(900, 1600), downsample_scale=2, y_cutoff=34, workspace=None, out=None):
    """The reference's rasteriser (cal_depthMap_flow + radarFlow2uv) on the device (crd_radar_rasterize).

    proj: the dictionary of project_radar, or fp64 cuda tensors [N] of the same names ('valid', uint8, is optional: without it every
    point counts).  Per pixel the point of smallest depth1 wins, the lowest index among equal depths.  Points with a non-finite
    value or depth1 <= 0 are skipped.  Returns {'radar': [B,h,w,3], 'rad_vel': [B,h,w]} fp32 with (h, w) = map_shape(...), the
    tensors assemble_batch takes.  workspace: a RadarWorkspace; out: a dictionary of the two tensors to write into."""
    off, B = _frames(frame_offsets)
    if not all(k in proj for k in PROJ_KEYS):
        raise L.CrdError(f"rasterize_radar: proj needs {PROJ_KEYS}")
    N = proj["x1"].shape[0] if torch.is_tensor(proj["x1"]) and proj["x1"].dim() == 1 else None
    p = [_dev(proj[k], torch.float64, (N,), f"proj['{k}']") for k in PROJ_KEYS]
    valid = proj.get("valid")
    if valid is not None:
        valid = _dev(valid, torch.uint8, (N,), "proj['valid']")
    K, k_stride = _intrinsics(K, B)
    im_h, im_w = _size(image_size)
    h, w = map_shape(image_size, downsample_scale, y_cutoff)
    need = workspace_bytes(B * h * w)
    if workspace is None:
        keys = torch.empty(need, dtype=torch.uint8, device=p[0].device)
    else:
        keys = workspace.keys
        if keys.numel() < need:
            raise L.CrdError(f"rasterize_radar: the workspace holds {keys.numel()} bytes, {need} are needed "
                             f"(B {B}, image {im_h} x {im_w}, downsample_scale {downsample_scale})")
    if out is None:
        out = {"radar": torch.empty(B, h, w, 3, device=p[0].device), "rad_vel": torch.empty(B, h, w, device=p[0].device)}
    else:
        out = {"radar": _dev(out["radar"], torch.float32, (B, h, w, 3), "out['radar']"),
               "rad_vel": _dev(out["rad_vel"], torch.float32, (B, h, w), "out['rad_vel']")}
    L.check(L.load().crd_radar_rasterize(*(L.ptr(t) for t in p), L.ptr(valid), L.ptr(off), B, N, L.ptr(K), k_stride, im_h, im_w,
                                         int(downsample_scale), int(y_cutoff), L.ptr(keys), keys.numel(), L.ptr(out["radar"]),
                                         L.ptr(out["rad_vel"]), L.stream()), "crd_radar_rasterize")
    return out


def radar_inputs(points, sweep_index, frame_offsets, cam1_from_sensor, cam2_from_sensor, lags, K, image_size=(900, 1600),
                 min_distance=1.0, min_z=2.0, downsample_scale=2, y_cutoff=34, workspace=None, out=None):
    """project_radar, then rasterize_radar: radar sweeps -> {'radar', 'rad_vel'}.  With a RadarWorkspace(max_points=) and out= nothing
    is allocated; a captured call sized for N points replays with any frame_offsets that end at or below N."""
    proj_out = workspace.proj_out(points.shape[0]) if workspace is not None and workspace.max_points is not None and \
        torch.is_tensor(points) else None
    proj = project_radar(points, sweep_index, frame_offsets, cam1_from_sensor, cam2_from_sensor, lags, K, image_size, min_distance,
                         min_z, out=proj_out)
    return rasterize_radar(proj, frame_offsets, K, image_size, downsample_scale, y_cutoff, workspace, out)
