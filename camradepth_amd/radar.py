"""GPU radar front end: accumulated radar sweeps -> the `radar [B,H,W,3]` and `rad_vel [B,H,W]` tensors assemble_batch takes.

The reference makes these maps offline, in a Python loop over points (lib/fuse_radar.py: the projection nested in
merge_selected_radar, then cal_depthMap_flow and radarFlow2uv).  Here both stages run on the device in fp64, the rasteriser bit for
bit as the reference's: INTEGRATION.md, "Radar front end".  The reference's time and RCS maps are not produced -- the network does
not read them.

Points of all frames of a batch lie in one array; `frame_offsets` (int32 cuda tensor [B + 1]) gives frame b the points
frame_offsets[b] .. frame_offsets[b + 1] - 1."""
import torch

from . import lib as L
from ._frontend import RasterWorkspace, _dev, _frames, _intrinsics, _size, map_shape, raster_args

PROJ_KEYS = ("x1", "y1", "depth1", "x2", "y2", "v_comp")
OUT_SPEC = {"radar": (torch.float32, (3,)), "rad_vel": (torch.float32, ())}


def workspace_bytes(n_pix):
    """include/camradepth_hip.h, crd_radar_rasterize: n_pix uint32 winners, then n_pix uint64 depth keys from a 16-byte boundary."""
    return ((4 * n_pix + 15) & ~15) + 8 * n_pix


class RadarWorkspace(RasterWorkspace):
    """The scratch memory of the front end for batches of up to B frames: the per-pixel key images of the rasteriser (sized for
    y_cutoff = 0, so any cutoff fits) and, with max_points given, the projection's outputs for up to that many points.  With
    workspace= and out= a call allocates nothing, so it can be captured in a graph on one stream."""
    GROUPS = (("proj", torch.float64, PROJ_KEYS), ("valid", torch.uint8, None))

    def __init__(self, B, image_size=(900, 1600), downsample_scale=2, max_points=None, device="cuda"):
        super().__init__(B, image_size, downsample_scale, max_points, workspace_bytes, device)


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
    head, keys, out, _, _, _ = raster_args("rasterize_radar", proj, frame_offsets, K, image_size, downsample_scale, y_cutoff, PROJ_KEYS, (),
                                           workspace, workspace_bytes, out, OUT_SPEC)
    L.check(L.load().crd_radar_rasterize(*head, L.ptr(keys), keys.numel(), L.ptr(out["radar"]), L.ptr(out["rad_vel"]), L.stream()),
            "crd_radar_rasterize")
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
