"""GPU lidar ground-truth front end: accumulated lidar sweeps -> the `gt_depth [B,H,W]` tensor assemble_batch takes, with the flow
(u, v) and the low-height mask the reference stores beside it.

The reference makes these maps offline (lib/fuse_lidar.py, driven by scripts/cal_gt.py): about a million points per key frame are
moved with their annotated boxes, projected into two camera frames, rasterised in a Python loop over every point and passed through
two occlusion filters.  Here all of it runs on the device in fp64, the ground-truth stage bit for bit as the reference's:
INTEGRATION.md, "Lidar ground-truth front end".

Points of all frames of a batch lie in one array; `frame_offsets` (int32 cuda tensor [B + 1]) gives frame b the points
frame_offsets[b] .. frame_offsets[b + 1] - 1."""
import torch

from . import lib as L
from ._frontend import RasterWorkspace, _dev, _frames, _intrinsics, _size, map_shape, raster_args

PROJ_KEYS = ("x1", "y1", "depth1", "x2", "y2")
FLAG_KEYS = ("low_h", "in_box", "valid")
ENTRY = 15               # doubles per box entry: box_from_sensor [3][4], then l/2, w/2, h/2
OUT_SPEC = {"gt": (torch.float32, (3,)), "depth": (torch.float32, ()), "msk_lh": (torch.uint8, ())}


def workspace_bytes(n_pix, n_boxes=0):
    """include/camradepth_hip.h, crd_lidar_ground_truth: n_pix uint32 winners, n_pix uint64 depth keys and 32 bytes per box, each from a
    16-byte boundary."""
    return ((((4 * n_pix + 15) & ~15) + 8 * n_pix + 15) & ~15) + 32 * n_boxes


class LidarWorkspace(RasterWorkspace):
    """The scratch memory of the front end for batches of up to B frames: the per-pixel key images of the rasteriser (sized for
    y_cutoff = 0, so any cutoff fits), room for the rectangles of up to max_boxes boxes and, with max_points given, the projection's
    outputs for up to that many points.  With workspace= and out= a call allocates nothing, so it can be captured in a graph on one
    stream."""
    GROUPS = (("proj", torch.float64, PROJ_KEYS), ("flags", torch.uint8, FLAG_KEYS), ("box_entry", torch.int32, None))

    def __init__(self, B, image_size=(900, 1600), downsample_scale=2, max_points=None, max_boxes=0, device="cuda"):
        if int(max_boxes) < 0:
            raise L.CrdError(f"LidarWorkspace: max_boxes = {max_boxes}")
        super().__init__(B, image_size, downsample_scale, max_points, lambda n_pix: workspace_bytes(n_pix, int(max_boxes)), device)


def project_lidar(points, sweep_index, frame_offsets, cam1_from_sensor, cam2_from_sensor, car_z_from_sensor, K, sweep_boxes=None,
                  box_entries=None, box_id=None, cam1_from_box=None, cam2_from_box=None, vehicle=None, image_size=(900, 1600),
                  min_distance=2.5, min_z=2.0, h_min=0.3, h_max=2.0, out=None):
    """Height mask, per-box motion compensation, pose chain and pinhole projection of every point into two camera frames
    (crd_lidar_project).

    points [N,3] fp64 in the lidar sensor frame; sweep_index [N] int32: the row of the point's sweep in cam1_from_sensor /
    cam2_from_sensor [S,3,4] and car_z_from_sensor [S,4] (fp64); K [3,3] or [B,3,3] fp64.  Boxes (all six tables or none):
    sweep_boxes [S+1] int32 gives sweep s the entries sweep_boxes[s] .. sweep_boxes[s+1] - 1 of box_entries [E,15] fp64
    (box_from_sensor at the sweep's time as 12 values, then l/2, w/2, h/2) and box_id [E] int32, the row of the box in
    cam1_from_box / cam2_from_box [Nb,3,4] fp64 and vehicle [Nb] uint8.  A point belongs to the first entry of its sweep whose box
    holds it.  Returns {'x1', 'y1', 'depth1', 'x2', 'y2'} fp64 [N], {'low_h', 'in_box', 'valid'} uint8 [N] and 'box_entry' int32
    [N] (-1: in no box), in the order of the points.  out: a dictionary of those nine tensors to write into."""
    off, B = _frames(frame_offsets)
    points = _dev(points, torch.float64, (None, 3), "points")
    N = points.shape[0]
    sweep_index = _dev(sweep_index, torch.int32, (N,), "sweep_index")
    cam1 = _dev(cam1_from_sensor, torch.float64, (None, 3, 4), "cam1_from_sensor")
    S = cam1.shape[0]
    cam2 = _dev(cam2_from_sensor, torch.float64, (S, 3, 4), "cam2_from_sensor")
    car_z = _dev(car_z_from_sensor, torch.float64, (S, 4), "car_z_from_sensor")
    tables = (sweep_boxes, box_entries, box_id, cam1_from_box, cam2_from_box, vehicle)
    if all(t is None for t in tables):
        sweep_boxes = torch.zeros(S + 1, dtype=torch.int32, device=points.device)
        E = Nb = 0
    elif any(t is None for t in tables):
        raise L.CrdError("project_lidar: sweep_boxes, box_entries, box_id, cam1_from_box, cam2_from_box and vehicle go together")
    else:
        sweep_boxes = _dev(sweep_boxes, torch.int32, (S + 1,), "sweep_boxes")
        box_entries = _dev(box_entries, torch.float64, (None, ENTRY), "box_entries")
        E = box_entries.shape[0]
        box_id = _dev(box_id, torch.int32, (E,), "box_id")
        cam1_from_box = _dev(cam1_from_box, torch.float64, (None, 3, 4), "cam1_from_box")
        Nb = cam1_from_box.shape[0]
        cam2_from_box = _dev(cam2_from_box, torch.float64, (Nb, 3, 4), "cam2_from_box")
        vehicle = _dev(vehicle, torch.uint8, (Nb,), "vehicle")
    K, k_stride = _intrinsics(K, B)
    h, w = _size(image_size)
    if out is None:
        buf = torch.empty(len(PROJ_KEYS), N, dtype=torch.float64, device=points.device)
        flags = torch.empty(len(FLAG_KEYS), N, dtype=torch.uint8, device=points.device)
        out = {k: buf[i] for i, k in enumerate(PROJ_KEYS)} | {k: flags[i] for i, k in enumerate(FLAG_KEYS)}
        out["box_entry"] = torch.empty(N, dtype=torch.int32, device=points.device)
    else:
        out = {k: _dev(out[k], torch.float64, (N,), f"out['{k}']") for k in PROJ_KEYS} | \
              {k: _dev(out[k], torch.uint8, (N,), f"out['{k}']") for k in FLAG_KEYS} | \
              {"box_entry": _dev(out["box_entry"], torch.int32, (N,), "out['box_entry']")}
    L.check(L.load().crd_lidar_project(
        L.ptr(points), L.ptr(sweep_index), L.ptr(off), B, N, L.ptr(cam1), L.ptr(cam2), L.ptr(car_z), L.ptr(sweep_boxes), S,
        L.ptr(box_entries) if E else None, L.ptr(box_id) if E else None, E, L.ptr(cam1_from_box) if E else None,
        L.ptr(cam2_from_box) if E else None, L.ptr(vehicle) if E else None, Nb, L.ptr(K), k_stride, h, w, float(min_distance), float(min_z),
        L.f64_bits(h_min), L.f64_bits(h_max), *(L.ptr(out[k]) for k in PROJ_KEYS), *(L.ptr(out[k]) for k in FLAG_KEYS),
        L.ptr(out["box_entry"]), L.stream()), "crd_lidar_project")
    return out


def project_corners(cam_from_box, size, corner_offsets, K, image_size=(900, 1600), min_z=2.0):
    """The corner table of the box occlusion filter, through project_lidar's code path: the eight corners (+-l/2, +-w/2, +-h/2) of every
    box through cam_from_box [Nb,3,4] fp64 -- the reference takes the boxes at camera time 1 with camera 2's pose (fuse_lidar.py:206-207,
    :269); the caller decides -- and K.  size [Nb,3] fp64 = (w, l, h) as nuScenes stores it; corner_offsets int32 [B+1]: frame b owns the
    boxes corner_offsets[b] .. corner_offsets[b+1] - 1.  Returns corners [Nb,8,4] fp64 = x, y, depth, in_view (proj2im's mask)."""
    off, B = _frames(corner_offsets)
    cam = _dev(cam_from_box, torch.float64, (None, 3, 4), "cam_from_box")
    Nb = cam.shape[0]
    size = _dev(size, torch.float64, (Nb, 3), "size")
    half = 0.5 * size[:, [1, 0, 2]]                                                    # l/2, w/2, h/2
    signs = torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)], dtype=torch.float64,
                         device=cam.device)                                            # :70-73
    pts = (half[:, None, :] * signs[None]).reshape(Nb * 8, 3).contiguous()
    sweep = torch.arange(Nb, dtype=torch.int32, device=cam.device).repeat_interleave(8)
    car_z = torch.zeros(Nb, 4, dtype=torch.float64, device=cam.device)
    p = project_lidar(pts, sweep, (off * 8).to(torch.int32), cam, cam, car_z, K, image_size=image_size, min_distance=0.0, min_z=min_z)
    return torch.stack([p["x1"], p["y1"], p["depth1"], p["valid"].double()], dim=1).reshape(Nb, 8, 4).contiguous()


def lidar_ground_truth(proj, frame_offsets, K, image_size=(900, 1600), downsample_scale=2, y_cutoff=34, seg=None, corners=None,
                       corner_offsets=None, flow_im=None, thres=3.0, workspace=None, out=None):
    """The reference's rasteriser, both occlusion filters and the flow's u, v on the device (crd_lidar_ground_truth).

    proj: the dictionary of project_lidar, or cuda tensors [N] of the same names ('valid' is optional: without it every point counts;
    'box_entry' is not read).  Per pixel the point of smallest depth1 wins, the lowest index among equal depths.  Box filter: seg
    [B,h,w] uint8 (non-zero = vehicle) with corners [Nb,8,4] fp64 (project_corners) and corner_offsets int32 [B+1].  Flow filter:
    flow_im [B,h,w,2] fp32 and thres.  Returns {'gt': [B,h,w,3] fp32 = depth, u, v; 'depth': [B,h,w] fp32, what
    assemble_batch(gt_depth=) takes; 'msk_lh': [B,h,w] uint8} with (h, w) = map_shape(...).  workspace: a LidarWorkspace; out: a
    dictionary of the three tensors to write into."""
    fn = "lidar_ground_truth"
    Nb, box_filter = 0, seg is not None or corners is not None or corner_offsets is not None
    if box_filter:
        if seg is None or corners is None or corner_offsets is None:
            raise L.CrdError(f"{fn}: the box filter takes seg, corners and corner_offsets together")
        corners = _dev(corners, torch.float64, (None, 8, 4), "corners")
        Nb = corners.shape[0]
    head, keys, out, B, h, w = raster_args(fn, proj, frame_offsets, K, image_size, downsample_scale, y_cutoff, PROJ_KEYS, ("low_h", "in_box"),
                                           workspace, lambda n_pix: workspace_bytes(n_pix, Nb), out, OUT_SPEC, detail=f", {Nb} boxes")
    if box_filter:
        seg = _dev(seg, torch.uint8, (B, h, w), "seg")
        corner_offsets = _dev(corner_offsets, torch.int32, (B + 1,), "corner_offsets")
    if flow_im is not None:
        flow_im = _dev(flow_im, torch.float32, (B, h, w, 2), "flow_im")
    L.check(L.load().crd_lidar_ground_truth(
        *head, L.ptr(seg), L.ptr(corners) if Nb else None, L.ptr(corner_offsets), Nb, L.ptr(flow_im), L.f64_bits(thres), L.ptr(keys),
        keys.numel(), L.ptr(out["gt"]), L.ptr(out["depth"]), L.ptr(out["msk_lh"]), L.stream()), fn)
    return out


def lidar_gt(points, sweep_index, frame_offsets, cam1_from_sensor, cam2_from_sensor, car_z_from_sensor, K, sweep_boxes=None,
             box_entries=None, box_id=None, cam1_from_box=None, cam2_from_box=None, vehicle=None, image_size=(900, 1600),
             min_distance=2.5, min_z=2.0, h_min=0.3, h_max=2.0, downsample_scale=2, y_cutoff=34, seg=None, corners=None,
             corner_offsets=None, flow_im=None, thres=3.0, workspace=None, out=None):
    """project_lidar, then lidar_ground_truth: lidar sweeps -> {'gt', 'depth', 'msk_lh'}.  With a LidarWorkspace(max_points=), the box
    tables given and out= nothing is allocated; a captured call sized for N points replays with any frame_offsets that end at or below
    N."""
    proj_out = workspace.proj_out(points.shape[0]) if workspace is not None and workspace.max_points is not None and \
        torch.is_tensor(points) else None
    proj = project_lidar(points, sweep_index, frame_offsets, cam1_from_sensor, cam2_from_sensor, car_z_from_sensor, K, sweep_boxes,
                         box_entries, box_id, cam1_from_box, cam2_from_box, vehicle, image_size, min_distance, min_z, h_min, h_max,
                         out=proj_out)
    return lidar_ground_truth(proj, frame_offsets, K, image_size, downsample_scale, y_cutoff, seg, corners, corner_offsets, flow_im,
                              thres, workspace, out)
