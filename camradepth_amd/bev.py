"""GPU bird's-eye-view back end: a point cloud -> top-down grids in the caller's frame.

The step after cloud.point_cloud / cloud.unproject_depth: per cell of an x-y grid the number of points, the highest and the lowest
point, the row of the highest point with its class, and occupancy (`bev_grid`); `picture` colours the height map with viz.colorize.
Which frame owns a row comes from the cloud's own `frame_offsets` on the device, so nothing waits for the host.  All arithmetic is
fp64 on the device, specified operation by operation in include/camradepth_hip.h and the same bits every run: INTEGRATION.md,
"Bird's-eye-view back end".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from . import viz
from ._frontend import _dev, _rows

OPTIONAL = ("z_min", "top_index", "occupancy")
GRID_OPTIONS = {"x_range": (0.0, 80.0), "y_range": (-40.0, 40.0), "cell": 0.5, "z_range": (-math.inf, math.inf), "min_points": 1,
                "flip": (False, False)}
# camera frame (x right, y down, z forward) -> x forward, y left, z up: grid_from_points for a cloud without a pose.  A host tensor:
# put it on the device once (CAM_TO_BEV.cuda()), outside a captured region
CAM_TO_BEV = torch.tensor(((0.0, 0.0, 1.0, 0.0), (-1.0, 0.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.0)), dtype=torch.float64)


def workspace_bytes(B, nx, ny):
    """include/camradepth_hip.h, crd_bev_grid: two uint64 key images and one uint32 winner image of B * nx * ny cells, each from a
    16-byte boundary."""
    cells = B * nx * ny
    return 2 * ((8 * cells + 15) & ~15) + ((4 * cells + 15) & ~15)


def _cells(lo, hi, cell, what):
    n = round((hi - lo) / cell) if cell > 0 and math.isfinite(cell) and math.isfinite(hi - lo) else 0
    if n < 1 or n > 65535 or abs(n * cell - (hi - lo)) > 1e-9 * abs(hi - lo):
        raise L.CrdError(f"bev: {what} ({lo}, {hi}) is not a whole number (1 .. 65535) of cells of {cell}")
    return n


def grid_shape(x_range=(0, 80), y_range=(-40, 40), cell=0.5):
    """(nx, ny): the cells of the grid along x and y; the ranges are a whole number of cells within 1e-9 relative."""
    try:
        (x_lo, x_hi), (y_lo, y_hi), cell = (float(v) for v in x_range), (float(v) for v in y_range), float(cell)
    except (TypeError, ValueError):
        raise L.CrdError(f"bev: x_range {x_range!r}, y_range {y_range!r}, cell {cell!r}: two pairs of numbers and a number") from None
    return _cells(x_lo, x_hi, cell, "x_range"), _cells(y_lo, y_hi, cell, "y_range")


class BevWorkspace:
    """The scratch memory of bev_grid and its preallocated outputs for B frames of nx x ny cells.  `outputs(label=)` is the dictionary
    bev_grid(out=) takes (label: with 'top_label', for a cloud that carries labels).  With workspace= and out= a call allocates
    nothing, so it can be captured in a graph on one stream."""

    def __init__(self, B, nx, ny, device="cuda"):
        if int(B) <= 0 or not 1 <= int(nx) <= 65535 or not 1 <= int(ny) <= 65535 or int(B) * int(nx) * int(ny) >= 2 ** 31:
            raise L.CrdError(f"BevWorkspace: B {B}, grid {nx} x {ny}")
        self.B, self.nx, self.ny = int(B), int(nx), int(ny)
        shape = (self.B, self.nx, self.ny)
        self.keys = torch.empty(workspace_bytes(*shape), dtype=torch.uint8, device=device)
        self.count = torch.empty(shape, dtype=torch.int32, device=device)
        self.z_max = torch.empty(shape, device=device)
        self.z_min = torch.empty(shape, device=device)
        self.top_index = torch.empty(shape, dtype=torch.int32, device=device)
        self.top_label = torch.empty(shape, dtype=torch.uint8, device=device)
        self.occupancy = torch.empty(shape, dtype=torch.uint8, device=device)

    def outputs(self, label=False):
        keys = ("count", "z_max") + OPTIONAL + (("top_label",) if label else ())
        return {k: getattr(self, k) for k in keys}

    @property
    def out(self):
        return self.outputs()


def bev_grid(cloud_or_xyz, frame_offsets=None, x_range=(0, 80), y_range=(-40, 40), cell=0.5, z_range=(-math.inf, math.inf), min_points=1,
             grid_from_points=None, valid=None, labels=None, flip=(False, False), workspace=None, out=None):
    """The grids of a point cloud (crd_bev_grid): cell [b][i][j] covers x_range[0] + i * cell <= X < .. + cell and y_range[0] + j * cell
    <= Y < .. + cell of frame b (flip: the x or the y axis reversed, e.g. for a picture with forward up).

    cloud_or_xyz: point_cloud's dictionary ('xyz', 'frame_offsets', and 'label' if it has one), unproject_depth's dictionary ('points',
    'valid') or an fp32 [n,3] cuda tensor with frame_offsets (int32 [B+1], device).  grid_from_points: fp64 [3,4] or [B,3,4], applied to
    every point first (CAM_TO_BEV.cuda() for a cloud in the camera's frame); None: the cloud is in the grid's frame already, as with
    point_cloud(out_from_cam=).  Points outside z_range (inclusive; infinite bounds allowed), outside the grid, masked by valid (uint8
    [n]) or non-finite are left out.  labels: uint8 [n], the points' classes ([B,h,w] with an organised cloud).

    Returns {'count' int32, 'z_max' fp32, 'z_min' fp32, 'top_index' int32, 'occupancy' uint8 [, 'top_label' uint8]}, each [B,nx,ny]
    with (nx, ny) = grid_shape(x_range, y_range, cell): the points of the cell, its highest and lowest Z, the row of its highest point
    (the lowest row among equals), count >= min_points, and the label of that row.  An empty cell has 0, NaN (bits 0x7fc00000), NaN,
    -1, 0 and 255.  workspace: a BevWorkspace; out: a dictionary of exactly the tensors the call returns (BevWorkspace.outputs(...)):
    then nothing is allocated and nothing waits for the device."""
    fn = "bev_grid"
    nx, ny = grid_shape(x_range, y_range, cell)
    try:
        z_lo, z_hi = (float(v) for v in z_range)
        flip_x, flip_y = (bool(v) for v in flip)
    except (TypeError, ValueError):
        raise L.CrdError(f"{fn}: z_range {z_range!r} is two numbers, flip {flip!r} two booleans") from None
    if math.isnan(z_lo) or math.isnan(z_hi) or z_lo > z_hi:
        raise L.CrdError(f"{fn}: z_range ({z_lo}, {z_hi}): no NaN, low <= high")
    if int(min_points) != min_points or int(min_points) < 1:
        raise L.CrdError(f"{fn}: min_points must be an integer >= 1, not {min_points}")
    xyz, valid, labels, off, rows_per_frame, B = _rows(fn, cloud_or_xyz, frame_offsets, valid, labels)
    n = xyz.shape[0]
    if valid is not None:
        valid = _dev(valid, torch.uint8, (n,), "valid")
    if labels is not None:
        labels = _dev(labels, torch.uint8, (n,), "labels")
    T, t_stride = None, 0
    if grid_from_points is not None:
        per_frame = torch.is_tensor(grid_from_points) and grid_from_points.dim() == 3
        T = _dev(grid_from_points, torch.float64, (B, 3, 4) if per_frame else (3, 4), "grid_from_points")
        t_stride = 12 if per_frame else 0
    if B * nx * ny >= 2 ** 31:
        raise L.CrdError(f"{fn}: {B} grids of {nx} x {ny} cells are more than the 32-bit indices hold")
    dev = xyz.device
    need = workspace_bytes(B, nx, ny)
    if workspace is None:
        keys = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        keys = workspace.keys
        if keys.numel() < need:
            raise L.CrdError(f"{fn}: the workspace holds {keys.numel()} bytes, {need} are needed (B {B}, grid {nx} x {ny})")
    dtypes = {"count": torch.int32, "z_max": torch.float32, "z_min": torch.float32, "top_index": torch.int32, "occupancy": torch.uint8,
              "top_label": torch.uint8}
    names = ("count", "z_max") + OPTIONAL + (("top_label",) if labels is not None else ())
    if out is None:
        out = {k: torch.empty(B, nx, ny, dtype=dtypes[k], device=dev) for k in names}
    else:
        if not isinstance(out, dict) or set(out) != set(names):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(names)} ('top_label' goes with labels)")
        out = {k: _dev(out[k], dtypes[k], (B, nx, ny), f"out['{k}']") for k in names}
    L.check(L.load().crd_bev_grid(L.ptr(xyz), L.ptr(valid), L.ptr(labels), L.ptr(off), rows_per_frame, B, n, L.ptr(T), t_stride,
                                  L.f64_bits(float(x_range[0])), L.f64_bits(float(y_range[0])), L.f64_bits(cell), nx, ny, L.f64_bits(z_lo),
                                  L.f64_bits(z_hi), int(min_points), int(flip_x), int(flip_y), L.ptr(keys), keys.numel(), L.ptr(out["count"]),
                                  L.ptr(out["z_max"]), L.ptr(out["z_min"]), L.ptr(out["top_index"]), L.ptr(out.get("top_label")),
                                  L.ptr(out["occupancy"]), L.stream()), "crd_bev_grid")
    return out


def picture(grid, z_range, cmap="jet", out=None, workspace=None):
    """The height map grid['z_max'] in the colours of cmap -> uint8 RGB [B,nx,ny,3]: viz.colorize with the fixed finite range z_range =
    (low, high), which needs no reduction; an empty cell is drawn in colorize's bad_colour (black).  out and workspace as for
    viz.colorize."""
    if not isinstance(grid, dict) or "z_max" not in grid:
        raise L.CrdError("picture: grid is bev_grid's dictionary")
    try:
        lo, hi = (float(v) for v in z_range)
    except (TypeError, ValueError):
        raise L.CrdError(f"picture: z_range {z_range!r} is two finite numbers") from None
    return viz.colorize(grid["z_max"], cmap, vmin=lo, vmax=hi, out=out, workspace=workspace)
