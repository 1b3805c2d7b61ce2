"""GPU distance field: a state map -> clearance, costmap and path checks, the two questions a planner asks of the occupancy map.

The step after occupancy.update, whose `state` says free / occupied / unknown per cell.  distance_field gives, for every cell of the
window, the exact squared Euclidean distance in cells to the nearest source cell (by default the OCCUPIED ones) truncated at
max_cells, which cell that is, the clearance in metres and an inflated costmap by the rule of ROS costmap_2d; check_paths reads that
costmap along K candidate trajectories on the device.  The two tables that turn a squared distance into metres and into a cost are
made on the host (tables), so the device side is integers and look-ups only, specified operation by operation in
include/camradepth_hip.h and the same bits every run: INTEGRATION.md, "Distance field".  Nothing calls this module unless asked."""
import math

import numpy as np
import torch

from . import lib as L
from . import viz
from ._frontend import _dev
from .occupancy import OCCUPIED

OUTPUTS = {"dist2": torch.int32, "nearest": torch.int32, "clearance": torch.float32, "cost": torch.uint8}
OPTIONAL = ("clearance", "cost")                     # out= may hold None for these: the kernel then leaves them out
PATH_OUTPUTS = {"first_blocked": torch.int32, "max_cost": torch.uint8, "min_dist2": torch.int32, "n_outside": torch.int32,
                "n_unknown": torch.int32}
SPEC_OPTIONS = {"max_cells": 32, "inscribed": 0.0, "inflation": None, "scale": 10.0, "sources": (OCCUPIED,), "unknown_cost": 0,
                "cost_table": None}
LETHAL, INSCRIBED = 254, 253                         # costmap_2d's costs of a source cell and of a cell within the inscribed radius


def workspace_bytes(M, nx, ny):
    """include/camradepth_hip.h, crd_distance_field: row_near, int32 [M][nx][ny], up to a multiple of 16 bytes."""
    return (4 * M * nx * ny + 15) & ~15


def _whole(v, what, fn="FieldSpec"):
    try:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise L.CrdError(f"{fn}: {what} must be an integer, not {v!r}") from None
    return int(v)


def _numbers(cell, max_cells, inscribed, inflation, scale, fn):
    max_cells = _whole(max_cells, "max_cells", fn)
    try:
        cell, inscribed, scale = float(cell), float(inscribed), float(scale)
        inflation = None if inflation is None else float(inflation)
    except (TypeError, ValueError):
        raise L.CrdError(f"{fn}: cell, inscribed, inflation and scale are numbers") from None
    if not (cell > 0 and math.isfinite(cell)):
        raise L.CrdError(f"{fn}: cell {cell} is not a finite positive size")
    if not 1 <= max_cells <= 255:
        raise L.CrdError(f"{fn}: max_cells {max_cells} is not in 1 .. 255")
    if inflation is None:
        inflation = max_cells * cell
    for name, v in (("inscribed", inscribed), ("inflation", inflation), ("scale", scale)):
        if not (v >= 0 and math.isfinite(v)):
            raise L.CrdError(f"{fn}: {name} {v} is negative or not finite")
    if inflation > max_cells * cell:
        raise L.CrdError(f"{fn}: inflation {inflation} reaches beyond max_cells * cell = {max_cells * cell}, where the field ends")
    if inscribed > inflation:
        raise L.CrdError(f"{fn}: inscribed {inscribed} is larger than inflation {inflation}")
    return cell, max_cells, inscribed, inflation, scale


def tables(cell, max_cells, inscribed=0.0, inflation=None, scale=10.0):
    """-> (clear_table fp32, cost_table uint8), NumPy arrays of max_cells^2 + 2 entries indexed by a squared distance in cells; the
    last, FAR = max_cells^2 + 1, stands for "no source within max_cells".  With d = cell * sqrt(d2) in fp64: clear_table[d2] =
    float32(d), +inf at FAR; cost_table[d2], costmap_2d's rule: 254 at d2 = 0, 253 where d <= inscribed, int(252 * exp(-scale * (d -
    inscribed))) where d <= inflation, 0 beyond it and at FAR.  inflation None: max_cells * cell."""
    cell, R, inscribed, inflation, scale = _numbers(cell, max_cells, inscribed, inflation, scale, "tables")
    far = R * R + 1
    d = np.float64(cell) * np.sqrt(np.arange(far + 1, dtype=np.float64))
    clear = d.astype(np.float32)
    clear[far] = np.inf
    cost = np.where(d <= inscribed, np.float64(INSCRIBED),
                    np.where(d <= inflation, np.floor(252.0 * np.exp(-scale * (d - inscribed))), 0.0)).astype(np.uint8)
    cost[0], cost[far] = LETHAL, 0
    return clear, cost


class FieldSpec:
    """The numbers of a distance field, checked on the host, and its two tables on the device.

    cell: metres per cell, the map's.  max_cells: the radius R in cells, 1 .. 255, at which the field is truncated.  inscribed,
    inflation, scale: costmap_2d's radii in metres and its decay per metre (tables).  sources: the states that count as obstacles,
    each 0 .. 7.  unknown_cost: 0, or the least cost a cell of state 0 gets, up to 255.  cost_table: None, or the caller's own 1-D
    uint8 table of max_cells^2 + 2 entries in place of costmap_2d's.  `clear_table` and `cost_table` live on `device`."""

    def __init__(self, cell, max_cells=32, inscribed=0.0, inflation=None, scale=10.0, sources=(OCCUPIED,), unknown_cost=0, cost_table=None,
                 device="cuda"):
        fn = "FieldSpec"
        self.cell, self.max_cells, self.inscribed, self.inflation, self.scale = _numbers(cell, max_cells, inscribed, inflation, scale, fn)
        try:
            states = [_whole(s, "a state of sources", fn) for s in sources]
        except TypeError:
            raise L.CrdError(f"{fn}: sources {sources!r} is a sequence of states 0 .. 7") from None
        if not states or any(not 0 <= s <= 7 for s in states):
            raise L.CrdError(f"{fn}: sources {sources!r} holds at least one state, each 0 .. 7")
        self.sources = tuple(states)
        self.source_mask = 0
        for s in states:
            self.source_mask |= 1 << s
        self.unknown_cost = _whole(unknown_cost, "unknown_cost", fn)
        if not 0 <= self.unknown_cost <= 255:
            raise L.CrdError(f"{fn}: unknown_cost {unknown_cost} is not in 0 .. 255")
        self.far = self.max_cells * self.max_cells + 1
        clear, cost = tables(self.cell, self.max_cells, self.inscribed, self.inflation, self.scale)
        if cost_table is not None:
            if torch.is_tensor(cost_table):
                cost_table = cost_table.detach().cpu().numpy()
            cost_table = np.asarray(cost_table)
            if cost_table.dtype != np.uint8 or cost_table.shape != (self.far + 1,):
                raise L.CrdError(f"{fn}: cost_table is uint8 [{self.far + 1}] (max_cells^2 + 2), not {cost_table.dtype} "
                                 f"{list(cost_table.shape)}")
            cost = np.ascontiguousarray(cost_table)
        self.clear_table = torch.from_numpy(clear).to(device)
        self.cost_table = torch.from_numpy(cost.copy()).to(device)


def _spec(spec, fn):
    if not isinstance(spec, FieldSpec):
        raise L.CrdError(f"{fn}: the first argument is a FieldSpec")
    return spec


class FieldWorkspace:
    """The scratch memory of distance_field for M maps of nx x ny cells and its preallocated outputs: `row_near`, int32 [M,nx,ny], launch
    1's table, and `out`, the dictionary distance_field(out=) takes.  With workspace= and out= a call allocates nothing, so it can be
    captured in a graph on one stream."""

    def __init__(self, spec, M, nx, ny):
        _spec(spec, "FieldWorkspace")
        M, nx, ny = (_whole(v, k, "FieldWorkspace") for k, v in (("M", M), ("nx", nx), ("ny", ny)))
        if M <= 0 or not 1 <= nx <= 65535 or not 1 <= ny <= 65535 or M * nx * ny >= 2 ** 31:
            raise L.CrdError(f"FieldWorkspace: M {M} maps of {nx} x {ny} cells (M >= 1, each side 1 .. 65535, fewer than 2^31 cells)")
        dev = spec.clear_table.device
        self.shape = (M, nx, ny)
        self.buf = torch.empty(workspace_bytes(M, nx, ny), dtype=torch.uint8, device=dev)
        self.row_near = self.buf[:4 * M * nx * ny].view(torch.int32).view(M, nx, ny)
        self.out = {k: torch.empty(M, nx, ny, dtype=t, device=dev) for k, t in OUTPUTS.items()}


def _state_of(v, fn):
    state = v["state"] if isinstance(v, dict) and "state" in v else v
    return _dev(state, torch.uint8, (None, None, None), "state")


def distance_field(spec, state_or_update_result, workspace=None, out=None):
    """The field of a state map (crd_distance_field, two launches on the current stream).

    state_or_update_result: uint8 [M,nx,ny] on the device in WINDOW order, or occupancy.update's dictionary (its 'state').  A cell is a
    source when its state is one of spec.sources.  Returns 'dist2' int32 (squared distance in cells to the nearest source, spec.far =
    max_cells^2 + 1 where none lies within max_cells), 'nearest' int32 (i * ny + j of that source, the lowest among equal ones; -1),
    'clearance' fp32 (metres; +inf) and 'cost' uint8 (the costmap), each [M,nx,ny].  workspace: a FieldWorkspace; out: its `out`, in
    which 'clearance' and 'cost' may be None (left out): then nothing is allocated and nothing waits for the device."""
    fn = "field.distance_field"
    _spec(spec, fn)
    state = _state_of(state_or_update_result, fn)
    M, nx, ny = state.shape
    dev = state.device
    if spec.clear_table.device != dev:
        raise L.CrdError(f"{fn}: the tables live on {spec.clear_table.device}, the map on {dev}")
    need = workspace_bytes(M, nx, ny)
    if workspace is None:
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        buf = workspace.buf
        if buf.numel() < need or workspace.shape != (M, nx, ny):
            raise L.CrdError(f"{fn}: the workspace was made for {list(workspace.shape)}, the map is {[M, nx, ny]}")
    if out is None:
        out = {k: torch.empty(M, nx, ny, dtype=t, device=dev) for k, t in OUTPUTS.items()}
    else:
        if not isinstance(out, dict) or set(out) != set(OUTPUTS):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(OUTPUTS)}")
        out = {k: None if out[k] is None and k in OPTIONAL else _dev(out[k], t, (M, nx, ny), f"out['{k}']") for k, t in OUTPUTS.items()}
    L.check(L.load().crd_distance_field(L.ptr(state), M, nx, ny, spec.source_mask, spec.max_cells, spec.unknown_cost, L.ptr(spec.clear_table),
                                        L.ptr(spec.cost_table), L.ptr(buf), buf.numel(), L.ptr(out["dist2"]), L.ptr(out["nearest"]),
                                        L.ptr(out["clearance"]), L.ptr(out["cost"]), L.stream()), "crd_distance_field")
    return out


def path_outputs(K, P, pose_cell=False, device="cuda"):
    """The dictionary check_paths(out=) takes for K paths of P poses."""
    out = {k: torch.empty(K, dtype=t, device=device) for k, t in PATH_OUTPUTS.items()}
    if pose_cell:
        out["pose_cell"] = torch.empty(K, P, dtype=torch.int32, device=device)
    return out


def check_paths(spec, field_result, map_or_state_origin, xy, n_poses=None, path_map=None, blocked_at=253, outside_blocks=True, pose_cell=False,
                out=None):
    """K candidate trajectories against the costmap (crd_field_paths, one launch on the current stream).

    field_result: distance_field's dictionary, with its 'cost'.  map_or_state_origin: occupancy.update's dictionary, or (state, origin)
    -- uint8 [M,nx,ny] and int64 [M,2] on the device; the origin is read there, not on the host.  xy: fp64 [K,P,2] on the device, metres
    in the map frame.  n_poses: int32 [K], the poses of each path that count (None: all P).  path_map: int32 [K], the map of each path
    (None: map 0; an index outside 0 .. M-1 puts every pose of the path outside).  A pose is inside when it is finite and falls into the
    window, blocked when inside with cost >= blocked_at or outside with outside_blocks.

    Returns, per path: 'first_blocked' int32 (the first blocked pose, -1: the path is clear), 'max_cost' uint8 and 'min_dist2' int32
    over the inside poses (0 and spec.far without one), 'n_outside' int32, 'n_unknown' int32 (inside poses on cells of state 0), and with
    pose_cell=True 'pose_cell' int32 [K,P] (i * ny + j of every pose, -1 outside, -2 beyond n_poses).  out: path_outputs(): then nothing
    is allocated and nothing waits for the device."""
    fn = "field.check_paths"
    _spec(spec, fn)
    if not isinstance(field_result, dict) or not all(k in field_result for k in ("dist2", "cost")) or field_result["cost"] is None:
        raise L.CrdError(f"{fn}: field_result is distance_field's dictionary with its 'cost'")
    if isinstance(map_or_state_origin, dict) and "state" in map_or_state_origin and "origin" in map_or_state_origin:
        state, origin = map_or_state_origin["state"], map_or_state_origin["origin"]
    elif isinstance(map_or_state_origin, (tuple, list)) and len(map_or_state_origin) == 2:
        state, origin = map_or_state_origin
    else:
        raise L.CrdError(f"{fn}: the third argument is occupancy.update's dictionary or (state, origin)")
    state = _dev(state, torch.uint8, (None, None, None), "state")
    M, nx, ny = state.shape
    origin = _dev(origin, torch.int64, (M, 2), "origin")
    dist2 = _dev(field_result["dist2"], torch.int32, (M, nx, ny), "field_result['dist2']")
    cost = _dev(field_result["cost"], torch.uint8, (M, nx, ny), "field_result['cost']")
    xy = _dev(xy, torch.float64, (None, None, 2), "xy")
    K, P = xy.shape[:2]
    if K < 1 or P < 1:
        raise L.CrdError(f"{fn}: xy holds K {K} paths of P {P} poses; each is at least 1")
    if n_poses is not None:
        n_poses = _dev(n_poses, torch.int32, (K,), "n_poses")
    if path_map is not None:
        path_map = _dev(path_map, torch.int32, (K,), "path_map")
    blocked_at = _whole(blocked_at, "blocked_at", fn)
    if not 1 <= blocked_at <= 255:
        raise L.CrdError(f"{fn}: blocked_at {blocked_at} is not in 1 .. 255")
    names = list(PATH_OUTPUTS) + (["pose_cell"] if pose_cell else [])
    if out is None:
        out = path_outputs(K, P, pose_cell, xy.device)
    else:
        if not isinstance(out, dict) or set(out) != set(names):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {names}")
        out = {k: _dev(out[k], PATH_OUTPUTS.get(k, torch.int32), (K, P) if k == "pose_cell" else (K,), f"out['{k}']") for k in names}
    L.check(L.load().crd_field_paths(L.ptr(xy), L.ptr(n_poses), L.ptr(path_map), K, P, L.ptr(origin), L.f64_bits(spec.cell), L.ptr(state),
                                     L.ptr(dist2), L.ptr(cost), M, nx, ny, spec.max_cells, blocked_at, 1 if outside_blocks else 0,
                                     L.ptr(out["first_blocked"]), L.ptr(out["max_cost"]), L.ptr(out["min_dist2"]), L.ptr(out["n_outside"]),
                                     L.ptr(out["n_unknown"]), L.ptr(out.get("pose_cell")), L.stream()), "crd_field_paths")
    return out


def picture(result, spec, cmap="jet", out=None, workspace=None):
    """The clearance result['clearance'] in the colours of cmap -> uint8 RGB [M,nx,ny,3]: viz.colorize over the fixed range 0 ..
    max_cells * cell, which needs no reduction.  Cells without a source in reach are +inf and come out in viz's bad colour.  out and
    workspace as for viz.colorize."""
    if not isinstance(result, dict) or result.get("clearance") is None:
        raise L.CrdError("picture: result is distance_field's dictionary with its 'clearance'")
    _spec(spec, "picture")
    return viz.colorize(result["clearance"], cmap, vmin=0.0, vmax=spec.max_cells * spec.cell, out=out, workspace=workspace)
