"""GPU terrain map: point clouds -> a ground height per cell, fused over frames, and the traversability of every cell from local
height differences.

The occupancy map judges a point by its absolute height in the map frame, which holds on a flat world only: on a ramp the road itself
enters the obstacle band.  A TerrainMap holds, for the occupancy map's window of nx x ny cells (the same torus, the same origin rule),
the fused ground height and the fused highest point under the headroom as integers of z_quantum metres; `update` feeds it one batch
of clouds and derives per cell the step (inside the cell and to its neighbours), the squared slope, a state in occupancy's codes
(UNKNOWN, FREE, OCCUPIED) and a hazard in costmap_2d's (0 .. 253, 254 lethal, 255 no information).  field.distance_field,
field.check_paths, nav.nav_field, objects.map_objects and rollout.plan_rollouts take the result as they take occupancy.update's.  The
rows are fp64 on the device, everything behind them is integer arithmetic, specified operation by operation in
include/camradepth_hip.h and the same bits every run: INTEGRATION.md, "Terrain map".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from . import viz
from ._frontend import _dev, _rows
from .occupancy import FREE, OCCUPIED, SENSOR_NOT_FINITE, SKIPPED, UNKNOWN, _point  # noqa: F401  (re-exported)

OUTPUTS = {"ground": torch.int32, "top": torch.int32, "step": torch.int32, "slope2": torch.int64, "weight": torch.int16,
           "state": torch.uint8, "hazard": torch.uint8, "evidence": torch.uint8, "value": torch.float32, "origin": torch.int64}
MAP_OPTIONS = {"z_quantum": 0.01, "z_range": (-50.0, 50.0), "max_range": 80.0, "headroom": 2.5, "min_points": 2, "w_max": 15,
               "step_max": 0.25, "slope_max": 0.35}
NO_INFORMATION, LETHAL = 255, 254                    # 'hazard'
Q_LIMIT = 2 ** 24                                    # |z| / z_quantum stays below it
INT_CAP, SLOPE2_CAP = 2 ** 30, 2 ** 62               # head_q and step_max_q; slope2_max: no height difference reaches them


def workspace_bytes(B, M, nx, ny):
    """include/camradepth_hip.h, crd_terrain_update: lo, hi and n of M * nx * ny cells, B sensor positions and M flags, each from a
    16-byte boundary."""
    def up(n):
        return (n + 15) & ~15
    return 3 * up(4 * M * nx * ny) + up(24 * B) + up(4 * M)


def _whole(v, what):
    try:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise L.CrdError(f"TerrainMap: {what} must be an integer, not {v!r}") from None
    return int(v)


def _capped_floor(v, cap):
    """floor(v) for v >= 0 as an integer, at most cap (+inf and anything beyond give cap)."""
    return cap if not v < cap else int(math.floor(v))


class TerrainMap:
    """M maps of nx x ny cells of `cell` metres in a fixed map frame, with everything update() needs to know about them.

    z_quantum: the unit of the stored heights in metres.  z_range: points lower or higher in the map frame are left out; |z| /
    z_quantum stays below 2^24.  max_range: points farther from the sensor (in x, y) are left out.  headroom: what stands higher than
    this above the lowest point of its cell is not in the vehicle's way.  min_points rows make a cell observed.  w_max (1 .. 32767):
    the running mean of a cell turns into an exponential filter of gain 1 / (w_max + 1) after w_max observations.  A cell is OCCUPIED
    when its step exceeds step_max metres or its slope (rise over run) slope_max.

    State on the device: `ground`, `top` int32 and `weight` int16 [M,nx,ny] (the torus: world cell (wx, wy) in slot (wx mod nx, wy
    mod ny)), `prev_origin` and `cur_origin` int64 [M,2], `initialised` int32 [M], `status_word` int32 [M].  `head_q`, `step_max_q`,
    `slope2_max`: the thresholds in quanta, as the C entry takes them."""

    def __init__(self, M, nx, ny, cell, z_quantum=0.01, z_range=(-50.0, 50.0), max_range=80.0, headroom=2.5, min_points=2, w_max=15,
                 step_max=0.25, slope_max=0.35, device="cuda"):
        fn = "TerrainMap"
        M, nx, ny, min_points, w_max = (_whole(v, k) for k, v in (("M", M), ("nx", nx), ("ny", ny), ("min_points", min_points), ("w_max", w_max)))
        try:
            z_min, z_max = (float(v) for v in z_range)
            cell, z_quantum, max_range, headroom, step_max, slope_max = (float(v) for v in (cell, z_quantum, max_range, headroom, step_max,
                                                                                            slope_max))
        except (TypeError, ValueError):
            raise L.CrdError(f"{fn}: cell, z_quantum, max_range, headroom, step_max and slope_max are numbers, z_range is two") from None
        if M <= 0 or not 1 <= nx <= 65535 or not 1 <= ny <= 65535 or M * nx * ny >= 2 ** 31:
            raise L.CrdError(f"{fn}: M {M} maps of {nx} x {ny} cells (M >= 1, each side 1 .. 65535, fewer than 2^31 cells)")
        if not (cell > 0 and math.isfinite(cell)):
            raise L.CrdError(f"{fn}: cell {cell} is not a finite positive size")
        if not (z_quantum > 0 and math.isfinite(z_quantum)):
            raise L.CrdError(f"{fn}: z_quantum {z_quantum} is not a finite positive size")
        if not (math.isfinite(z_min) and math.isfinite(z_max) and z_min <= z_max and abs(z_min) / z_quantum < Q_LIMIT and
                abs(z_max) / z_quantum < Q_LIMIT):
            raise L.CrdError(f"{fn}: z_range {z_min} .. {z_max}: finite, ordered, |z| / z_quantum {z_quantum} below 2^24")
        if not (max_range > 0 and math.isfinite(max_range * max_range)):
            raise L.CrdError(f"{fn}: max_range {max_range} must be positive, with a finite square")
        if min_points < 1:
            raise L.CrdError(f"{fn}: min_points must be an integer >= 1, not {min_points}")
        if not 1 <= w_max <= 32767:
            raise L.CrdError(f"{fn}: w_max {w_max} is not in 1 .. 32767")
        for k, v in (("headroom", headroom), ("step_max", step_max), ("slope_max", slope_max)):
            if not (v >= 0 and math.isfinite(v)):
                raise L.CrdError(f"{fn}: {k} {v} is negative or not finite")
        self.M, self.nx, self.ny, self.cell, self.z_quantum, self.z_range, self.max_range = M, nx, ny, cell, z_quantum, (z_min, z_max), max_range
        self.headroom, self.min_points, self.w_max, self.step_max, self.slope_max = headroom, min_points, w_max, step_max, slope_max
        self.head_q = _capped_floor(headroom / z_quantum, INT_CAP)
        self.step_max_q = max(_capped_floor(step_max / z_quantum, INT_CAP), 1)
        run = 2.0 * cell * slope_max / z_quantum
        self.slope2_max = max(_capped_floor(run * run, SLOPE2_CAP), 1)
        self.ground = torch.zeros(M, nx, ny, dtype=torch.int32, device=device)
        self.top = torch.zeros(M, nx, ny, dtype=torch.int32, device=device)
        self.weight = torch.zeros(M, nx, ny, dtype=torch.int16, device=device)
        self.prev_origin = torch.zeros(M, 2, dtype=torch.int64, device=device)
        self.cur_origin = torch.zeros(M, 2, dtype=torch.int64, device=device)
        self.initialised = torch.zeros(M, dtype=torch.int32, device=device)
        self.status_word = torch.zeros(M, dtype=torch.int32, device=device)

    def reset(self):
        """Forget everything: the next update starts from an empty map.  One fill of the flag on the current stream; it allocates
        nothing, waits for nothing and can be captured."""
        self.initialised.zero_()

    def status(self):
        """The sticky status word of every map as a list of M integers: bit SKIPPED -- an update was skipped because the pose of its
        centre was not finite or too far out for 32-bit cells; bit SENSOR_NOT_FINITE -- a frame brought a sensor position that is not
        finite and contributed nothing.  This call, alone in this module, waits for the device."""
        return [int(v) for v in self.status_word.tolist()]


def _shapes(tmap):
    return {k: (tmap.M, 2) if k == "origin" else (tmap.M, tmap.nx, tmap.ny) for k in OUTPUTS}


class TerrainWorkspace:
    """The scratch memory of update() for B frames into `tmap` and its preallocated outputs.  `out` is the dictionary update(out=)
    takes.  With workspace= and out= a call allocates nothing, so it can be captured in a graph on one stream."""

    def __init__(self, tmap, B):
        if not isinstance(tmap, TerrainMap) or int(B) <= 0 or tmap.M not in (int(B), 1):
            raise L.CrdError(f"TerrainWorkspace: a TerrainMap of B = {B} maps or of one")
        self.B = int(B)
        dev = tmap.ground.device
        self.cells = torch.empty(workspace_bytes(self.B, tmap.M, tmap.nx, tmap.ny), dtype=torch.uint8, device=dev)
        self.out = {k: torch.empty(s, dtype=OUTPUTS[k], device=dev) for k, s in _shapes(tmap).items()}


def update(tmap, cloud_or_xyz, frame_offsets=None, map_from_points=None, sensor=None, centre=None, valid=None, workspace=None, out=None):
    """One batch of clouds into the map (crd_terrain_update, five launches on the current stream).

    Every argument but the first as for occupancy.update: the three forms of a cloud, the pose of the points' frame in the map frame,
    sensor and centre in the points' frame, tmap.M == B or 1.  The same centre and pose give the same origin as the occupancy map.

    Returns, in WINDOW order -- cell [m][i][j] is world cell (origin[m][0] + i, origin[m][1] + j): 'ground' and 'top' int32 in quanta
    (INT32_MIN where unknown), 'step' int32, 'slope2' int64, 'weight' int16, 'state' uint8 (UNKNOWN, FREE, OCCUPIED), 'hazard' uint8
    (0 .. 253, LETHAL, NO_INFORMATION), 'evidence' uint8 (1: observed in this call), 'value' fp32 (the ground in metres, NaN where
    unknown), each [M,nx,ny], and 'origin' int64 [M,2].  A map whose centre is not finite is left as it was (status()).  workspace: a
    TerrainWorkspace; out: its `out`: then nothing is allocated and nothing waits for the device."""
    fn = "terrain.update"
    if not isinstance(tmap, TerrainMap):
        raise L.CrdError(f"{fn}: the first argument is a TerrainMap")
    xyz, valid, _, off, rows_per_frame, B = _rows(fn, cloud_or_xyz, frame_offsets, valid, None)
    n = xyz.shape[0]
    if valid is not None:
        valid = _dev(valid, torch.uint8, (n,), "valid")
    M, nx, ny = tmap.M, tmap.nx, tmap.ny
    if M not in (B, 1):
        raise L.CrdError(f"{fn}: {M} maps for {B} frames: M is B (one map per frame) or 1 (one map for all)")
    T, t_stride = None, 0
    if map_from_points is not None:
        per_frame = torch.is_tensor(map_from_points) and map_from_points.dim() == 3
        T = _dev(map_from_points, torch.float64, (B, 3, 4) if per_frame else (3, 4), "map_from_points")
        t_stride = 12 if per_frame else 0
    sensor, s_stride = _point(sensor, B, "sensor")
    centre, c_stride = _point(centre, B, "centre")
    dev = xyz.device
    if tmap.ground.device != dev:
        raise L.CrdError(f"{fn}: the map lives on {tmap.ground.device}, the cloud on {dev}")
    need = workspace_bytes(B, M, nx, ny)
    if workspace is None:
        cells = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        if not isinstance(workspace, TerrainWorkspace):
            raise L.CrdError(f"{fn}: workspace= is a TerrainWorkspace")
        cells = workspace.cells
        if cells.numel() < need:
            raise L.CrdError(f"{fn}: the workspace holds {cells.numel()} bytes, {need} are needed (B {B}, {M} maps of {nx} x {ny})")
    shapes = _shapes(tmap)
    if out is None:
        out = {k: torch.empty(shapes[k], dtype=t, device=dev) for k, t in OUTPUTS.items()}
    else:
        if not isinstance(out, dict) or set(out) != set(OUTPUTS):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(OUTPUTS)}")
        out = {k: _dev(out[k], t, shapes[k], f"out['{k}']") for k, t in OUTPUTS.items()}
    b = L.f64_bits
    L.check(L.load().crd_terrain_update(L.ptr(xyz), L.ptr(valid), L.ptr(off), rows_per_frame, B, n, L.ptr(T), t_stride, L.ptr(sensor),
                                        s_stride, L.ptr(centre), c_stride, M, nx, ny, b(tmap.cell), b(tmap.z_quantum), b(tmap.z_range[0]),
                                        b(tmap.z_range[1]), b(tmap.max_range), tmap.head_q, tmap.min_points, tmap.w_max, tmap.step_max_q,
                                        tmap.slope2_max, L.ptr(tmap.ground), L.ptr(tmap.top), L.ptr(tmap.weight), L.ptr(tmap.prev_origin),
                                        L.ptr(tmap.cur_origin), L.ptr(tmap.initialised), L.ptr(tmap.status_word), L.ptr(cells),
                                        cells.numel(), *(L.ptr(out[k]) for k in OUTPUTS), L.stream()), "crd_terrain_update")
    return out


def picture(result, z_range, cmap="jet", bad_colour=(0, 0, 0), out=None, workspace=None):
    """The ground height result['value'] in the colours of cmap -> uint8 RGB [M,nx,ny,3]: viz.colorize over the fixed range z_range
    in metres, which needs no reduction; unknown cells (NaN) in bad_colour.  out and workspace as for viz.colorize."""
    if not isinstance(result, dict) or "value" not in result:
        raise L.CrdError("picture: result is update's dictionary")
    try:
        lo, hi = (float(v) for v in z_range)
    except (TypeError, ValueError):
        raise L.CrdError(f"picture: z_range {z_range!r} is two numbers") from None
    return viz.colorize(result["value"], cmap, vmin=lo, vmax=hi, bad_colour=bad_colour, out=out, workspace=workspace)
