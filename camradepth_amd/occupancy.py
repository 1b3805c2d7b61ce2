"""GPU occupancy map: point clouds -> free / occupied / unknown per cell, fused over frames while the vehicle moves.

The step after bev.bev_grid, whose `occupancy` is one frame's count and knows neither "seen and empty" nor the frame before.  An
OccupancyMap holds int16 log-odds for a world-aligned window of nx x ny cells that follows the vehicle by whole cells; it is stored as
a torus, so moving it copies nothing.  `update` feeds it one batch of clouds: a cell with enough points in the obstacle band is
occupied, a cell whose centre lies nearer than the first obstacle on its bearing from the sensor and no farther than something seen
there is free, everything else keeps what it had.  The window's origin is computed on the device from the pose, so nothing waits for
the host.  All arithmetic is fp64 add, multiply, divide, floor and compare on the device, specified operation by operation in
include/camradepth_hip.h and the same bits every run: INTEGRATION.md, "Occupancy map".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from . import viz
from ._frontend import _dev, _rows

OUTPUTS = {"log_odds": torch.int16, "state": torch.uint8, "evidence": torch.uint8, "value": torch.float32, "origin": torch.int64}
# z_floor, z_lo, z_hi: heights in the map frame (z up, 0 on the road under the vehicle) -- seen from z_floor, an obstacle from z_lo
MAP_OPTIONS = {"n_bins": 720, "max_range": 80.0, "z_floor": -math.inf, "z_lo": 0.3, "z_hi": 2.5, "min_points": 2, "l_occ": 6, "l_free": 2,
               "l_max": 60, "occupied_at": 12, "free_at": 6}
UNKNOWN, FREE, OCCUPIED = 0, 1, 2                    # 'state' and 'evidence'
SKIPPED, SENSOR_NOT_FINITE = 1, 2                    # bits of the status word


def workspace_bytes(B, n_bins, M, nx, ny):
    """include/camradepth_hip.h, crd_occupancy_update: two uint64 key tables of B * n_bins bins, B sensor positions, the hit counts of
    M * nx * ny cells and M flags, each from a 16-byte boundary."""
    def up(n):
        return (n + 15) & ~15
    return 2 * up(8 * B * n_bins) + up(24 * B) + up(4 * M * nx * ny) + up(4 * M)


def _whole(v, what):
    try:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise L.CrdError(f"OccupancyMap: {what} must be an integer, not {v!r}") from None
    return int(v)


class OccupancyMap:
    """M maps of nx x ny cells of `cell` metres in a fixed map frame, with everything update() needs to know about them.

    n_bins: bearing bins around the sensor (a multiple of 4, 4 .. 65536).  max_range: points farther from the sensor (in x, y) are left
    out.  A point with z_floor <= Z <= z_hi was seen, one with z_lo <= Z <= z_hi is an obstacle (z_floor <= z_lo: the road counts as
    seen, not as an obstacle).  min_points obstacle points make a cell occupied.  The log-odds of a cell rise by l_occ when occupied,
    fall by l_free when free, and stay within +-l_max (integers, 1 <= l_occ, l_free <= l_max <= 32767); its state is OCCUPIED from
    occupied_at up, FREE from -free_at down, UNKNOWN between (each 1 .. l_max).

    State on the device: `log_odds` int16 [M,nx,ny] (the torus: world cell (wx, wy) in slot (wx mod nx, wy mod ny)), `prev_origin` and
    `cur_origin` int64 [M,2], `initialised` int32 [M], `status_word` int32 [M]."""

    def __init__(self, M, nx, ny, cell, n_bins=720, max_range=80.0, z_floor=-math.inf, z_lo=0.3, z_hi=2.5, min_points=2, l_occ=6, l_free=2,
                 l_max=60, occupied_at=12, free_at=6, device="cuda"):
        fn = "OccupancyMap"
        M, nx, ny, n_bins, min_points = (_whole(v, k) for k, v in (("M", M), ("nx", nx), ("ny", ny), ("n_bins", n_bins), ("min_points", min_points)))
        l_occ, l_free, l_max, occupied_at, free_at = (_whole(v, k) for k, v in (("l_occ", l_occ), ("l_free", l_free), ("l_max", l_max),
                                                                               ("occupied_at", occupied_at), ("free_at", free_at)))
        try:
            cell, max_range, z_floor, z_lo, z_hi = (float(v) for v in (cell, max_range, z_floor, z_lo, z_hi))
        except (TypeError, ValueError):
            raise L.CrdError(f"{fn}: cell, max_range, z_floor, z_lo and z_hi are numbers") from None
        if M <= 0 or not 1 <= nx <= 65535 or not 1 <= ny <= 65535 or M * nx * ny >= 2 ** 31:
            raise L.CrdError(f"{fn}: M {M} maps of {nx} x {ny} cells (M >= 1, each side 1 .. 65535, fewer than 2^31 cells)")
        if not (cell > 0 and math.isfinite(cell)):
            raise L.CrdError(f"{fn}: cell {cell} is not a finite positive size")
        if not 4 <= n_bins <= 65536 or n_bins % 4:
            raise L.CrdError(f"{fn}: n_bins {n_bins} is not a multiple of 4 in 4 .. 65536")
        if not (max_range > 0 and math.isfinite(max_range * max_range)):
            raise L.CrdError(f"{fn}: max_range {max_range} must be positive, with a finite square")
        if not z_floor <= z_lo <= z_hi:
            raise L.CrdError(f"{fn}: z_floor {z_floor}, z_lo {z_lo}, z_hi {z_hi}: no NaN, z_floor <= z_lo <= z_hi")
        if min_points < 1:
            raise L.CrdError(f"{fn}: min_points must be an integer >= 1, not {min_points}")
        if not (1 <= l_occ <= l_max and 1 <= l_free <= l_max and l_max <= 32767):
            raise L.CrdError(f"{fn}: l_occ {l_occ}, l_free {l_free}, l_max {l_max}: 1 <= l_occ, l_free <= l_max <= 32767")
        if not (1 <= occupied_at <= l_max and 1 <= free_at <= l_max):
            raise L.CrdError(f"{fn}: occupied_at {occupied_at}, free_at {free_at}: each is 1 .. l_max {l_max}")
        self.M, self.nx, self.ny, self.cell, self.n_bins, self.max_range = M, nx, ny, cell, n_bins, max_range
        self.z_floor, self.z_lo, self.z_hi, self.min_points = z_floor, z_lo, z_hi, min_points
        self.l_occ, self.l_free, self.l_max, self.occupied_at, self.free_at = l_occ, l_free, l_max, occupied_at, free_at
        self.log_odds = torch.zeros(M, nx, ny, dtype=torch.int16, device=device)
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


class OccupancyWorkspace:
    """The scratch memory of update() for B frames into `omap` and its preallocated outputs.  `out` is the dictionary update(out=)
    takes.  With workspace= and out= a call allocates nothing, so it can be captured in a graph on one stream."""

    def __init__(self, omap, B):
        if not isinstance(omap, OccupancyMap) or int(B) <= 0 or omap.M not in (int(B), 1):
            raise L.CrdError(f"OccupancyWorkspace: an OccupancyMap of B = {B} maps or of one")
        self.B = int(B)
        M, nx, ny, dev = omap.M, omap.nx, omap.ny, omap.log_odds.device
        self.keys = torch.empty(workspace_bytes(self.B, omap.n_bins, M, nx, ny), dtype=torch.uint8, device=dev)
        self.out = {k: torch.empty((M, 2) if k == "origin" else (M, nx, ny), dtype=t, device=dev) for k, t in OUTPUTS.items()}


def _point(v, B, what):
    """-> (tensor or None, stride): one fp64 point for every frame, or one per frame."""
    if v is None:
        return None, 0
    if torch.is_tensor(v) and v.dim() == 2:
        return _dev(v, torch.float64, (B, 3), what), 3
    return _dev(v, torch.float64, (3,), what), 0


def update(omap, cloud_or_xyz, frame_offsets=None, map_from_points=None, sensor=None, centre=None, valid=None, workspace=None, out=None):
    """One batch of clouds into the map (crd_occupancy_update, three launches on the current stream).

    cloud_or_xyz, frame_offsets, valid: the three forms bev_grid takes.  map_from_points: fp64 [3,4] or [B,3,4] on the device, the
    pose of the points' frame in the map frame; None: the identity.  sensor, centre: fp64 [3] or [B,3] on the device IN THE POINTS'
    FRAME, taken through the same transform: where the rays start (None: the origin) and the point the window is centred on (None:
    the sensor; e.g. 20 m ahead of it).  omap.M == B: frame b feeds map b; omap.M == 1: all frames feed the one map -- the cameras of
    one rig -- and its centre is frame 0's.

    Returns, in WINDOW order -- cell [m][i][j] is world cell (origin[m][0] + i, origin[m][1] + j), which covers (origin[m][0] + i) *
    cell <= X < .. + cell: 'log_odds' int16, 'state' uint8 (UNKNOWN, FREE, OCCUPIED), 'evidence' uint8 (this call's alone), 'value'
    fp32 (the log-odds, for a picture), each [M,nx,ny], and 'origin' int64 [M,2].  A map whose centre is not finite is left as it was
    (status()).  workspace: an OccupancyWorkspace; out: its `out`: then nothing is allocated and nothing waits for the device."""
    fn = "occupancy.update"
    if not isinstance(omap, OccupancyMap):
        raise L.CrdError(f"{fn}: the first argument is an OccupancyMap")
    xyz, valid, _, off, rows_per_frame, B = _rows(fn, cloud_or_xyz, frame_offsets, valid, None)
    n = xyz.shape[0]
    if valid is not None:
        valid = _dev(valid, torch.uint8, (n,), "valid")
    M, nx, ny = omap.M, omap.nx, omap.ny
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
    if omap.log_odds.device != dev:
        raise L.CrdError(f"{fn}: the map lives on {omap.log_odds.device}, the cloud on {dev}")
    need = workspace_bytes(B, omap.n_bins, M, nx, ny)
    if workspace is None:
        keys = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        keys = workspace.keys
        if keys.numel() < need:
            raise L.CrdError(f"{fn}: the workspace holds {keys.numel()} bytes, {need} are needed (B {B}, {omap.n_bins} bins, {M} maps of "
                             f"{nx} x {ny})")
    shapes = {k: (M, 2) if k == "origin" else (M, nx, ny) for k in OUTPUTS}
    if out is None:
        out = {k: torch.empty(shapes[k], dtype=t, device=dev) for k, t in OUTPUTS.items()}
    else:
        if not isinstance(out, dict) or set(out) != set(OUTPUTS):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(OUTPUTS)}")
        out = {k: _dev(out[k], t, shapes[k], f"out['{k}']") for k, t in OUTPUTS.items()}
    b = L.f64_bits
    L.check(L.load().crd_occupancy_update(L.ptr(xyz), L.ptr(valid), L.ptr(off), rows_per_frame, B, n, L.ptr(T), t_stride, L.ptr(sensor),
                                          s_stride, L.ptr(centre), c_stride, M, nx, ny, b(omap.cell), omap.n_bins, b(omap.max_range),
                                          b(omap.z_floor), b(omap.z_lo), b(omap.z_hi), omap.min_points, omap.l_occ, omap.l_free, omap.l_max,
                                          omap.occupied_at, omap.free_at, L.ptr(omap.log_odds), L.ptr(omap.prev_origin),
                                          L.ptr(omap.cur_origin), L.ptr(omap.initialised), L.ptr(omap.status_word), L.ptr(keys),
                                          keys.numel(), L.ptr(out["log_odds"]), L.ptr(out["state"]), L.ptr(out["evidence"]),
                                          L.ptr(out["value"]), L.ptr(out["origin"]), L.stream()), "crd_occupancy_update")
    return out


def picture(result, l_max, cmap="jet", out=None, workspace=None):
    """The log-odds result['value'] in the colours of cmap -> uint8 RGB [M,nx,ny,3]: viz.colorize over the fixed range -l_max ..
    l_max, which needs no reduction (l_max: the number, or the OccupancyMap that has it).  out and workspace as for viz.colorize."""
    if not isinstance(result, dict) or "value" not in result:
        raise L.CrdError("picture: result is update's dictionary")
    try:
        hi = float(getattr(l_max, "l_max", l_max))
    except (TypeError, ValueError):
        raise L.CrdError(f"picture: l_max {l_max!r} is a number or an OccupancyMap") from None
    return viz.colorize(result["value"], cmap, vmin=-hi, vmax=hi, out=out, workspace=workspace)
