"""GPU scan matcher: the pose of a cloud corrected against the occupancy map before the cloud is fused into it.

The stage in front of occupancy.update, which fuses frames by the pose it is given and by nothing else: a heading error of half a
degree moves a wall 40 m out by two cells of 0.2 m and smears it.  match_scan scores a small window of turns about the sensor and
whole-cell shifts of the cloud's obstacle cells against the map's int16 log-odds as it stands (correlative scan matching: Olson, ICRA
2009) and returns the pose of the best candidate, fp64 [B,3,4], which update takes as it is.  The map is read only.  The score is a
sum of integers and the pick the least element of a total order, so the bits are the same every run; the entry is specified
operation by operation in include/camradepth_hip.h: INTEGRATION.md, "Scan matching".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from ._frontend import _dev, _rows
from .field import _whole
from .occupancy import OccupancyMap, _point

MAX_XY, MAX_THETA = 16, 32
UNINITIALISED, NOT_FINITE, FEW_CELLS, LOW_SCORE, ON_BORDER = 1, 2, 4, 8, 16          # bits of 'status'
KEEPS_PRIOR = UNINITIALISED | NOT_FINITE | FEW_CELLS | LOW_SCORE
OUTPUTS = {"pose": torch.float64, "pick": torch.int32, "score": torch.int64, "prior_score": torch.int64, "n_cells": torch.int32,
           "status": torch.int32}
SPEC_OPTIONS = {"n_xy": 4, "n_theta": 4, "d_theta": math.radians(0.25), "min_points": None, "min_cells": 8, "min_score": 1}


def workspace_bytes(B, M, nx, ny, n_xy, n_theta):
    """include/camradepth_hip.h, crd_match_scan: the candidate poses of B frames and NT turns, B sensor positions, the count grids of
    M maps and NT turns, grown by n_xy cells on every side, and the score table, each from a 16-byte boundary."""
    def up(n):
        return (n + 15) & ~15
    nt, ns = 2 * n_theta + 1, 2 * n_xy + 1
    return up(96 * B * nt) + up(24 * B) + up(4 * M * nt * (nx + 2 * n_xy) * (ny + 2 * n_xy)) + up(8 * M * nt * ns * ns)


class MatchSpec:
    """The search window of the matcher and its guards, checked on the host.  n_xy: 0 .. 16, the shifts tried are -n_xy .. n_xy whole
    cells along each axis.  n_theta: 0 .. 32, the turns tried are -n_theta .. n_theta steps of d_theta radians (finite, positive, the
    whole range below a half turn).  min_points: the obstacle points that make a scan cell (None: the map's).  min_cells: >= 0, the scan
    cells of the prior inside the window below which the prior is kept.  min_score: an integer, the score below which it is kept.

    `rot`, fp64 [2 n_theta + 1, 2] on `device`: (cos, sin) of every turn by math.cos and math.sin; the centre row is exactly (1, 0)."""

    def __init__(self, n_xy=4, n_theta=4, d_theta=math.radians(0.25), min_points=None, min_cells=8, min_score=1, device="cuda"):
        fn = "MatchSpec"
        self.n_xy, self.n_theta, self.min_cells, self.min_score = (_whole(v, k, fn) for k, v in (
            ("n_xy", n_xy), ("n_theta", n_theta), ("min_cells", min_cells), ("min_score", min_score)))
        self.min_points = None if min_points is None else _whole(min_points, "min_points", fn)
        try:
            if isinstance(d_theta, bool):
                raise TypeError
            self.d_theta = float(d_theta)
        except (TypeError, ValueError):
            raise L.CrdError(f"{fn}: d_theta is a number, not {d_theta!r}") from None
        if not 0 <= self.n_xy <= MAX_XY:
            raise L.CrdError(f"{fn}: n_xy {n_xy} is not in 0 .. {MAX_XY}")
        if not 0 <= self.n_theta <= MAX_THETA:
            raise L.CrdError(f"{fn}: n_theta {n_theta} is not in 0 .. {MAX_THETA}")
        if not (self.d_theta > 0 and math.isfinite(self.d_theta) and self.n_theta * self.d_theta < math.pi):
            raise L.CrdError(f"{fn}: d_theta {d_theta} is not finite and positive with n_theta * d_theta below a half turn")
        if self.min_points is not None and not 1 <= self.min_points < 2 ** 31:
            raise L.CrdError(f"{fn}: min_points {min_points} is not None or in 1 .. 2^31 - 1")
        if not 0 <= self.min_cells < 2 ** 31:
            raise L.CrdError(f"{fn}: min_cells {min_cells} is not in 0 .. 2^31 - 1")
        if not -2 ** 63 <= self.min_score < 2 ** 63:
            raise L.CrdError(f"{fn}: min_score {min_score} is not a 64-bit integer")
        self.angles = [(t - self.n_theta) * self.d_theta for t in range(2 * self.n_theta + 1)]
        rows = [(1.0, 0.0) if t == self.n_theta else (math.cos(a), math.sin(a)) for t, a in enumerate(self.angles)]
        self.rot = torch.tensor(rows, dtype=torch.float64).to(device)

    def table_shape(self, M):
        return (M, 2 * self.n_theta + 1, 2 * self.n_xy + 1, 2 * self.n_xy + 1)


def _spec(spec, fn):
    if not isinstance(spec, MatchSpec):
        raise L.CrdError(f"{fn}: the second argument is a MatchSpec")
    return spec


def _shapes(spec, omap, B, scores):
    M = omap.M
    shapes = {"pose": (B, 3, 4), "pick": (M, 3), "score": (M,), "prior_score": (M,), "n_cells": (M,), "status": (M,)}
    if scores:
        shapes["scores"] = spec.table_shape(M)
    return shapes


class MatchWorkspace:
    """The scratch memory of match_scan for B frames against `omap` and its preallocated outputs: `out`, the dictionary
    match_scan(out=) takes, with 'scores' when scores=True.  With workspace= a call allocates nothing, so it can be captured in a graph
    on one stream."""

    def __init__(self, omap, spec, B, scores=False):
        fn = "MatchWorkspace"
        if not isinstance(omap, OccupancyMap) or isinstance(B, bool) or int(B) <= 0 or omap.M not in (int(B), 1):
            raise L.CrdError(f"{fn}: an OccupancyMap of B = {B} maps or of one")
        _spec(spec, fn)
        self.B, self.M, self.scores = int(B), omap.M, bool(scores)
        dev = omap.log_odds.device
        self.buf = torch.empty(workspace_bytes(self.B, omap.M, omap.nx, omap.ny, spec.n_xy, spec.n_theta), dtype=torch.uint8, device=dev)
        self.out = {k: torch.empty(s, dtype=OUTPUTS.get(k, torch.int64), device=dev) for k, s in _shapes(spec, omap, self.B, scores).items()}


def match_scan(omap, spec, cloud_or_xyz, frame_offsets=None, map_from_points=None, sensor=None, valid=None, workspace=None, out=None,
               scores=False):
    """The pose of one batch of clouds corrected against the map (crd_match_scan, four launches on the current stream).

    omap: the OccupancyMap, read only.  cloud_or_xyz, frame_offsets, valid, map_from_points (the prior pose), sensor: as for
    occupancy.update, to which the same arguments go afterwards with map_from_points=out['pose'].  omap.M == B: frame b is matched
    against map b; omap.M == 1: all frames against the one map, with one correction for all, turned about frame 0's sensor.

    Returns 'pose' fp64 [B,3,4] (the prior itself where 'status' has a bit of KEEPS_PRIOR), 'pick' int32 [M,3] (turn steps, cells in
    x, cells in y of the best candidate), 'score' and 'prior_score' int64 [M], 'n_cells' int32 [M], 'status' int32 [M] (UNINITIALISED,
    NOT_FINITE, FEW_CELLS, LOW_SCORE, ON_BORDER; this call's alone) and, with scores=True, 'scores' int64 [M, 2 n_theta + 1, 2 n_xy + 1,
    2 n_xy + 1].  workspace: a MatchWorkspace (its `out` is then the default of out=); out: a dictionary of exactly these: then nothing
    is allocated and nothing waits for the device."""
    fn = "match.match_scan"
    if not isinstance(omap, OccupancyMap):
        raise L.CrdError(f"{fn}: the first argument is an OccupancyMap")
    _spec(spec, fn)
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
    dev = xyz.device
    if omap.log_odds.device != dev:
        raise L.CrdError(f"{fn}: the map lives on {omap.log_odds.device}, the cloud on {dev}")
    rot = _dev(spec.rot, torch.float64, (2 * spec.n_theta + 1, 2), "spec.rot")
    need = workspace_bytes(B, M, nx, ny, spec.n_xy, spec.n_theta)
    if M * (2 * spec.n_theta + 1) * (nx + 2 * spec.n_xy) * (ny + 2 * spec.n_xy) >= 2 ** 31:
        raise L.CrdError(f"{fn}: {M} maps of {nx} x {ny} cells with n_xy {spec.n_xy} and n_theta {spec.n_theta} need 2^31 counts or more")
    if workspace is None:
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        if not isinstance(workspace, MatchWorkspace) or (workspace.B, workspace.M) != (B, M):
            raise L.CrdError(f"{fn}: the workspace was made for {getattr(workspace, 'B', None)} frames and {getattr(workspace, 'M', None)} "
                             f"maps, these are {B} frames and {M} maps")
        buf = workspace.buf
        if buf.numel() < need:
            raise L.CrdError(f"{fn}: the workspace holds {buf.numel()} bytes, {need} are needed (B {B}, {M} maps of {nx} x {ny}, n_xy "
                             f"{spec.n_xy}, n_theta {spec.n_theta})")
        out = workspace.out if out is None else out
    shapes = _shapes(spec, omap, B, scores)
    if out is None:
        out = {k: torch.empty(s, dtype=OUTPUTS.get(k, torch.int64), device=dev) for k, s in shapes.items()}
    else:
        if not isinstance(out, dict) or not set(shapes) <= set(out) <= set(shapes) | {"scores"}:
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(shapes)}")
        out = {k: _dev(out[k], OUTPUTS.get(k, torch.int64), s, f"out['{k}']") for k, s in shapes.items()}
    b = L.f64_bits
    min_points = omap.min_points if spec.min_points is None else spec.min_points
    L.check(L.load().crd_match_scan(L.ptr(xyz), L.ptr(valid), L.ptr(off), rows_per_frame, B, n, L.ptr(T), t_stride, L.ptr(sensor), s_stride,
                                    M, nx, ny, b(omap.cell), b(omap.max_range), b(omap.z_lo), b(omap.z_hi), min_points,
                                    L.ptr(omap.log_odds), L.ptr(omap.cur_origin), L.ptr(omap.initialised), spec.n_xy, spec.n_theta,
                                    L.ptr(rot), spec.min_cells, spec.min_score, L.ptr(buf), buf.numel(), L.ptr(out["pose"]),
                                    L.ptr(out["pick"]), L.ptr(out["score"]), L.ptr(out["prior_score"]), L.ptr(out["n_cells"]),
                                    L.ptr(out["status"]), L.ptr(out.get("scores")), L.stream()), "crd_match_scan")
    return out
