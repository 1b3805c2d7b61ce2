"""GPU local planner: velocity candidates rolled out on the costmap, against the predicted object tracks and towards the cost-to-go.

The stage behind field.distance_field, nav.nav_field and tracks.track_objects, and the one that turns the map into a command: the local
planner of ROS base_local_planner / dwa_local_planner (the dynamic window approach: Fox, Burgard, Thrun 1997).  plan_rollouts takes K =
n_v x n_w velocity candidates (v, w), rolls each out over P poses of a circular arc from the vehicle's pose, rejects the rollouts that
meet a blocked cell of the costmap or come within keep_out of where a counting track will be at that time, scores the rest by the
cost-to-go at their end and the costs along them, and picks the least.  The arcs are a table made on the host (RolloutSpec), so the
device never evaluates a sine, a cosine or a square root; every decision is an integer or the least element of a total order, specified
operation by operation in include/camradepth_hip.h and the same bits every run: INTEGRATION.md, "Local planner".  Nothing calls this
module unless asked."""
import math

import torch

from . import lib as L
from . import tracks as trk
from ._frontend import _dev
from .field import _whole

MAX_V, MAX_W, MAX_K, MAX_POSES, MAX_WEIGHT = 64, 129, 4096, 256, 32767
NOT_FINITE, NO_CANDIDATE = 1, 2                                          # bits of info[:, STATUS]
N_ADMISSIBLE, N_CLEAR_STATIC, N_CLEAR, N_VALID, STATUS = range(5)        # the columns of 'info'
UNREACHED = 0x7FFFFFFF                                                   # nav.UNREACHED: 'end_togo' of a rollout that ends outside
OUTPUTS = {"best": torch.int32, "command": torch.float64, "score": torch.int64, "info": torch.int32}
TABLES = {"scores": torch.int64, "first_blocked": torch.int32, "first_track": torch.int32, "max_cost": torch.int32, "end_togo": torch.int32}
WEIGHTS = {"togo": 1, "max_cost": 0, "sum_cost": 1, "slow": 0, "turn": 0}
SPEC_OPTIONS = {"v": (0.0, 2.0, 8), "w": (1.0, 17), "dt": 0.1, "n_poses": 32, "track_dt": None, "keep_out": 0.0, "min_speed": 0.0,
                "max_object_cells": 64, "min_status": trk.CONFIRMED, "accel": None, "blocked_at": 253, "outside_blocks": True,
                "weights": WEIGHTS, "cell": None}


def workspace_bytes(M, K):
    """include/camradepth_hip.h, crd_plan_rollouts: a record of 32 bytes per candidate and map."""
    return 32 * M * K


def _number(v, what, fn):
    try:
        if isinstance(v, bool):
            raise TypeError
        return float(v)
    except (TypeError, ValueError):
        raise L.CrdError(f"{fn}: {what} is a number, not {v!r}") from None


def _seq(v, n, what, fn):
    try:
        v = tuple(v)
    except TypeError:
        v = ()
    if len(v) != n:
        raise L.CrdError(f"{fn}: {what} holds {n} values, not {v!r}")
    return v


def candidates(v_min, v_max, n_v, w_max, n_w):
    """-> the K = n_v * n_w candidates (v_k, w_k), k = iv * n_w + iw, as a list of pairs of Python floats.  The centre column has w
    exactly 0."""
    c = (n_w - 1) // 2
    rows = []
    for iv in range(n_v):
        v = v_min if n_v == 1 else v_min + iv * (v_max - v_min) / (n_v - 1)
        for iw in range(n_w):
            rows.append((v, 0.0 if iw == c else (iw - c) * w_max / c))
    return rows


def arc_table(vw, dt, n_poses):
    """-> [K][P][2] as nested lists: the pose of candidate (v, w) at time t = (p + 1) * dt in the vehicle's frame, x forward and y left.
    w == 0: exactly (v * t, 0.0); otherwise the arc (v / w * sin(w t), v / w * (1 - cos(w t))) by math.sin and math.cos."""
    rows = []
    for v, w in vw:
        row = []
        for p in range(n_poses):
            t = (p + 1) * dt
            if w == 0.0:
                row.append((v * t, 0.0))
            else:
                r = v / w
                row.append((r * math.sin(w * t), r * (1.0 - math.cos(w * t))))
        rows.append(row)
    return rows


class RolloutSpec:
    """The candidates of the local planner, its tests and its weights, checked on the host, and its three tables on the device.

    v = (v_min, v_max, n_v): n_v 1 .. 64 forward speeds from v_min to v_max, finite, v_min <= v_max (metres per second).  w = (w_max,
    n_w): n_w turn rates from -w_max to w_max, n_w odd and 1 .. 129, w_max finite and >= 0 (radians per second, positive to the left); K
    = n_v * n_w <= 4096.  dt: seconds between two poses, finite and positive; n_poses: P, 1 .. 256.  track_dt: seconds per track update
    (None: dt), finite and positive.  keep_out: metres, a pose this close to a counting track's predicted position is hit.  A track
    counts with a status >= min_status (tracks.TENTATIVE or CONFIRMED), at most max_object_cells cells and a speed of at least
    min_speed metres per update.  accel = (a_v, a_w): the accelerations that bound the dynamic window around run-time's twist, finite
    and >= 0; None: no window.  blocked_at, outside_blocks: as for field.check_paths.  weights: integers 0 .. 32767 under 'togo',
    'max_cost', 'sum_cost', 'slow' and 'turn'; names left out keep their defaults.  cell: metres per cell, the map's; None: plan_rollouts
    takes that of its tracks=.

    `vw` fp64 [K,2], `arc` fp64 [K,P,2] and `tau` fp64 [P] = (p + 1) * dt / track_dt live on `device`."""

    def __init__(self, v=(0.0, 2.0, 8), w=(1.0, 17), dt=0.1, n_poses=32, track_dt=None, keep_out=0.0, min_speed=0.0, max_object_cells=64,
                 min_status=trk.CONFIRMED, accel=None, blocked_at=253, outside_blocks=True, weights=None, cell=None, device="cuda"):
        fn = "RolloutSpec"
        self.cell = None if cell is None else _number(cell, "cell", fn)
        if self.cell is not None and not (self.cell > 0 and math.isfinite(self.cell)):
            raise L.CrdError(f"{fn}: cell {cell} is not a finite positive size")
        v, w = _seq(v, 3, "v = (v_min, v_max, n_v)", fn), _seq(w, 2, "w = (w_max, n_w)", fn)
        self.v_min, self.v_max, self.w_max = _number(v[0], "v_min", fn), _number(v[1], "v_max", fn), _number(w[0], "w_max", fn)
        self.n_v, self.n_w, self.n_poses = _whole(v[2], "n_v", fn), _whole(w[1], "n_w", fn), _whole(n_poses, "n_poses", fn)
        self.dt = _number(dt, "dt", fn)
        self.track_dt = self.dt if track_dt is None else _number(track_dt, "track_dt", fn)
        self.keep_out, self.min_speed = _number(keep_out, "keep_out", fn), _number(min_speed, "min_speed", fn)
        self.max_object_cells, self.min_status = _whole(max_object_cells, "max_object_cells", fn), _whole(min_status, "min_status", fn)
        self.blocked_at, self.outside_blocks = _whole(blocked_at, "blocked_at", fn), bool(outside_blocks)
        if not (math.isfinite(self.v_min) and math.isfinite(self.v_max) and self.v_min <= self.v_max):
            raise L.CrdError(f"{fn}: v_min {v[0]} and v_max {v[1]} are not finite with v_min <= v_max")
        if not 1 <= self.n_v <= MAX_V:
            raise L.CrdError(f"{fn}: n_v {self.n_v} is not in 1 .. {MAX_V}")
        if not (math.isfinite(self.w_max) and self.w_max >= 0):
            raise L.CrdError(f"{fn}: w_max {w[0]} is negative or not finite")
        if not (1 <= self.n_w <= MAX_W and self.n_w % 2 == 1):
            raise L.CrdError(f"{fn}: n_w {self.n_w} is not odd and in 1 .. {MAX_W}")
        self.K = self.n_v * self.n_w
        if self.K > MAX_K:
            raise L.CrdError(f"{fn}: n_v * n_w = {self.K} candidates; at most {MAX_K}")
        if not 1 <= self.n_poses <= MAX_POSES:
            raise L.CrdError(f"{fn}: n_poses {self.n_poses} is not in 1 .. {MAX_POSES}")
        if not (self.dt > 0 and math.isfinite(self.dt)):
            raise L.CrdError(f"{fn}: dt {dt} is not finite and positive")
        if not (self.track_dt > 0 and math.isfinite(self.track_dt)):
            raise L.CrdError(f"{fn}: track_dt {track_dt} is not finite and positive")
        for name, x in (("keep_out", self.keep_out), ("min_speed", self.min_speed)):
            if not (x >= 0 and math.isfinite(x) and math.isfinite(x * x)):
                raise L.CrdError(f"{fn}: {name} {x} is not finite and >= 0 with a finite square")
        if not 0 <= self.max_object_cells < 2 ** 31:
            raise L.CrdError(f"{fn}: max_object_cells {max_object_cells} is not in 0 .. 2^31 - 1")
        if self.min_status not in (trk.TENTATIVE, trk.CONFIRMED):
            raise L.CrdError(f"{fn}: min_status {min_status} is neither tracks.TENTATIVE nor tracks.CONFIRMED")
        if not 1 <= self.blocked_at <= 255:
            raise L.CrdError(f"{fn}: blocked_at {blocked_at} is not in 1 .. 255")
        self.accel = None
        if accel is not None:
            a = _seq(accel, 2, "accel = (a_v, a_w)", fn)
            self.accel = (_number(a[0], "accel a_v", fn), _number(a[1], "accel a_w", fn))
            if not all(x >= 0 and math.isfinite(x) for x in self.accel):
                raise L.CrdError(f"{fn}: accel {accel!r} holds a value that is negative or not finite")
        if weights is not None and (not isinstance(weights, dict) or not set(weights) <= set(WEIGHTS)):
            raise L.CrdError(f"{fn}: weights holds {sorted(WEIGHTS)}, not {weights!r}")
        self.weights = {k: _whole(x, f"weights['{k}']", fn) for k, x in dict(WEIGHTS, **(weights or {})).items()}
        for k, x in self.weights.items():
            if not 0 <= x <= MAX_WEIGHT:
                raise L.CrdError(f"{fn}: weights['{k}'] {x} is not in 0 .. {MAX_WEIGHT}")
        self.keep_out2, self.min_speed2 = self.keep_out * self.keep_out, self.min_speed * self.min_speed
        self.a_v_dt, self.a_w_dt = (0.0, 0.0) if self.accel is None else (self.accel[0] * self.dt, self.accel[1] * self.dt)
        rows = candidates(self.v_min, self.v_max, self.n_v, self.w_max, self.n_w)
        self.vw = torch.tensor(rows, dtype=torch.float64).view(self.K, 2).to(device)
        self.arc = torch.tensor(arc_table(rows, self.dt, self.n_poses), dtype=torch.float64).view(self.K, self.n_poses, 2).to(device)
        self.tau = torch.tensor([(p + 1) * self.dt / self.track_dt for p in range(self.n_poses)], dtype=torch.float64).to(device)


def _spec(spec, fn):
    if not isinstance(spec, RolloutSpec):
        raise L.CrdError(f"{fn}: the first argument is a RolloutSpec")
    return spec


def _shapes(spec, M, tables, xy):
    K = spec.K
    shapes = {"best": (M,), "command": (M, 2), "score": (M,), "info": (M, 8)}
    if tables:
        shapes.update({k: (M, K) for k in TABLES})
    if xy:
        shapes["xy"] = (M, K, spec.n_poses, 2)
    return shapes


def _dtype(k):
    return OUTPUTS.get(k, TABLES.get(k, torch.float64))


class RolloutWorkspace:
    """The scratch memory of plan_rollouts for M maps and its preallocated outputs: `buf`, workspace_bytes(M, K) bytes, and `out`, the
    dictionary plan_rollouts(out=) takes, with the per-candidate tables when tables=True and 'xy' when xy=True.  With workspace= a call
    allocates nothing, so it can be captured in a graph on one stream."""

    def __init__(self, spec, M, tables=False, xy=False):
        fn = "RolloutWorkspace"
        _spec(spec, fn)
        M = _whole(M, "M", fn)
        if not 1 <= M <= 65535:
            raise L.CrdError(f"{fn}: M {M} maps; 1 .. 65535")
        self.M, self.K, self.P, self.tables, self.xy = M, spec.K, spec.n_poses, bool(tables), bool(xy)
        dev = spec.vw.device
        self.buf = torch.empty(workspace_bytes(M, spec.K), dtype=torch.uint8, device=dev)
        self.out = {k: torch.empty(s, dtype=_dtype(k), device=dev) for k, s in _shapes(spec, M, tables, xy).items()}


def plan_rollouts(spec, pose, field_result, map_or_state_origin, nav_result=None, tracks=None, twist=None, workspace=None, out=None,
                  tables=False, xy=False):
    """The velocity command of M vehicles, one per map (crd_plan_rollouts, two launches on the current stream).

    pose: fp64 [M,3,4] on the device, the map-from-vehicle pose: what match.match_scan returns as 'pose' and what occupancy.update
    takes.  field_result: distance_field's dictionary with its 'cost'; map_or_state_origin: occupancy.update's dictionary or (state,
    origin), exactly as for field.check_paths; the origin is read on the device.  nav_result: nav.nav_field's dictionary, whose 'togo'
    is used; None drops the cost-to-go term.  tracks: a tracks.ObjectTracks of M maps, or None.  twist: fp64 [M,2] on the device, the
    current (v, w); with the spec's accel = (a_v, a_w) a candidate is admissible when |v_k - v| <= a_v * dt and |w_k - w| <= a_w * dt;
    None: every candidate is.

    Returns 'best' int32 [M] (the picked k = iv * n_w + iw, or -1), 'command' fp64 [M,2] (spec.vw[best], or exactly (0.0, 0.0): the
    vehicle stops), 'score' int64 [M] and 'info' int32 [M,8] (n_admissible, n_clear_static, n_clear, n_valid, status with the bits
    NOT_FINITE and NO_CANDIDATE, 0, 0, 0); with tables=True also 'scores' int64 and 'first_blocked', 'first_track', 'max_cost', 'end_togo'
    int32, each [M,K]; with xy=True also 'xy' fp64 [M,K,P,2], the rollouts in the map frame, of which field.check_paths takes a map's
    as they are.  workspace: a RolloutWorkspace (its `out` is then the default of out=); out: a dictionary of exactly these: then
    nothing is allocated and nothing waits for the device."""
    fn = "rollout.plan_rollouts"
    _spec(spec, fn)
    pose = _dev(pose, torch.float64, (None, 3, 4), "pose")
    M, dev = pose.shape[0], pose.device
    if not 1 <= M <= 65535:
        raise L.CrdError(f"{fn}: pose holds M {M} poses; 1 .. 65535")
    if not isinstance(field_result, dict) or field_result.get("cost") is None:
        raise L.CrdError(f"{fn}: field_result is distance_field's dictionary with its 'cost'")
    if isinstance(map_or_state_origin, dict) and "state" in map_or_state_origin and "origin" in map_or_state_origin:
        origin = map_or_state_origin["origin"]
    elif isinstance(map_or_state_origin, (tuple, list)) and len(map_or_state_origin) == 2:
        origin = map_or_state_origin[1]
    else:
        raise L.CrdError(f"{fn}: the fourth argument is occupancy.update's dictionary or (state, origin)")
    cost = _dev(field_result["cost"], torch.uint8, (M, None, None), "field_result['cost']")
    nx, ny = cost.shape[1:]
    origin = _dev(origin, torch.int64, (M, 2), "origin")
    togo = None
    if nav_result is not None:
        if not isinstance(nav_result, dict) or nav_result.get("togo") is None:
            raise L.CrdError(f"{fn}: nav_result is nav_field's dictionary with its 'togo'")
        togo = _dev(nav_result["togo"], torch.int32, (M, nx, ny), "nav_result['togo']")
    rows = pos = vel = None
    T = 0
    if tracks is not None:
        if not isinstance(tracks, trk.ObjectTracks) or tracks.M != M:
            raise L.CrdError(f"{fn}: tracks is an ObjectTracks of M = {M} maps, not {getattr(tracks, 'M', tracks)!r}")
        T = tracks.max_tracks
        rows = _dev(tracks.tracks, torch.int32, (M, T, 8), "tracks.tracks")
        pos, vel = _dev(tracks.pos, torch.float64, (M, T, 2), "tracks.pos"), _dev(tracks.vel, torch.float64, (M, T, 2), "tracks.vel")
    if twist is not None:
        if spec.accel is None:
            raise L.CrdError(f"{fn}: twist goes with a spec of accel=(a_v, a_w), which bounds the window around it")
        twist = _dev(twist, torch.float64, (M, 2), "twist")
    if spec.vw.device != dev:
        raise L.CrdError(f"{fn}: the spec's tables live on {spec.vw.device}, the pose on {dev}")
    cell = spec.cell if spec.cell is not None else getattr(tracks, "cell", None)
    if cell is None:
        raise L.CrdError(f"{fn}: the map's cell is not known: RolloutSpec(cell=), or tracks=, which bring it")
    if tracks is not None and tracks.cell != cell:
        raise L.CrdError(f"{fn}: the spec's cell {cell} is not the tracks' {tracks.cell}")
    K, P = spec.K, spec.n_poses
    vw, arc, tau = _dev(spec.vw, torch.float64, (K, 2), "spec.vw"), _dev(spec.arc, torch.float64, (K, P, 2), "spec.arc"), \
        _dev(spec.tau, torch.float64, (P,), "spec.tau")
    need = workspace_bytes(M, K)
    if workspace is None:
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        if not isinstance(workspace, RolloutWorkspace) or (workspace.M, workspace.K, workspace.P) != (M, K, P):
            raise L.CrdError(f"{fn}: the workspace was made for {getattr(workspace, 'M', None)} maps, {getattr(workspace, 'K', None)} "
                             f"candidates and {getattr(workspace, 'P', None)} poses, these are {M}, {K} and {P}")
        buf = workspace.buf
        if buf.numel() < need:
            raise L.CrdError(f"{fn}: the workspace holds {buf.numel()} bytes, {need} are needed (M {M}, K {K})")
        out = workspace.out if out is None else out
    shapes = _shapes(spec, M, tables, xy)
    if out is None:
        out = {k: torch.empty(s, dtype=_dtype(k), device=dev) for k, s in shapes.items()}
    else:
        if not isinstance(out, dict) or not set(shapes) <= set(out) <= set(shapes) | set(TABLES) | {"xy"}:
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(shapes)}")
        out = {k: _dev(out[k], _dtype(k), s, f"out['{k}']") for k, s in shapes.items()}
    b, w = L.f64_bits, spec.weights
    L.check(L.load().crd_plan_rollouts(L.ptr(pose), L.ptr(vw), L.ptr(arc), L.ptr(tau), M, spec.n_v, spec.n_w, P, L.ptr(origin),
                                       b(cell), L.ptr(cost), L.ptr(togo), nx, ny,
                                       spec.blocked_at, 1 if spec.outside_blocks else 0, L.ptr(rows), L.ptr(pos), L.ptr(vel), T,
                                       spec.min_status, spec.max_object_cells, b(spec.min_speed2), b(spec.keep_out2), L.ptr(twist),
                                       b(spec.a_v_dt), b(spec.a_w_dt), w["togo"], w["max_cost"], w["sum_cost"], w["slow"], w["turn"],
                                       L.ptr(buf), buf.numel(), L.ptr(out["best"]), L.ptr(out["command"]), L.ptr(out["score"]),
                                       L.ptr(out["info"]), *(L.ptr(out.get(k)) for k in TABLES), L.ptr(out.get("xy")), L.stream()),
            "crd_plan_rollouts")
    return out
