"""GPU navigation field: a costmap and goal points -> the cost-to-go of every cell and planned paths, the question the costmap exists for.

The step after field.distance_field, whose 'cost' says what standing on a cell costs.  nav_field gives, for every cell of the window,
the least cost to reach a goal over 8-connected paths of passable cells (ROS navfn / global_planner's navigation function, chamfer
weights 5 and 7 times neutral + cost) and the neighbour to step to; plan_paths follows those steps from K starts on the device and
returns the cells and their centres, which field.check_paths takes as they are.  Integers only, specified operation by operation in
include/camradepth_hip.h and the same bits every run: INTEGRATION.md, "Navigation field".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from ._frontend import _dev
from .field import _whole

UNREACHED = 0x7FFFFFFF                                # togo of an impassable cell and of a cell without a path to a goal
ON_GOAL, NO_STEP = 8, 255                             # codes of 'next' beside the neighbours 0 .. 7
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))       # (di, dj) of code n
MAX_CELLS = 1 << 19                                   # of one map: every cost-to-go then fits int32
OUTPUTS = {"togo": torch.int32, "next": torch.uint8, "info": torch.int32}
OPTIONAL = ("next",)                                  # out= may hold None for it: the launch is then left out
PATH_OUTPUTS = {"cells": torch.int32, "n_cells": torch.int32, "start_togo": torch.int32, "status": torch.int32}
SPEC_OPTIONS = {"neutral": 50, "blocked_at": 253, "max_rounds": 64}
ENDED_ON_GOAL, CUT_AT_P, NO_START, START_UNREACHED = 0, 1, 2, 3


class NavSpec:
    """The numbers of a navigation field, checked on the host.  cell: metres per cell, the map's.  neutral: 1 .. 255, what a cell of
    cost 0 costs to stand on (navfn's COST_NEUTRAL).  blocked_at: 1 .. 255, a cell of this cost or more is impassable.  max_rounds:
    1 .. 4096, the most relaxation rounds (a sweep down and a sweep up each)."""

    def __init__(self, cell, neutral=50, blocked_at=253, max_rounds=64):
        fn = "NavSpec"
        try:
            self.cell = float(cell)
        except (TypeError, ValueError):
            raise L.CrdError(f"{fn}: cell is a number, not {cell!r}") from None
        if not (self.cell > 0 and math.isfinite(self.cell)):
            raise L.CrdError(f"{fn}: cell {cell} is not a finite positive size")
        self.neutral, self.blocked_at, self.max_rounds = (_whole(v, k, fn) for k, v in (("neutral", neutral), ("blocked_at", blocked_at),
                                                                                       ("max_rounds", max_rounds)))
        if not 1 <= self.neutral <= 255:
            raise L.CrdError(f"{fn}: neutral {neutral} is not in 1 .. 255")
        if not 1 <= self.blocked_at <= 255:
            raise L.CrdError(f"{fn}: blocked_at {blocked_at} is not in 1 .. 255")
        if not 1 <= self.max_rounds <= 4096:
            raise L.CrdError(f"{fn}: max_rounds {max_rounds} is not in 1 .. 4096")


def _spec(spec, fn):
    if not isinstance(spec, NavSpec):
        raise L.CrdError(f"{fn}: the first argument is a NavSpec")
    return spec


def _shape(M, nx, ny, fn):
    M, nx, ny = (_whole(v, k, fn) for k, v in (("M", M), ("nx", nx), ("ny", ny)))
    if M <= 0 or not 1 <= nx <= 65535 or not 1 <= ny <= 65535 or nx * ny > MAX_CELLS or M * nx * ny >= 2 ** 31:
        raise L.CrdError(f"{fn}: M {M} maps of {nx} x {ny} cells (M >= 1, each side 1 .. 65535, at most 2^19 cells a map, fewer than 2^31 in all)")
    return M, nx, ny


def workspace_bytes(M, nx, ny):
    """include/camradepth_hip.h, crd_nav_field: the kernels keep everything in registers and in togo itself, so none."""
    _shape(M, nx, ny, "nav.workspace_bytes")
    return 0


class NavWorkspace:
    """The preallocated outputs of nav_field for M maps of nx x ny cells: `out`, the dictionary nav_field(out=) takes ('next' may be
    set to None).  crd_nav_field needs no scratch memory; with out= a call allocates nothing, so it can be captured in a graph."""

    def __init__(self, spec, M, nx, ny, device="cuda"):
        _spec(spec, "NavWorkspace")
        M, nx, ny = _shape(M, nx, ny, "NavWorkspace")
        self.shape = (M, nx, ny)
        self.out = {"togo": torch.empty(M, nx, ny, dtype=torch.int32, device=device),
                    "next": torch.empty(M, nx, ny, dtype=torch.uint8, device=device), "info": torch.empty(M, 4, dtype=torch.int32, device=device)}


def _origin_of(v, M, fn):
    if isinstance(v, dict) and "origin" in v:
        v = v["origin"]
    elif isinstance(v, (tuple, list)) and len(v) == 2:
        v = v[1]
    if v is None or isinstance(v, (dict, tuple, list)):
        raise L.CrdError(f"{fn}: the third argument is occupancy.update's dictionary, (state, origin) or the origin, int64 [M,2]")
    return _dev(v, torch.int64, (M, 2), "origin")


def nav_field(spec, field_result_or_cost, map_or_state_origin, goals, n_goals=None, workspace=None, out=None):
    """The cost-to-go of a costmap (crd_nav_field, three launches on the current stream).

    field_result_or_cost: field.distance_field's dictionary (its 'cost') or uint8 [M,nx,ny] on the device, at most 2^19 cells a map.
    map_or_state_origin: occupancy.update's dictionary, (state, origin) or the origin itself, int64 [M,2] on the device, read there.
    goals: fp64 [M,G,2] on the device, metres in the map frame; n_goals: int32 [M], the goals of each map that count (None: all G).
    A goal that is not finite, outside the window or on an impassable cell is skipped.

    Returns 'togo' int32 [M,nx,ny] (0 on a goal cell, UNREACHED on impassable cells and those without a path), 'next' uint8 [M,nx,ny]
    (the neighbour code 0 .. 7 of NEIGHBOURS to step to, 8 on a goal cell, 255 where UNREACHED) and 'info' int32 [M,4] (converged,
    rounds, goals_used, goals_skipped).  workspace: a NavWorkspace (its `out` is then the default of out=); out: a dictionary of the
    three, in which 'next' may be None (left out): then nothing is allocated and nothing waits for the device."""
    fn = "nav.nav_field"
    _spec(spec, fn)
    cost = field_result_or_cost
    if isinstance(cost, dict):
        if cost.get("cost") is None:
            raise L.CrdError(f"{fn}: the second argument is distance_field's dictionary with its 'cost', or the costmap")
        cost = cost["cost"]
    cost = _dev(cost, torch.uint8, (None, None, None), "cost")
    M, nx, ny = _shape(*cost.shape, fn)
    origin = _origin_of(map_or_state_origin, M, fn)
    goals = _dev(goals, torch.float64, (M, None, 2), "goals")
    G = goals.shape[1]
    if G < 1:
        raise L.CrdError(f"{fn}: goals holds G {G} goals per map; at least 1")
    if n_goals is not None:
        n_goals = _dev(n_goals, torch.int32, (M,), "n_goals")
    if workspace is not None:
        if not isinstance(workspace, NavWorkspace) or workspace.shape != (M, nx, ny):
            raise L.CrdError(f"{fn}: the workspace was made for {list(getattr(workspace, 'shape', ()))}, the map is {[M, nx, ny]}")
        out = workspace.out if out is None else out
    shapes = {"togo": (M, nx, ny), "next": (M, nx, ny), "info": (M, 4)}
    if out is None:
        out = {k: torch.empty(shapes[k], dtype=t, device=cost.device) for k, t in OUTPUTS.items()}
    else:
        if not isinstance(out, dict) or set(out) != set(OUTPUTS):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(OUTPUTS)}")
        out = {k: None if out[k] is None and k in OPTIONAL else _dev(out[k], t, shapes[k], f"out['{k}']") for k, t in OUTPUTS.items()}
    L.check(L.load().crd_nav_field(L.ptr(cost), M, nx, ny, L.ptr(goals), L.ptr(n_goals), G, L.ptr(origin), L.f64_bits(spec.cell), spec.neutral,
                                   spec.blocked_at, spec.max_rounds, L.ptr(out["togo"]), L.ptr(out["next"]), L.ptr(out["info"]), L.stream()),
            "crd_nav_field")
    return out


def path_outputs(K, P, xy=True, device="cuda"):
    """The dictionary plan_paths(out=) takes for K paths of at most P cells."""
    out = {k: torch.empty((K, P) if k == "cells" else (K,), dtype=t, device=device) for k, t in PATH_OUTPUTS.items()}
    if xy:
        out["xy"] = torch.empty(K, P, 2, dtype=torch.float64, device=device)
    return out


def plan_paths(spec, nav_result, map_or_state_origin, starts, P, path_map=None, xy=True, out=None):
    """The paths that follow 'next' from K starts (crd_nav_paths, one launch on the current stream, one lane per path: a path is a chain
    of dependent reads, so its time grows with its length, not with K up to 64).

    nav_result: nav_field's dictionary with its 'next'.  starts: fp64 [K,2] on the device, metres in the map frame.  P: the most cells
    of a path.  path_map: int32 [K], the map of each path (None: map 0; an index outside 0 .. M-1: no start cell).

    Returns 'cells' int32 [K,P] (i * ny + j from the start cell on, the goal cell included when reached, -1 behind the end), with
    xy=True 'xy' fp64 [K,P,2] (the cells' centres in metres, NaN behind the end: check_paths(xy, n_poses=n_cells) takes it), 'n_cells'
    int32 [K], 'start_togo' int32 [K] (UNREACHED without a start cell) and 'status' int32 [K]: 0 ended on a goal, 1 cut at P, 2 the
    start is not finite, outside the window or on no map, 3 the start cell is UNREACHED (n_cells is 0 with 2 and 3).  out:
    path_outputs(): then nothing is allocated and nothing waits for the device."""
    fn = "nav.plan_paths"
    _spec(spec, fn)
    if not isinstance(nav_result, dict) or nav_result.get("togo") is None or nav_result.get("next") is None:
        raise L.CrdError(f"{fn}: nav_result is nav_field's dictionary with its 'togo' and 'next'")
    togo = _dev(nav_result["togo"], torch.int32, (None, None, None), "nav_result['togo']")
    M, nx, ny = _shape(*togo.shape, fn)
    nxt = _dev(nav_result["next"], torch.uint8, (M, nx, ny), "nav_result['next']")
    origin = _origin_of(map_or_state_origin, M, fn)
    starts = _dev(starts, torch.float64, (None, 2), "starts")
    K, P = starts.shape[0], _whole(P, "P", fn)
    if K < 1 or P < 1 or K * P >= 2 ** 30:
        raise L.CrdError(f"{fn}: K {K} paths of at most P {P} cells; each is at least 1 and K * P below 2^30")
    if path_map is not None:
        path_map = _dev(path_map, torch.int32, (K,), "path_map")
    names = list(PATH_OUTPUTS) + (["xy"] if xy else [])
    if out is None:
        out = path_outputs(K, P, xy, starts.device)
    else:
        if not isinstance(out, dict) or set(out) != set(names):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {names}")
        out = {k: _dev(out[k], PATH_OUTPUTS.get(k, torch.float64), {"cells": (K, P), "xy": (K, P, 2)}.get(k, (K,)), f"out['{k}']") for k in names}
    L.check(L.load().crd_nav_paths(L.ptr(starts), L.ptr(path_map), K, P, L.ptr(origin), L.f64_bits(spec.cell), L.ptr(togo), L.ptr(nxt), M, nx, ny,
                                   L.ptr(out["cells"]), L.ptr(out.get("xy")), L.ptr(out["n_cells"]), L.ptr(out["start_togo"]),
                                   L.ptr(out["status"]), L.stream()), "crd_nav_paths")
    return out
