"""GPU map objects: a state map -> the connected sets of its obstacle cells as a label per cell and a table of objects.

A stage beside field.distance_field on occupancy.update's `state`.  distance_field says how far the nearest occupied cell is;
map_objects says which obstacle that is, how many there are, where they are and how large: per object its first cell, its cells,
its box, whether it touches the window's edge, its coordinate sums and its centre in map metres, which field.check_paths and
nav.nav_field(goals=) take as they are.  The map's window is world-aligned and moves by whole cells, so an object's cells and centre
stay put from frame to frame.  Connected-component labelling by union-find in eight launches, integer atomics only, specified in
include/camradepth_hip.h and the same bits every run: INTEGRATION.md, "Map objects".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from ._frontend import _dev
from .field import _state_of, _whole
from .nav import _origin_of
from .occupancy import OCCUPIED

BACKGROUND, SMALL, OVERFLOW = -1, -2, -3             # label of a non-source cell, of a cell of a small and of an overflowing object
FIRST_CELL, N_CELLS, I_MIN, I_MAX, J_MIN, J_MAX, FLAGS = range(7)      # the columns of 'objects'
TOUCHES_EDGE = 1                                     # bit 0 of FLAGS
N_OBJECTS, N_OVERFLOW, N_SMALL, GUARD = range(4)     # the columns of 'info'
OUTPUTS = {"label": torch.int32, "objects": torch.int32, "sums": torch.int64, "centre": torch.float64, "info": torch.int32}
OPTIONAL = ("centre",)                               # out= may hold None for it: the launch is then left out
SPEC_OPTIONS = {"sources": (OCCUPIED,), "connectivity": 8, "min_cells": 1, "max_objects": 256}


class ObjectSpec:
    """The numbers of an object table, checked on the host.  cell: metres per cell, the map's.  sources: the states that count as
    obstacle cells, each 0 .. 7.  connectivity: 4, or 8 (cells that touch at a corner belong together).  min_cells: >= 1, an object of
    fewer cells is SMALL and gets no row.  max_objects: 1 .. 65535, the rows of the table; kept objects beyond them OVERFLOW."""

    def __init__(self, cell, sources=(OCCUPIED,), connectivity=8, min_cells=1, max_objects=256):
        fn = "ObjectSpec"
        try:
            self.cell = float(cell)
        except (TypeError, ValueError):
            raise L.CrdError(f"{fn}: cell is a number, not {cell!r}") from None
        if not (self.cell > 0 and math.isfinite(self.cell)):
            raise L.CrdError(f"{fn}: cell {cell} is not a finite positive size")
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
        self.connectivity, self.min_cells, self.max_objects = (_whole(v, k, fn) for k, v in (
            ("connectivity", connectivity), ("min_cells", min_cells), ("max_objects", max_objects)))
        if self.connectivity not in (4, 8):
            raise L.CrdError(f"{fn}: connectivity {connectivity} is neither 4 nor 8")
        if not 1 <= self.min_cells < 2 ** 31:
            raise L.CrdError(f"{fn}: min_cells {min_cells} is not in 1 .. 2^31 - 1")
        if not 1 <= self.max_objects <= 65535:
            raise L.CrdError(f"{fn}: max_objects {max_objects} is not in 1 .. 65535")


def _spec(spec, fn):
    if not isinstance(spec, ObjectSpec):
        raise L.CrdError(f"{fn}: the first argument is an ObjectSpec")
    return spec


def _shape(M, nx, ny, fn):
    M, nx, ny = (_whole(v, k, fn) for k, v in (("M", M), ("nx", nx), ("ny", ny)))
    if M <= 0 or not 1 <= nx <= 65535 or not 1 <= ny <= 65535 or M * nx * ny >= 2 ** 31:
        raise L.CrdError(f"{fn}: M {M} maps of {nx} x {ny} cells (M >= 1, each side 1 .. 65535, fewer than 2^31 cells)")
    return M, nx, ny


def workspace_bytes(M, nx, ny):
    """include/camradepth_hip.h, crd_map_objects: a root and a count per cell, int32 [M][nx][ny] each, up to a multiple of 16 bytes."""
    M, nx, ny = _shape(M, nx, ny, "objects.workspace_bytes")
    return (8 * M * nx * ny + 15) & ~15


def _shapes(spec, M, nx, ny):
    N = spec.max_objects
    return {"label": (M, nx, ny), "objects": (M, N, 8), "sums": (M, N, 2), "centre": (M, N, 2), "info": (M, 4)}


class ObjectWorkspace:
    """The scratch memory of map_objects for M maps of nx x ny cells, `buf`, and its preallocated outputs: `out`, the dictionary
    map_objects(out=) takes ('centre' may be set to None).  With workspace= a call allocates nothing, so it can be captured in a graph
    on one stream."""

    def __init__(self, spec, M, nx, ny, device="cuda"):
        _spec(spec, "ObjectWorkspace")
        M, nx, ny = _shape(M, nx, ny, "ObjectWorkspace")
        self.shape, self.max_objects = (M, nx, ny), spec.max_objects
        self.buf = torch.empty(workspace_bytes(M, nx, ny), dtype=torch.uint8, device=device)
        self.out = {k: torch.empty(s, dtype=OUTPUTS[k], device=device) for k, s in _shapes(spec, M, nx, ny).items()}


def map_objects(spec, state_or_update_result, map_or_state_origin, workspace=None, out=None):
    """The objects of a state map (crd_map_objects, eight launches on the current stream, seven without 'centre').

    state_or_update_result: occupancy.update's dictionary (its 'state') or uint8 [M,nx,ny] on the device.  map_or_state_origin:
    occupancy.update's dictionary, (state, origin) or the origin itself, int64 [M,2] on the device, read there.

    Returns 'label' int32 [M,nx,ny] (BACKGROUND on a non-source cell, SMALL, OVERFLOW, else the object's number), 'objects' int32
    [M,N,8] (first_cell, n_cells, i_min, i_max, j_min, j_max, flags, 0; N = spec.max_objects; unused rows -1, 0, -1, -1, -1, -1, 0, 0),
    'sums' int64 [M,N,2] (of i and of j over the cells), 'centre' fp64 [M,N,2] (metres in the map frame, NaN in unused rows) and
    'info' int32 [M,4] (n_objects, n_overflow, n_small, guard; guard is 0 in every correct run).  The objects are numbered in the
    order of their first cells, as scipy.ndimage.label numbers them.  workspace: an ObjectWorkspace (its `out` is then the default of
    out=); out: a dictionary of the five, in which 'centre' may be None (left out): then nothing is allocated and nothing waits for
    the device."""
    fn = "objects.map_objects"
    _spec(spec, fn)
    state = _state_of(state_or_update_result, fn)
    M, nx, ny = _shape(*state.shape, fn)
    origin = _origin_of(map_or_state_origin, M, fn)
    if workspace is not None:
        if not isinstance(workspace, ObjectWorkspace) or workspace.shape != (M, nx, ny) or workspace.max_objects != spec.max_objects:
            raise L.CrdError(f"{fn}: the workspace was made for {list(getattr(workspace, 'shape', ()))} and max_objects "
                             f"{getattr(workspace, 'max_objects', None)}, the map is {[M, nx, ny]} and the spec holds {spec.max_objects}")
        buf = workspace.buf
        out = workspace.out if out is None else out
    else:
        buf = torch.empty(workspace_bytes(M, nx, ny), dtype=torch.uint8, device=state.device)
    shapes = _shapes(spec, M, nx, ny)
    if out is None:
        out = {k: torch.empty(shapes[k], dtype=t, device=state.device) for k, t in OUTPUTS.items()}
    else:
        if not isinstance(out, dict) or set(out) != set(OUTPUTS):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(OUTPUTS)}")
        out = {k: None if out[k] is None and k in OPTIONAL else _dev(out[k], t, shapes[k], f"out['{k}']") for k, t in OUTPUTS.items()}
    L.check(L.load().crd_map_objects(L.ptr(state), M, nx, ny, spec.source_mask, spec.connectivity, spec.min_cells, spec.max_objects,
                                     L.ptr(origin), L.f64_bits(spec.cell), L.ptr(buf), buf.numel(), L.ptr(out["label"]), L.ptr(out["objects"]),
                                     L.ptr(out["sums"]), L.ptr(out["centre"]), L.ptr(out["info"]), L.stream()), "crd_map_objects")
    return out
