"""GPU object tracks: the object tables of objects.map_objects followed over the frames, with ids that stay.

The stage behind objects.map_objects, whose object numbers are the raster order of first cells: object 3 of this frame has nothing to
do with object 3 of the next.  The map's window is world-aligned and moves by whole cells, so an object's centre in map metres stays
put from frame to frame: track_objects predicts every track (pos + vel), assigns the table's rows to the tracks greedily by distance
within a gate, moves the matched tracks (an alpha-beta filter), lets the others coast for max_misses frames, drops those that left the
window and gives every unmatched row a new track.  One launch per call, specified operation by operation in
include/camradepth_hip.h and the same bits every run: INTEGRATION.md, "Object tracks".  Nothing calls this module unless asked."""
import math

import torch

from . import lib as L
from ._frontend import _dev
from .field import _whole
from .nav import _origin_of

FREE, TENTATIVE, CONFIRMED = 0, 1, 2                                     # a slot's status
STATUS, AGE, HITS, MISSES, OBJECT, N_CELLS, FLAGS = range(7)             # the columns of 'tracks'
N_LIVE, N_MATCHED, N_BORN, N_MISSED_OUT, N_LEFT, N_OVERFLOW, ROUNDS, GUARD = range(8)     # the columns of 'info'
FREE_ROW = (FREE, 0, 0, 0, -1, 0, 0, 0)                                  # 'tracks' of a free slot
MAX_TRACKS = MAX_ROWS = 1024                                             # one thread per slot and per table row
STATE = {"ids": torch.int64, "tracks": torch.int32, "pos": torch.float64, "vel": torch.float64, "box": torch.int64, "next_id": torch.int64}
OUTPUTS = {"track_of": torch.int32, "id_of": torch.int64, "info": torch.int32}
SPEC_OPTIONS = {"max_tracks": 256, "gate": 2.0, "alpha": 0.5, "beta": 0.25, "confirm_hits": 3, "max_misses": 3}


class TrackSpec:
    """The numbers of a set of tracks, checked on the host.  max_tracks: 1 .. 1024, the slots per map.  gate: metres, finite and
    positive with a finite square; a row farther from a track's prediction is not its object.  alpha in (0, 1] and beta in [0, 2]: the
    share of the residual that goes into the position and into the velocity (metres per update).  confirm_hits: >= 1, the matches that
    make a track CONFIRMED.  max_misses: >= 0, the updates in a row a track may go unmatched before it is dropped."""

    def __init__(self, max_tracks=256, gate=2.0, alpha=0.5, beta=0.25, confirm_hits=3, max_misses=3):
        fn = "TrackSpec"
        self.max_tracks, self.confirm_hits, self.max_misses = (_whole(v, k, fn) for k, v in (
            ("max_tracks", max_tracks), ("confirm_hits", confirm_hits), ("max_misses", max_misses)))
        try:
            if any(isinstance(v, bool) for v in (gate, alpha, beta)):
                raise TypeError
            self.gate, self.alpha, self.beta = float(gate), float(alpha), float(beta)
        except (TypeError, ValueError):
            raise L.CrdError(f"{fn}: gate, alpha and beta are numbers, not {gate!r}, {alpha!r} and {beta!r}") from None
        if not 1 <= self.max_tracks <= MAX_TRACKS:
            raise L.CrdError(f"{fn}: max_tracks {max_tracks} is not in 1 .. {MAX_TRACKS}")
        if not (self.gate > 0 and math.isfinite(self.gate) and math.isfinite(self.gate * self.gate)):
            raise L.CrdError(f"{fn}: gate {gate} is not finite and positive with a finite square")
        if not 0 < self.alpha <= 1:
            raise L.CrdError(f"{fn}: alpha {alpha} is not in (0, 1]")
        if not 0 <= self.beta <= 2:
            raise L.CrdError(f"{fn}: beta {beta} is not in [0, 2]")
        if not 1 <= self.confirm_hits < 2 ** 31:
            raise L.CrdError(f"{fn}: confirm_hits {confirm_hits} is not in 1 .. 2^31 - 1")
        if not 0 <= self.max_misses < 2 ** 31:
            raise L.CrdError(f"{fn}: max_misses {max_misses} is not in 0 .. 2^31 - 1")


def _spec(spec, fn):
    if not isinstance(spec, TrackSpec):
        raise L.CrdError(f"{fn}: the first argument is a TrackSpec")
    return spec


class ObjectTracks:
    """The tracks of M maps of nx x ny cells of `cell` metres, T = spec.max_tracks slots each: the state that persists over the
    frames, on the device.  `ids` int64 [M,T] (-1 in a free slot), `tracks` int32 [M,T,8] (status, age, hits, misses, object, n_cells,
    flags, 0), `pos` and `vel` fp64 [M,T,2] (map metres and metres per update; NaN in a free slot), `box` int64 [M,T,4] (world cells
    ox + i_min, ox + i_max, oy + j_min, oy + j_max) and `next_id` int64 [M].  Empty after construction."""

    def __init__(self, spec, M, nx, ny, cell, device="cuda"):
        fn = "ObjectTracks"
        _spec(spec, fn)
        M, nx, ny = (_whole(v, k, fn) for k, v in (("M", M), ("nx", nx), ("ny", ny)))
        if M <= 0 or not 1 <= nx <= 65535 or not 1 <= ny <= 65535:
            raise L.CrdError(f"{fn}: M {M} maps of {nx} x {ny} cells (M >= 1, each side 1 .. 65535)")
        try:
            self.cell = float(cell)
        except (TypeError, ValueError):
            raise L.CrdError(f"{fn}: cell is a number, not {cell!r}") from None
        if not (self.cell > 0 and math.isfinite(self.cell)):
            raise L.CrdError(f"{fn}: cell {cell} is not a finite positive size")
        self.M, self.nx, self.ny, self.max_tracks = M, nx, ny, spec.max_tracks
        T = spec.max_tracks
        shapes = {"ids": (M, T), "tracks": (M, T, 8), "pos": (M, T, 2), "vel": (M, T, 2), "box": (M, T, 4), "next_id": (M,)}
        for k, t in STATE.items():
            setattr(self, k, torch.empty(shapes[k], dtype=t, device=device))
        self.reset()

    def state(self):
        """The state tensors by name: the views track_objects returns beside its outputs."""
        return {k: getattr(self, k) for k in STATE}

    def reset(self):
        """Every slot free and the ids from 0 again.  Fills only: it can be captured."""
        self.ids.fill_(-1)
        self.tracks.zero_()
        self.tracks[..., OBJECT].fill_(-1)
        self.pos.fill_(math.nan)
        self.vel.fill_(math.nan)
        self.box.zero_()
        self.next_id.zero_()


def _rows(N, fn):
    if not 1 <= N <= MAX_ROWS:
        raise L.CrdError(f"{fn}: an object table of N {N} rows; 1 .. {MAX_ROWS} are tracked (ObjectSpec(max_objects=))")
    return N


class TrackWorkspace:
    """The preallocated per-call outputs of track_objects for object tables of N rows: `out`, the dictionary track_objects(out=) takes.
    With workspace= a call allocates nothing, so it can be captured in a graph on one stream."""

    def __init__(self, spec, tracks, N):
        fn = "TrackWorkspace"
        _spec(spec, fn)
        if not isinstance(tracks, ObjectTracks):
            raise L.CrdError(f"{fn}: the second argument is an ObjectTracks")
        self.N, self.M = _rows(_whole(N, "N", fn), fn), tracks.M
        dev = tracks.ids.device
        self.out = {"track_of": torch.empty(tracks.M, self.N, dtype=torch.int32, device=dev),
                    "id_of": torch.empty(tracks.M, self.N, dtype=torch.int64, device=dev),
                    "info": torch.empty(tracks.M, 8, dtype=torch.int32, device=dev)}


def track_objects(spec, tracks, objects_out, origin_or_update_result, workspace=None, out=None):
    """One frame's object table into the tracks (crd_track_objects, one launch on the current stream).

    tracks: an ObjectTracks, updated in place.  objects_out: objects.map_objects' dictionary ('objects', 'centre', which must not be
    None, and 'info') with a table of N = 1 .. 1024 rows.  origin_or_update_result: occupancy.update's dictionary, (state, origin) or
    the origin itself, int64 [M,2] on the device, read there: the same one map_objects was given.

    Returns 'track_of' int32 [M,N] (the slot that holds row k's track, -1 for a row without one), 'id_of' int64 [M,N] (its id, -1),
    'info' int32 [M,8] (n_live, n_matched, n_born, n_missed_out, n_left, n_overflow, rounds, guard; guard is 0 in every correct run)
    and the state tensors of `tracks` by name, as views.  workspace: a TrackWorkspace (its `out` is then the default of out=); out: a
    dictionary of the three: then nothing is allocated and nothing waits for the device."""
    fn = "tracks.track_objects"
    _spec(spec, fn)
    if not isinstance(tracks, ObjectTracks) or tracks.max_tracks != spec.max_tracks:
        raise L.CrdError(f"{fn}: the second argument is an ObjectTracks of the spec's max_tracks {spec.max_tracks}, not "
                         f"{getattr(tracks, 'max_tracks', tracks)!r}")
    if not isinstance(objects_out, dict) or not {"objects", "centre", "info"} <= set(objects_out):
        raise L.CrdError(f"{fn}: the third argument is map_objects' dictionary with 'objects', 'centre' and 'info'")
    if objects_out["centre"] is None:
        raise L.CrdError(f"{fn}: the object table has 'centre': None; the tracks follow the centres (map_objects with a 'centre')")
    M, T = tracks.M, tracks.max_tracks
    table = objects_out["objects"]
    if torch.is_tensor(table) and table.dim() == 3:                      # the sizes first: they are the caller's choice of specs
        N = _rows(table.shape[1], fn)
        if workspace is not None and (not isinstance(workspace, TrackWorkspace) or (workspace.M, workspace.N) != (M, N)):
            raise L.CrdError(f"{fn}: the workspace was made for {getattr(workspace, 'M', None)} maps and tables of "
                             f"{getattr(workspace, 'N', None)} rows, these are {M} maps and {N} rows")
    table = _dev(table, torch.int32, (M, None, 8), "objects_out['objects']")
    N = table.shape[1]
    centre = _dev(objects_out["centre"], torch.float64, (M, N, 2), "objects_out['centre']")
    table_info = _dev(objects_out["info"], torch.int32, (M, 4), "objects_out['info']")
    origin = _origin_of(origin_or_update_result, M, fn)
    shapes = {"ids": (M, T), "tracks": (M, T, 8), "pos": (M, T, 2), "vel": (M, T, 2), "box": (M, T, 4), "next_id": (M,)}
    state = {k: _dev(getattr(tracks, k), t, shapes[k], f"tracks.{k}") for k, t in STATE.items()}
    if workspace is not None:
        out = workspace.out if out is None else out
    shapes = {"track_of": (M, N), "id_of": (M, N), "info": (M, 8)}
    if out is None:
        out = {k: torch.empty(shapes[k], dtype=t, device=table.device) for k, t in OUTPUTS.items()}
    else:
        if not isinstance(out, dict) or set(out) != set(OUTPUTS):
            raise L.CrdError(f"{fn}: out= is a dictionary that holds exactly {list(OUTPUTS)}")
        out = {k: _dev(out[k], t, shapes[k], f"out['{k}']") for k, t in OUTPUTS.items()}
    L.check(L.load().crd_track_objects(L.ptr(table), L.ptr(centre), L.ptr(table_info), L.ptr(origin), M, N, T, tracks.nx, tracks.ny,
                                       L.f64_bits(tracks.cell), L.f64_bits(spec.gate), L.f64_bits(spec.alpha), L.f64_bits(spec.beta),
                                       spec.confirm_hits, spec.max_misses, L.ptr(state["ids"]), L.ptr(state["tracks"]), L.ptr(state["pos"]),
                                       L.ptr(state["vel"]), L.ptr(state["box"]), L.ptr(state["next_id"]), L.ptr(out["track_of"]),
                                       L.ptr(out["id_of"]), L.ptr(out["info"]), L.stream()), "crd_track_objects")
    return dict(out, **state)
