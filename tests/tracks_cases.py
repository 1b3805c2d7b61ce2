"""Sequences of object tables for the tests of camradepth_amd.tracks: built directly with the layout of objects.map_objects' output, so
that every situation is placed exactly.  A case is a dictionary: M, N, nx, ny, cell, spec (TrackSpec's arguments) and frames; a frame
holds 'objects' int32 [M,N,8], 'centre' fp64 [M,N,2], 'info' int32 [M,4], 'origin' int64 [M,2] and 'reset' (the tracks are reset before
it).  M <= 3, N and T <= 64, 3 to 12 frames."""
import math

import numpy as np

UNUSED_ROW = (-1, 0, -1, -1, -1, -1, 0, 0)
SPEC = dict(max_tracks=8, gate=2.0, alpha=0.5, beta=0.25, confirm_hits=3, max_misses=3)
SNAP = dict(alpha=1.0, beta=0.0)                                         # a matched track sits on its object and has no velocity
_CASES = None


def frame(M, N, nx, ny, cell, origin, rows, n_objects=None, garbage=None, reset=False):
    """rows: per map a list of (x, y) or (x, y, n_cells) in map metres, or None for a row inside n_objects whose centre is NaN.  A row's
    box is the cell of its centre.  n_objects: per map, the rows that count (default: all given).  garbage: per map (x, y) rows written
    BEHIND the rows that count, as a table that was not cleared would hold them."""
    origin = np.asarray(origin, np.int64).reshape(M, 2)
    objects = np.tile(np.array(UNUSED_ROW, np.int32), (M, N, 1))
    centre = np.full((M, N, 2), np.nan)
    info = np.zeros((M, 4), np.int32)
    for m in range(M):
        listed = list(rows[m]) + list((garbage or {}).get(m, ()))
        assert len(listed) <= N
        for k, r in enumerate(listed):
            if r is None:
                objects[m, k] = (0, 1, 0, 0, 0, 0, 0, 0)
                continue
            x, y, cells = (r[0], r[1], r[2] if len(r) > 2 else 1)
            i, j = math.floor(x / cell) - int(origin[m, 0]), math.floor(y / cell) - int(origin[m, 1])
            edge = int(i in (0, nx - 1) or j in (0, ny - 1))
            objects[m, k] = (i * ny + j, cells, i, i, j, j, edge, 0)
            centre[m, k] = (x, y)
        info[m, 0] = len(rows[m]) if n_objects is None else n_objects[m]
    return dict(objects=objects, centre=centre, info=info, origin=origin, reset=reset)


def case(M, N, nx, ny, cell, frames, **spec):
    assert M <= 3 and N <= 64 and 3 <= len(frames) <= 12
    spec = dict(SPEC, **spec)
    assert spec["max_tracks"] <= 64
    return dict(M=M, N=N, nx=nx, ny=ny, cell=cell, spec=spec, frames=frames)


def chain(P):
    """P tracks and P objects alternating on a line with strictly falling gaps, o0 t0 o1 t1 ...: every object is nearest to the track on
    its right, every track but the last to the object on ITS right, so a round takes one pair, the last, and frees the next."""
    gaps = [10.0 * 0.9 ** i for i in range(2 * P)]
    xs = [1.0]
    for g in gaps[:-1]:
        xs.append(xs[-1] + g)
    return [(x, 1.25) for x in xs[0::2]], [(x, 1.25) for x in xs[1::2]]     # objects, tracks


def all_cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    c = {}
    o = [[0, 0]]

    def f1(N, rows, nx=32, ny=32, cell=0.5, origin=o, **kw):
        return frame(1, N, nx, ny, cell, origin, [rows], **kw)

    c["empty table, first frame"] = case(1, 8, 32, 32, 0.5, [f1(8, []), f1(8, [(4.25, 4.25)]), f1(8, [])])
    c["one static object, six frames"] = case(1, 8, 32, 32, 0.5, [f1(8, [(6.25, 7.75, 5)]) for _ in range(6)])
    c["moving a cell per frame"] = case(1, 8, 64, 32, 0.5, [f1(8, [(2.25 + 0.5 * s, 5.25)], nx=64) for s in range(12)])
    c["exact ties of d2"] = case(1, 8, 32, 32, 0.5, [
        f1(8, [(5.0, 5.0), (9.0, 5.0)]),                                 # slots 0 and 1
        f1(8, [(7.0, 5.0)]),                                             # d2 = 4 to both: the lower slot
        f1(8, [(8.0, 6.0), (8.0, 4.0)]),                                 # slots at (7, 5) and (9, 5): d2 = 2 for all four pairs
        f1(8, [(8.0, 3.0), (9.0, 4.0), (8.0, 7.0)]),                     # slots at (8, 6) and (8, 4): rows 0 and 1 tie for slot 1
    ], gate=3.0, **SNAP)
    c["on the gate and the next double above"] = case(1, 8, 64, 64, 0.5, [
        f1(8, [(4.0, 4.0), (20.0, 20.0)], nx=64, ny=64),
        f1(8, [(6.0, 4.0), (22.0, 20.0 + 2.0 ** -25)], nx=64, ny=64),    # d2 = 4 = gate * gate, and 4 + 2^-50
        f1(8, [(6.0, 4.0)], nx=64, ny=64),
    ], gate=2.0, **SNAP)
    for P, NT in ((20, 32), (16, 16)):
        objs, trks = chain(P)
        c[f"a displacement chain of {P} in {NT} slots"] = case(1, NT, 256, 8, 0.5, [
            f1(NT, trks, nx=256, ny=8), f1(NT, objs, nx=256, ny=8), f1(NT, objs, nx=256, ny=8)], max_tracks=NT, gate=11.0, **SNAP)
    there, away = f1(8, [(6.25, 6.25), (12.25, 3.25)]), f1(8, [(12.25, 3.25)])
    for mm in (0, 2):
        c[f"max_misses {mm}, gone for two frames"] = case(1, 8, 32, 32, 0.5, [there, there, away, away, there, there], max_misses=mm)
    six = [(2.25 + 2.5 * q, 3.25) for q in range(6)]
    c["births beyond the free slots"] = case(1, 8, 64, 32, 0.5, [
        f1(8, six, nx=64),                                               # four slots: two rows overflow
        f1(8, six[:3] + [(2.25 + 2.5 * q, 9.25) for q in range(3)], nx=64),      # slot 3 is freed and refilled in this call, two overflow
        f1(8, six[:3], nx=64),
    ], max_tracks=4, max_misses=0)
    abc = [(3.25, 3.25), (8.25, 4.25), (5.25, 11.25)]
    c["rows renumbered between frames"] = case(1, 8, 32, 32, 0.5, [f1(8, abc), f1(8, [abc[2], abc[0], abc[1]]), f1(8, [abc[1], abc[2], abc[0]]),
                                                                   f1(8, [(1.25, 1.25)] + abc)])
    c["the origin shifts by (+1, -2) a frame"] = case(1, 8, 32, 32, 0.5, [f1(8, abc, origin=[[-3 + s, 2 - 2 * s]]) for s in range(4)])
    c["a coasting track leaves the window"] = case(1, 8, 16, 16, 1.0, [
        f1(8, [(12.5 + s, 4.5), (3.5, 3.5)], nx=16, ny=16, cell=1.0) for s in range(3)] + [
        f1(8, [(3.5, 3.5)], nx=16, ny=16, cell=1.0) for _ in range(3)], alpha=1.0, beta=1.0, max_misses=5)
    c["NaN centre rows inside n_objects"] = case(1, 8, 32, 32, 0.5, [f1(8, [(3.25, 3.25), None, (9.25, 9.25)]), f1(8, [None, (3.25, 3.25), (9.25, 9.25)]),
                                                                    f1(8, [(3.25, 3.25), (9.25, 9.25), None])])
    c["stale rows behind n_objects"] = case(1, 8, 32, 32, 0.5, [
        f1(8, [(3.25, 3.25), (9.25, 9.25)]),
        f1(8, [(3.25, 3.25)], garbage={0: [(9.25, 9.25), (12.25, 12.25)]}),      # the second track misses, nothing is born
        f1(8, [], garbage={0: [(3.25, 3.25), (9.25, 9.25)]}),
        f1(8, [(3.25, 3.25), (9.25, 9.25)], n_objects=[99]),             # n_objects above N counts as N
    ])
    rng = np.random.default_rng(5)
    base = [[(float(x), float(y)) for x, y in rng.uniform(2.0, 14.0, (n, 2)).round(1)] for n in (5, 0, 9)]
    three, origins = [], [[0, 0], [-40, 7], [1 << 40, -(1 << 40)]]
    for s in range(6):
        rows = [[(x + 0.25 * s * (q % 3 - 1), y + 0.125 * s) for q, (x, y) in enumerate(b)][:len(b) - (s if m == 2 else 0)] for m, b in enumerate(base)]
        if s >= 3:
            rows[1] = [(5.0, 5.0 + s)]
        rows = [[(x + ox * 0.5, y + oy * 0.5) for x, y in r] for r, (ox, oy) in zip(rows, origins)]      # window-relative -> map metres
        three.append(frame(3, 16, 32, 32, 0.5, origins, rows))
    c["three maps with different histories"] = case(3, 16, 32, 32, 0.5, three, max_tracks=12)
    c["reset mid-sequence"] = case(1, 8, 32, 32, 0.5, [f1(8, abc), f1(8, abc), f1(8, abc, reset=True), f1(8, abc[:2])])
    # a crowd: rows jitter on a 0.5 lattice (tie-heavy), come and go; N > T
    crowd = []
    pts = rng.integers(2, 28, (2, 40, 2)) * 0.5
    for s in range(8):
        pts = pts + rng.integers(-1, 2, pts.shape) * 0.5
        rows = [[(float(x), float(y), int(q % 7 + 1)) for q, (x, y) in enumerate(pts[m]) if (q + s) % 5 and 0.5 <= x < 15.5 and 0.5 <= y < 15.5]
                for m in range(2)]
        crowd.append(frame(2, 48, 32, 32, 0.5, [[0, 0], [0, 0]], rows))
    c["a crowd on a lattice, two maps"] = case(2, 48, 32, 32, 0.5, crowd, max_tracks=32, gate=1.5, max_misses=1)
    _CASES = c
    return c
