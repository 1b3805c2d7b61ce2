"""Inputs for the scan-matcher tests, as NumPy arrays and plain numbers.  A case is {'params': the numbers of an OccupancyMap, 'B',
'build': the keyword arguments of tests/occupancy_ref.py's update, one per call, that make the map (none: the map stays
uninitialised), 'matches': a list of {'spec', 'kw', and perhaps 'planted': the (turn steps, dx, dy) that undo the prior's offset}}.
state_of(case) runs the build once.  Shared by tests/test_match_ref_cpu.py, tests/test_match_pick_cpu.py and tests/test_gpu_match.py."""
import math

import numpy as np

from tests import match_ref, occupancy_ref
from tests.occupancy_cases import INF, NAN, compact, params, pose

D_THETA = math.radians(2.0)
_STATES = {}


def map_params(**changes):
    return params(**dict(dict(n_bins=360, max_range=12.0, z_floor=-0.5, z_lo=0.25, z_hi=2.0, min_points=2, l_occ=3, l_free=1, l_max=10), **changes))


def l_scene(rs, cx=0.0, cy=0.0, walls=True, n_ground=1500, far=False):
    """World points around (cx, cy): an L-shaped wall of two arms, three posts, the ground; far: three posts more, 10 to 13 m out, which a
    window 37 cells wide holds just outside its edge and beyond it.  -> fp64 [n,3]."""
    rows = []
    if walls:
        t = np.arange(-5.0, 5.17, 0.04)
        rows.append(np.stack([np.full_like(t, cx + 6.13) + rs.uniform(-0.02, 0.02, len(t)), cy + t, rs.uniform(0.3, 1.9, len(t))], axis=1))
        t = np.arange(-2.0, 6.13, 0.04)
        rows.append(np.stack([cx + t, np.full_like(t, cy + 5.17) + rs.uniform(-0.02, 0.02, len(t)), rs.uniform(0.3, 1.9, len(t))], axis=1))
    for px, py in ((-3.3, -2.2), (2.6, -4.4), (-4.1, 1.7)) + (((-10.2, 0.6), (-13.1, -0.7), (0.4, -12.3)) if far else ()):
        rows.append(np.stack([cx + px + rs.uniform(-0.05, 0.05, 30), cy + py + rs.uniform(-0.05, 0.05, 30), rs.uniform(0.3, 1.9, 30)], axis=1))
    a, r = rs.uniform(-np.pi, np.pi, n_ground), rs.uniform(0.4, 9.0, n_ground)
    rows.append(np.stack([cx + r * np.cos(a), cy + r * np.sin(a), rs.uniform(-0.05, 0.05, n_ground)], axis=1))
    return np.concatenate(rows)


def corridor_scene(rs, cx, cy, half_length):
    """Two walls along x, 3.2 m to either side of (cx, cy), and the ground between them."""
    t = np.arange(-half_length, half_length, 0.04)
    rows = [np.stack([cx + t, np.full_like(t, cy + side) + rs.uniform(-0.02, 0.02, len(t)), rs.uniform(0.3, 1.9, len(t))], axis=1)
            for side in (3.2, -3.2)]
    g = 40 * int(half_length)
    rows.append(np.stack([cx + rs.uniform(-half_length, half_length, g), cy + rs.uniform(-3.0, 3.0, g), rs.uniform(-0.05, 0.05, g)], axis=1))
    return np.concatenate(rows)


def seen_from(world, T):
    """World points in the frame of the pose T (a turn about z and a translation) -> fp32 [n,3]."""
    d = world - T[:, 3]
    return (d @ T[:, :3]).astype(np.float32)


def off_by(x, y, heading, planted, cell, d_theta=D_THETA):
    """The prior that the candidate `planted` = (turn steps, dx, dy) brings back to pose(x, y, heading): the sensor is the origin of
    the points' frame, so the turn about it changes the heading alone."""
    k, dx, dy = planted
    return pose(x - dx * cell, y - dy * cell, heading - k * d_theta)


def planted_case(seed, nx, ny, x, y, heading, spec, offsets, extra_range=False):
    """The L-shaped scene fused three times from one pose, then seen again from the same place with the prior off by each of `offsets`."""
    rs = np.random.RandomState(seed)
    p = map_params(nx=nx, ny=ny, max_range=14.0 if extra_range else 12.0)
    T = pose(x, y, heading)
    cloud = seen_from(l_scene(rs, x, y, far=extra_range), T)
    kw = dict(compact([cloud]), valid=None, sensor=None)
    build = [dict(kw, T=T, centre=None)] * 3
    matches = [dict(spec=spec, kw=dict(kw, T=off_by(x, y, heading, o, p["cell"], spec["d_theta"])), planted=o) for o in offsets]
    return dict(params=p, B=1, build=build, matches=matches)


def corridor_case():
    """A corridor fused from five poses along it, four times each, so that its walls fill the window at the clamp; then a scan that reaches 6 m: every shift along
    the corridor scores the same, and the tie rule keeps dx at the prior's."""
    rs = np.random.RandomState(21)
    p = map_params(nx=64, ny=65, max_range=6.0)
    world = corridor_scene(rs, 3.1, -2.3, 30.0)
    build = [dict(compact([seen_from(world, pose(3.1 + s, -2.3, 0.0))]), valid=None, sensor=None, T=pose(3.1 + s, -2.3, 0.0),
                  centre=np.array([-s, 0.0, 0.0])) for s in (-8.0, -4.0, 0.0, 4.0, 8.0, 0.0) for _ in range(4)]
    spec = match_ref.spec(n_xy=3, n_theta=1, d_theta=D_THETA)
    kw = dict(compact([seen_from(world, pose(3.1, -2.3, 0.0))]), valid=None, sensor=None)
    return dict(params=p, B=1, build=build, matches=[dict(spec=spec, kw=dict(kw, T=pose(3.1, -2.3 - 0.5, 0.0)), planted=(0, 0, 1)),
                                                     dict(spec=spec, kw=dict(kw, T=pose(3.1 + 1.0, -2.3, 0.0)), planted=None)])


def symmetric_case():
    """Four posts point-symmetric about a sensor that stands on a cell centre, fused from there: the occupied cells are point-symmetric
    about the window's middle, several turns score the same, and the prior wins.  Then the same scan with a prior one cell off along x towards the middle between two
    posts of a map that holds posts two cells apart: +1 and -1 tie, and the least dx is taken."""
    p = map_params(nx=37, ny=53, n_bins=8, max_range=8.0, min_points=1)
    q = np.array([(2.1, 1.1), (-2.1, -1.1), (1.1, -3.1), (-1.1, 3.1)])
    posts = np.concatenate([np.concatenate([q + (dx, dy) for dx in (-0.05, 0.05) for dy in (-0.05, 0.05)], axis=0)])
    cloud = np.concatenate([posts, np.full((len(posts), 1), 1.0)], axis=1).astype(np.float32)
    T = pose(0.25, 0.25, 0.0)
    kw = dict(compact([cloud]), valid=None, sensor=None)
    spec = match_ref.spec(n_xy=3, n_theta=2, d_theta=D_THETA, min_cells=1)
    pair = np.array([(3.1 + s + dx, 0.1 + dy, 1.0) for s in (-1.0, 1.0) for dx in (-0.05, 0.05) for dy in (-0.05, 0.05)], np.float32)
    single = np.array([(3.1 + dx, 0.1 + dy, 1.0) for dx in (-0.05, 0.05) for dy in (-0.05, 0.05)], np.float32)
    two = dict(params=p, B=1, build=[dict(compact([pair]), valid=None, sensor=None, T=T, centre=None)] * 2,
               matches=[dict(spec=match_ref.spec(n_xy=3, n_theta=0, d_theta=D_THETA, min_cells=1), kw=dict(compact([single]), valid=None, sensor=None, T=T),
                             planted=None)])
    return dict(params=p, B=1, build=[dict(kw, T=T, centre=None)] * 2, matches=[dict(spec=spec, kw=dict(kw, T=T), planted=(0, 0, 0))]), two


def forms_case(form, M, nx=37, ny=53, nan_pose=False, seed=31):
    """Three frames of the L-shaped scene seen from three poses near (-30.2, -17.7) -- negative world cells, a window that wraps the
    torus in both axes --, in one of the three forms of a cloud, with rows that are not finite, a valid mask and rows beyond the last
    frame; the priors off by a cell and a step.  M == 1: the three frames are one rig with one prior; nan_pose: map 1's prior is NaN."""
    rs = np.random.RandomState(seed)
    x, y, h = -30.2, -17.7, 0.4
    p = map_params(M=M, nx=nx, ny=ny, max_range=14.0)
    world = l_scene(rs, x, y, n_ground=900, far=True)
    rig = [(0.0, 0.0, 0.0), (0.6, -0.4, 0.7), (-0.5, 0.3, -0.9)]
    if M == 1:
        Ts = pose(x, y, h)
        sensors = np.array([(a, b, 0.0) for a, b, _ in rig])
        clouds = [seen_from(world, Ts) for _ in rig]                      # one frame of points, three sensors on it
        clouds = [c[i::3] for i, c in enumerate(clouds)]
        prior = off_by(x, y, h, (0, 1, -1), p["cell"])                    # a shift alone: the turn would go about frame 0's sensor
        planted = (0, 1, -1)
    else:
        Ts = np.stack([pose(x + a, y + b, h + c) for a, b, c in rig])
        sensors = None
        clouds = [seen_from(world, T) for T in Ts]
        prior = np.stack([off_by(x + a, y + b, h + c, (1, -1, 1), p["cell"]) for a, b, c in rig])
        planted = (1, -1, 1)
    for c in clouds:
        c[rs.randint(0, len(c), 4), rs.randint(0, 3, 4)] = [NAN, INF, -INF, NAN]
    if form == "organised":
        rows = min(len(c) for c in clouds)
        kw = dict(xyz=np.concatenate([c[:rows] for c in clouds]), rows_per_frame=rows, valid=(rs.uniform(size=3 * rows) > 0.05).astype(np.uint8))
    else:
        kw = compact(clouds, extra=7)
        kw["valid"] = (rs.uniform(size=len(kw["xyz"])) > 0.05).astype(np.uint8) if form == "compact" else None
    kw["sensor"] = sensors
    if nan_pose:
        prior = prior.copy()
        prior[1, 0, 1] = NAN
    spec = match_ref.spec(n_xy=2, n_theta=2, d_theta=D_THETA)
    return dict(params=p, B=3, build=[dict(kw, T=Ts, centre=None)] * 3, matches=[dict(spec=spec, kw=dict(kw, T=prior), planted=planted)], form=form)


def contention_case(n=4096):
    """4,096 rows into one cell of a map that holds it: min_points 1, 3 and more than there are rows."""
    rs = np.random.RandomState(8)
    xyz = np.stack([3.1 + rs.randint(0, 4, n) / 16.0, 0.05 + rs.randint(0, 2, n) / 64.0, 0.5 + rs.randint(0, 3, n) / 4.0], axis=1).astype(np.float32)
    kw = dict(xyz=xyz, frame_offsets=np.array([0, n], np.int32), valid=None, sensor=None, T=None)
    specs = [match_ref.spec(n_xy=1, n_theta=1, d_theta=D_THETA, min_points=k, min_cells=1) for k in (1, 3, n + 1)]
    return dict(params=map_params(nx=16, ny=16, n_bins=8), B=1, build=[dict(kw, centre=None)] * 2, matches=[dict(spec=s, kw=kw, planted=None) for s in specs])


def guard_case():
    """One match per guard on the 37 x 53 planted map: too few cells, a score too low, a sensor that is not finite, then a search
    range too small for the offset (the pick on its border) and no rows at all."""
    c = planted_case(41, 37, 53, 2.3, -1.9, 0.3, match_ref.spec(n_xy=2, n_theta=1, d_theta=D_THETA), [(0, 0, 0)])
    kw, T = c["matches"][0]["kw"], pose(2.3, -1.9, 0.3)
    s = match_ref.spec
    c["matches"] = [
        dict(spec=s(n_xy=2, n_theta=1, d_theta=D_THETA, min_cells=10 ** 6), kw=dict(kw, T=T), planted=None),
        dict(spec=s(n_xy=2, n_theta=1, d_theta=D_THETA, min_score=10 ** 9), kw=dict(kw, T=T), planted=None),
        dict(spec=s(n_xy=2, n_theta=1, d_theta=D_THETA), kw=dict(kw, T=T, sensor=np.array([0.0, INF, 0.0])), planted=None),
        dict(spec=s(n_xy=1, n_theta=1, d_theta=D_THETA), kw=dict(kw, T=off_by(2.3, -1.9, 0.3, (1, 2, -2), 0.5)), planted=None),
        dict(spec=s(n_xy=2, n_theta=1, d_theta=D_THETA, min_cells=0, min_score=0),
             kw=dict(xyz=np.zeros((0, 3), np.float32), frame_offsets=np.zeros(2, np.int32), valid=None, sensor=None, T=T), planted=None)]
    return c


def uninitialised_case():
    c = planted_case(43, 37, 53, 2.3, -1.9, 0.3, match_ref.spec(n_xy=2, n_theta=1, d_theta=D_THETA), [(1, 1, 1)])
    return dict(c, build=[])


def all_cases():
    s = match_ref.spec
    sym, two = symmetric_case()
    return {
        "37 x 53, planted offsets": planted_case(41, 37, 53, 2.3, -1.9, 0.3, s(n_xy=3, n_theta=3, d_theta=D_THETA),
                                                 [(0, 0, 0), (2, 0, 0), (0, -3, 2), (-1, 1, -2), (1, 2, 3)], extra_range=True),
        "64 x 65, turns only": planted_case(42, 64, 65, -7.6, 4.1, -1.1, s(n_xy=0, n_theta=4, d_theta=D_THETA), [(3, 0, 0), (-4, 0, 0)]),
        "64 x 65, shifts only": planted_case(44, 64, 65, -7.6, 4.1, -1.1, s(n_xy=5, n_theta=0, d_theta=D_THETA), [(0, 4, -5), (0, -1, 0)]),
        "37 x 53, n_xy 16 with n_theta 2": planted_case(45, 37, 53, 12.4, 8.8, 2.0, s(n_xy=16, n_theta=2, d_theta=D_THETA), [(-1, 9, -13)],
                                                        extra_range=True),
        "a corridor": corridor_case(),
        "a point-symmetric scene": sym,
        "two posts, one seen between them": two,
        "three maps, compact": forms_case("compact", 3),
        "three maps, organised, 64 x 65": forms_case("organised", 3, 64, 65),
        "one rig of three frames, bare xyz": forms_case("bare", 1),
        "three maps, a NaN pose for one": forms_case("compact", 3, nan_pose=True),
        "contention": contention_case(),
        "the guards": guard_case(),
        "an uninitialised map": uninitialised_case(),
    }


def state_of(name, case):
    """The map of a case after its build, made once and left unchanged."""
    if name not in _STATES:
        state = occupancy_ref.new_state(case["params"])
        for kw in case["build"]:
            occupancy_ref.update(case["params"], state, kw["xyz"], case["B"], frame_offsets=kw.get("frame_offsets"),
                                 rows_per_frame=kw.get("rows_per_frame", 0), valid=kw.get("valid"), T=kw.get("T"), sensor=kw.get("sensor"),
                                 centre=kw.get("centre"))
        _STATES[name] = state
    return _STATES[name]


def match_of(case, state, i):
    """The restatement's outputs of the case's match i."""
    m = case["matches"][i]
    kw = m["kw"]
    return match_ref.match_scan(case["params"], state, m["spec"], kw["xyz"], case["B"], frame_offsets=kw.get("frame_offsets"),
                                rows_per_frame=kw.get("rows_per_frame", 0), valid=kw.get("valid"), T=kw.get("T"), sensor=kw.get("sensor"))
