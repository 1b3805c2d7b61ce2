"""Inputs for the occupancy-map tests, as NumPy arrays and plain numbers.  A case is {'params': the numbers of an OccupancyMap, 'B',
'frames': a list of the keyword arguments of tests/occupancy_ref.py's update, one per call, in order}.  Shared by
tests/test_occupancy_ref_cpu.py (restatement against loops) and tests/test_gpu_occupancy.py (kernels against the restatement)."""
import numpy as np

NAN, INF = float("nan"), float("inf")
# every number an exact binary fraction, so that edges are edges
PARAMS = dict(M=1, nx=40, ny=36, cell=0.5, n_bins=720, max_range=12.0, z_floor=-0.5, z_lo=0.25, z_hi=2.0, min_points=2, l_occ=3, l_free=1,
              l_max=10, occupied_at=4, free_at=2)


def params(**changes):
    return dict(PARAMS, **changes)


def pose(x, y, heading, z=0.0):
    """[3,4]: a turn about z by `heading` radians and a translation."""
    c, s = np.cos(heading), np.sin(heading)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, z]])


def fan(rs, n_ground=500, n_wall=200, wall=6.0, spread=np.pi / 4, reach=11.0):
    """A 90-degree fan seen from the origin of the points' frame (x forward, y left, z up): ground points out to the wall `wall`
    metres ahead (None: no wall, out to `reach`), the wall itself between 0.3 and 1.9 m, a few points above the band, a few
    non-finite.  -> fp32 [n,3]."""
    a = rs.uniform(-spread, spread, n_ground)
    r = rs.uniform(0.4, reach, n_ground)
    x, y = r * np.cos(a), r * np.sin(a)
    if wall is not None:
        ok = x < wall
        x, y = x[ok], y[ok]
    rows = [np.stack([x, y, rs.uniform(-0.05, 0.05, len(x))], axis=1)]
    if wall is not None:
        rows.append(np.stack([np.full(n_wall, wall) + rs.uniform(0.0, 0.2, n_wall), rs.uniform(-wall, wall, n_wall), rs.uniform(0.3, 1.9, n_wall)], axis=1))
    rows.append(np.stack([rs.uniform(1.0, 5.0, 8), rs.uniform(-2.0, 2.0, 8), rs.uniform(2.5, 4.0, 8)], axis=1))       # above z_hi
    xyz = np.concatenate(rows).astype(np.float32)
    xyz = xyz[rs.permutation(len(xyz))]
    xyz[rs.randint(0, len(xyz), 3), rs.randint(0, 3, 3)] = [NAN, INF, -INF]
    return xyz


def compact(clouds, extra=0):
    """Clouds of B frames -> xyz with frame_offsets; `extra` rows of the last cloud lie beyond frame_offsets[B]."""
    cuts = np.cumsum([0] + [len(c) for c in clouds])
    cuts[-1] -= extra
    return dict(xyz=np.concatenate(clouds), frame_offsets=cuts.astype(np.int32))


# where frame 0 stands, call after call: a repeated pose (scroll by 0), one cell on, across zero into negative cells, a jump farther
# than any window here (everything reads 0), and on from there
DRIVE = ((0.3, 0.2, 0.1), (0.3, 0.2, 0.1), (0.8, 0.2, 0.2), (-0.7, -0.9, 2.5), (-1.3, -1.1, 2.6), (-30.0, 55.0, -1.0), (-30.2, 55.6, -1.2))


def drive(seed, nx, ny, n_bins, M, form, B=3, shared_pose=False, sensor=None, centre=None, masked=True, **changes):
    """B frames along DRIVE, each frame displaced and turned against frame 0, in one of the three forms of a cloud."""
    rs = np.random.RandomState(seed)
    p = params(M=M, nx=nx, ny=ny, n_bins=n_bins, **changes)
    frames = []
    for step, (x, y, heading) in enumerate(DRIVE):
        n_ground, n_wall = (120, 60) if nx * ny < 100 else (500, 200)
        clouds = [fan(rs, n_ground, n_wall, wall=1.5 if nx * ny < 100 else 6.0, reach=2.5 if nx * ny < 100 else 11.0) for _ in range(B)]
        T = np.stack([pose(x + 0.6 * b, y - 0.4 * b, heading + 0.7 * b, 0.01 * b) for b in range(B)])
        kw = dict(T=T[0] if shared_pose else T, sensor=sensor, centre=centre)
        if form == "organised":
            rows = min(len(c) for c in clouds)
            kw.update(xyz=np.concatenate([c[:rows] for c in clouds]), rows_per_frame=rows, valid=(rs.uniform(size=B * rows) > 0.1).astype(np.uint8))
        else:
            kw.update(compact(clouds, extra=5))
            if masked:
                kw.update(valid=(rs.uniform(size=len(kw["xyz"])) > 0.1).astype(np.uint8))
        if step == 4 and B == 3 and form == "compact":
            kw["frame_offsets"][2] = kw["frame_offsets"][1]                      # an empty frame
        frames.append(kw)
    return dict(params=p, B=B, frames=frames, form=form)


def planted():
    """One frame of hand-placed rows around a sensor that stands exactly on a cell centre, without a transform.  max_range 4; the
    window of 5 x 7 cells is the world cells -2 .. 2 by -3 .. 3: -1.0 <= X < 1.5 and -1.5 <= Y < 2.0."""
    f32 = np.float32
    up, down = (lambda v: float(np.nextafter(f32(v), f32(INF)))), (lambda v: float(np.nextafter(f32(v), f32(-INF))))
    sx = sy = 0.25
    rows = [
        # the four diagonals, |dx| == |dy|: s is +1 or -1, and +1 is the clamp
        (sx + 1, sy + 1, 1.0), (sx - 1, sy + 1, 1.0), (sx - 1, sy - 1, 1.0), (sx + 1, sy - 1, 1.0),
        # the same bearings again, nearer and farther: the minimum and the maximum have something to decide
        (sx + 0.5, sy + 0.5, 1.0), (sx - 0.25, sy + 0.25, 0.0), (sx - 1.25, sy - 1.25, 0.0), (sx + 0.75, sy - 0.75, 1.5),
        # on the axes: s == 0; the point at the sensor itself (r2 == 0) is left out
        (sx + 1, sy, 1.0), (sx, sy + 1, 1.0), (sx - 1, sy, 1.0), (sx, sy - 1, 1.0), (sx, sy, 1.0),
        # exactly at max_range: in; one step beyond: out
        (sx + 4.0, sy, 1.0), (up(sx + 4.0), sy, 1.0), (sx, sy - 4.0, 0.0), (sx, down(sy - 4.0), 0.0),
        # the band's edges: z_lo, z_hi and z_floor belong to it, one step outside does not
        (0.6, 0.1, 0.25), (0.6, 0.15, down(0.25)), (0.6, -0.1, 2.0), (0.6, -0.15, up(2.0)), (0.1, 0.6, -0.5), (0.15, 0.6, down(-0.5)),
        # the window's edges: the lower ones belong to it, the upper ones do not
        (-1.0, 0.3, 1.0), (down(-1.0), 0.3, 1.0), (1.5, 0.3, 1.0), (down(1.5), 0.3, 1.0), (0.3, -1.5, 1.0), (0.3, down(-1.5), 1.0), (0.3, 2.0, 1.0),
        (0.3, down(2.0), 1.0),
        # not finite
        (NAN, 0.3, 1.0), (0.3, INF, 1.0), (0.3, 0.3, NAN), (-INF, 0.3, 1.0),
        # masked out by valid; beyond frame_offsets[B]
        (0.9, 0.9, 1.0), (0.9, -0.9, 1.0), (-0.9, 0.9, 1.0),
    ]
    xyz = np.array(rows, dtype=np.float32)
    n = len(rows)
    valid = np.ones(n, np.uint8)
    valid[n - 3] = 0
    frame = dict(xyz=xyz, frame_offsets=np.array([0, n - 2], np.int32), valid=valid, T=None, sensor=np.array([sx, sy, 0.0]), centre=None)
    return dict(params=params(nx=5, ny=7, n_bins=8, max_range=4.0, min_points=1), B=1, frames=[frame, frame], form="compact")


def saturation():
    """The same wall l_max / l_occ + 2 times, then the same ground without the wall until every cell of it has turned free."""
    p = params(nx=16, ny=16, n_bins=64, max_range=8.0)
    with_wall = compact([fan(np.random.RandomState(5), 400, 300, wall=2.0, reach=3.5)])
    without = compact([fan(np.random.RandomState(6), 2500, 0, wall=None, reach=3.5)])
    kw = dict(T=pose(0.1, 0.1, 0.0), sensor=None, centre=None)
    n_occ = p["l_max"] // p["l_occ"] + 2
    n_free = (p["l_max"] + p["free_at"] + p["l_free"] - 1) // p["l_free"]
    return dict(params=p, B=1, frames=[dict(with_wall, **kw)] * n_occ + [dict(without, **kw)] * n_free, form="compact", n_occ=n_occ)


def contention(n=4096):
    """Every row in one cell and, seen from the sensor, one bin; a handful of ranges among them."""
    rs = np.random.RandomState(8)
    xyz = np.stack([3.1 + rs.randint(0, 4, n) / 16.0, 0.05 + rs.randint(0, 2, n) / 64.0, 0.5 + rs.randint(0, 3, n) / 4.0], axis=1).astype(np.float32)
    frame = dict(xyz=xyz, frame_offsets=np.array([0, n], np.int32), valid=None, T=None, sensor=None, centre=None)
    return dict(params=params(nx=16, ny=16, n_bins=8), B=1, frames=[frame], form="compact")


def nothing():
    frame = dict(xyz=np.zeros((0, 3), np.float32), frame_offsets=np.zeros(4, np.int32), valid=None, T=None, sensor=None, centre=None)
    return dict(params=params(M=3, nx=5, ny=7, n_bins=4), B=3, frames=[frame], form="compact")


def bad_poses():
    """Three maps; after two good calls the centre of map 1 is NaN for one call, then the sensor of frame 2, then all is well again."""
    case = drive(31, 16, 12, 64, 3, "compact", sensor=np.zeros((3, 3)), centre=np.array([[1.0, 0.0, 0.0]] * 3))
    case["frames"] = case["frames"][:5]
    centre = case["frames"][2]["centre"].copy()
    centre[1, 0] = NAN
    case["frames"][2]["centre"] = centre
    sensor = case["frames"][3]["sensor"].copy()
    sensor[2, 1] = INF
    case["frames"][3]["sensor"] = sensor
    return case


def sequence_cases():
    one_rig = np.array([[0.0, 0.0, 0.0], [0.25, -0.25, 0.0], [-0.5, 0.5, 0.25]])
    return {
        "40 x 36, 720 bins, a map per frame, compact": drive(11, 40, 36, 720, 3, "compact"),
        "40 x 36, 8 bins, one rig, bare xyz": drive(12, 40, 36, 8, 1, "bare", shared_pose=True, sensor=one_rig, centre=np.array([2.0, 0.0, 0.0]),
                                                     masked=False),
        "40 x 36, 4 bins, a map per frame, organised": drive(13, 40, 36, 4, 3, "organised", centre=np.array([[1.0, 0.0, 0.0]] * 3)),
        "5 x 7, 8 bins, a map per frame, organised": drive(14, 5, 7, 8, 3, "organised", max_range=3.0),
        "5 x 7, 720 bins, one rig, compact": drive(15, 5, 7, 720, 1, "compact", sensor=one_rig, max_range=3.0, min_points=1),
        "5 x 7, 4 bins, one frame, bare xyz": drive(16, 5, 7, 4, 1, "bare", B=1, shared_pose=True, max_range=3.0),
    }


def all_cases():
    return dict(sequence_cases(), **{"planted edges": planted(), "saturation": saturation(), "contention": contention(), "no rows": nothing(),
                                     "bad poses": bad_poses()})
