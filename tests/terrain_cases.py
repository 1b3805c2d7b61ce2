"""Inputs for the terrain-map tests, as NumPy arrays and plain numbers.  A case is {'params': the numbers of a TerrainMap, 'B',
'frames': a list of the keyword arguments of tests/terrain_ref.py's update, one per call, in order, 'form'}.  Shared by
tests/test_terrain_ref_cpu.py (restatement against loops and closed forms), tests/test_terrain_cell_cpu.py (terrain_cell.h on the
host) and tests/test_gpu_terrain.py (kernels against the restatement)."""
import numpy as np

from tests.occupancy_cases import DRIVE, compact, pose

NAN, INF = float("nan"), float("inf")
# every number an exact binary fraction, so that edges are edges: a quantum of 1/64 m, a headroom of 128 quanta, step_max_q 16,
# slope2_max (2 * 0.5 * 0.25 * 64)^2 = 256
PARAMS = dict(M=1, nx=40, ny=36, cell=0.5, z_quantum=1.0 / 64, z_range=(-8.0, 8.0), max_range=12.0, headroom=2.0, min_points=2, w_max=3,
              step_max=0.25, slope_max=0.25)


def params(**changes):
    return dict(PARAMS, **changes)


def hills(rs, n_ground=600, n_box=120, n_over=40, reach=11.0):
    """Rolling ground seen from the origin of the points' frame (x forward, y left, z up) out to `reach` metres all around, a box of
    0.6 m on it, a canopy 3 m up (over the headroom), a few rows outside z_range, a few non-finite.  -> fp32 [n,3]."""
    x, y = rs.uniform(-reach, reach, n_ground), rs.uniform(-reach, reach, n_ground)
    rows = [np.stack([x, y, 0.4 * np.sin(0.5 * x) + 0.08 * y + rs.uniform(-0.02, 0.02, n_ground)], axis=1)]
    bx, by = rs.uniform(0.2 * reach, 0.35 * reach, n_box), rs.uniform(-0.1 * reach, 0.1 * reach, n_box)
    rows.append(np.stack([bx, by, 0.4 * np.sin(0.5 * bx) + 0.08 * by + rs.uniform(0.0, 0.6, n_box)], axis=1))
    ox, oy = rs.uniform(-0.3 * reach, 0.3 * reach, n_over), rs.uniform(-0.3 * reach, 0.3 * reach, n_over)
    rows.append(np.stack([ox, oy, rs.uniform(3.0, 4.0, n_over)], axis=1))
    rows.append(np.stack([rs.uniform(-2.0, 2.0, 6), rs.uniform(-2.0, 2.0, 6), np.array([9.0, -9.0, 20.0, -20.0, 8.5, -8.5])], axis=1))
    xyz = np.concatenate(rows).astype(np.float32)
    xyz = xyz[rs.permutation(len(xyz))]
    xyz[rs.randint(0, len(xyz), 3), rs.randint(0, 3, 3)] = [NAN, INF, -INF]
    return xyz


def drive(seed, nx, ny, M, form, B=3, shared_pose=False, sensor=None, centre=None, masked=True, **changes):
    """B frames along occupancy_cases.DRIVE -- a repeated pose, one cell on, into negative cells, a jump past the whole window, on
    from there --, each frame displaced and turned against frame 0, in one of the three forms of a cloud."""
    rs = np.random.RandomState(seed)
    p = params(M=M, nx=nx, ny=ny, **changes)
    small = nx * ny < 100
    frames = []
    for step, (x, y, heading) in enumerate(DRIVE):
        clouds = [hills(rs, 150, 40, 12, 2.5) if small else hills(rs) for _ in range(B)]
        T = np.stack([pose(x + 0.6 * b, y - 0.4 * b, heading + 0.7 * b, 0.25 * b - 0.125 * step) for b in range(B)])
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


def frame_of(xyz, **kw):
    """One frame of a compact cloud, without a transform unless given."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return dict(dict(xyz=xyz, frame_offsets=np.array([0, len(xyz)], np.int32), valid=None, T=None, sensor=None, centre=None), **kw)


def surface(height, nx, ny, cell=0.5, copies=2, origin=None):
    """`copies` rows at the centre of every cell of the window that a sensor at the origin gives (world cells -(nx // 2) .. by
    -(ny // 2) ..), at the height height(wx, wy) in metres, where wx, wy are integer arrays.  -> fp32 [nx * ny * copies, 3], cell by cell."""
    ox, oy = (-(nx // 2), -(ny // 2)) if origin is None else origin
    wx, wy = np.meshgrid(ox + np.arange(nx), oy + np.arange(ny), indexing="ij")
    z = np.broadcast_to(np.asarray(height(wx, wy), np.float64), wx.shape)
    one = np.stack([(wx + 0.5) * cell, (wy + 0.5) * cell, z], axis=-1).reshape(-1, 1, 3)
    return np.repeat(one, copies, axis=1).reshape(-1, 3).astype(np.float32)


def planted():
    """One frame of hand-placed rows around a sensor that stands exactly on a cell centre, without a transform.  max_range 4; the
    window of 5 x 7 cells is the world cells -2 .. 2 by -3 .. 3: -1.0 <= X < 1.5 and -1.5 <= Y < 2.0.  min_points 1."""
    f32 = np.float32
    up, down = (lambda v: float(np.nextafter(f32(v), f32(INF)))), (lambda v: float(np.nextafter(f32(v), f32(-INF))))
    sx = sy = 0.25
    q = 1.0 / 64
    rows = [
        # the point at the sensor itself (r2 == 0) counts; a pair in its cell
        (sx, sy, 0.0), (sx + 0.125, sy, 0.25),
        # Z exactly on a quantum boundary, one step under it, and negative ones: floor, not truncation
        (0.6, 0.1, 3 * q), (0.6, 0.15, down(3 * q)), (0.6, -0.1, -3 * q), (0.6, -0.15, down(-3 * q)), (0.6, -0.3, up(-3 * q)),
        # both ends of z_range belong to it, one step outside does not
        (0.1, 0.6, 8.0), (0.15, 0.6, up(8.0)), (0.1, 1.1, -8.0), (0.15, 1.1, down(-8.0)),
        # the headroom: lo + head_q counts towards hi, one quantum more does not
        (-0.6, 0.1, 1.0), (-0.6, 0.15, 3.0), (-0.6, 0.2, 3.0 + q), (-0.6, -0.6, 1.0), (-0.6, -0.7, down(3.0)), (-0.6, -0.8, 5.0),
        # the window's edges: the lower ones belong to it, the upper ones do not
        (-1.0, 0.3, 1.0), (down(-1.0), 0.3, 1.0), (1.5, 0.3, 1.0), (down(1.5), 0.3, 1.0), (0.3, -1.5, 1.0), (0.3, down(-1.5), 1.0), (0.3, 2.0, 1.0),
        (0.3, down(2.0), 1.0),
        # exactly on a cell boundary inside the window
        (0.5, 0.5, 0.5), (0.5, down(0.5), 0.5), (down(0.5), 0.5, 0.5), (-0.5, -0.5, 0.125), (down(-0.5), down(-0.5), 0.125),
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
    return dict(params=params(nx=5, ny=7, max_range=4.0, min_points=1), B=1, frames=[frame, frame], form="compact")


def range_edge():
    """A sensor on a cell centre and max_range 2: the rows exactly at max_range are in, one step beyond is out (min_points 1)."""
    f32 = np.float32
    up, down = (lambda v: float(np.nextafter(f32(v), f32(INF)))), (lambda v: float(np.nextafter(f32(v), f32(-INF))))
    # the row beyond falls into the cell of the row at the range and lies lower: it would show as the cell's ground
    rows = [(2.25, 0.25, 1.0), (up(2.25), 0.25, 0.5), (0.25, -1.75, 0.5), (0.25, down(-1.75), 0.25), (-1.75, 0.25, 0.25), (down(-1.75), 0.25, 0.0)]
    frame = frame_of(np.array(rows), sensor=np.array([0.25, 0.25, 0.0]))
    return dict(params=params(nx=16, ny=16, max_range=2.0, min_points=1), B=1, frames=[frame], form="compact")


def contention(n=4096):
    """Every row in one cell, with n distinct heights in shuffled order: -n/2 .. n/2 - 1 quanta, so lo = -n/2 and hi = lo + head_q."""
    rs = np.random.RandomState(8)
    z = (rs.permutation(n) - n // 2) / 64.0
    xyz = np.stack([3.1 + rs.randint(0, 4, n) / 16.0, 0.05 + rs.randint(0, 2, n) / 64.0, z], axis=1).astype(np.float32)
    return dict(params=params(nx=16, ny=16, z_range=(-40.0, 40.0)), B=1, frames=[frame_of(xyz), frame_of(xyz[::-1].copy())], form="compact")


def runs(n=1003):
    """Rows in image order: runs of equal cells of every length from 1 to 150, so that they start, end and cross at every lane of a
    wave and across the workgroups; a row count that is no multiple of 64 or 256; heights that fall and rise inside a run."""
    rs = np.random.RandomState(9)
    rows, c = [], 0
    while len(rows) < n:
        length = 1 + (c * 37) % 150
        wx, wy = -8 + c % 16, -8 + (c // 16) % 16
        for k in range(length):
            rows.append(((wx + rs.uniform(0.1, 0.9)) * 0.5, (wy + rs.uniform(0.1, 0.9)) * 0.5, 0.02 * ((k * 7) % 11) - 0.1 * (c % 3) + (3.0 if k % 29 == 5 else 0)))
        c += 1
    xyz = np.array(rows[:n], np.float32)
    return dict(params=params(nx=16, ny=16), B=1, frames=[frame_of(xyz), frame_of(xyz)], form="compact")


def rig():
    """Two frames of a rig (M == 1) that look at the same cells from two sensors: each brings one row per cell, so a cell is observed
    (min_points 2) only because both feed it, and lo comes from one frame, hi from the other."""
    nx = ny = 12
    low = surface(lambda wx, wy: 0.0625 * wx, nx, ny, copies=1)
    high = surface(lambda wx, wy: 0.0625 * wx + 0.125, nx, ny, copies=1)
    both = compact([low, high[::-1].copy()])
    sensor = np.array([[0.0, 0.0, 0.0], [0.25, -0.25, 0.0]])
    return dict(params=params(M=1, nx=nx, ny=ny), B=2, frames=[dict(both, valid=None, T=None, sensor=sensor, centre=None)] * 2, form="compact")


def nothing():
    frame = dict(xyz=np.zeros((0, 3), np.float32), frame_offsets=np.zeros(4, np.int32), valid=None, T=None, sensor=None, centre=None)
    return dict(params=params(M=3, nx=5, ny=7), B=3, frames=[frame], form="compact")


def saturation():
    """The same flat ground w_max + 2 times, then ground 64 quanta higher four times: the weight stops at w_max and the filter then
    moves by 1 / (w_max + 1) of what is left, with floor division."""
    nx = ny = 8
    flat, raised = surface(lambda wx, wy: -0.5, nx, ny), surface(lambda wx, wy: 0.5 - 1.0 / 64, nx, ny)
    p = params(nx=nx, ny=ny)
    return dict(params=p, B=1, frames=[frame_of(flat)] * (p["w_max"] + 2) + [frame_of(raised)] * 4, form="compact")


def bad_poses():
    """Three maps; after two good calls the centre of map 1 is NaN for one call, then the sensor of frame 2, then all is well again."""
    case = drive(31, 16, 12, 3, "compact", sensor=np.zeros((3, 3)), centre=np.array([[1.0, 0.0, 0.0]] * 3))
    case["frames"] = case["frames"][:5]
    centre = case["frames"][2]["centre"].copy()
    centre[1, 0] = NAN
    case["frames"][2]["centre"] = centre
    sensor = case["frames"][3]["sensor"].copy()
    sensor[2, 1] = INF
    case["frames"][3]["sensor"] = sensor
    return case


def skipped_first():
    """The very first call of a map is skipped (a NaN pose): it reports nothing known; then a good call."""
    good = frame_of(surface(lambda wx, wy: 0.25, 5, 7))
    return dict(params=params(nx=5, ny=7), B=1, frames=[dict(good, T=np.full((3, 4), NAN)), good], form="compact")


def ramp_cloud(slope=0.1, box=None, length=16.0, half_width=3.0, step=0.125):
    """A ramp that rises by `slope` along x from the sensor on, sampled every `step` metres; box = (x0, x1, y0, y1, height): a box of
    that height standing on it, its top and its sides sampled as well.  -> fp32 [n,3], in image-like order (far rows first)."""
    xs, ys = np.arange(length - step / 2, 0.0, -step), np.arange(-half_width + step / 2, half_width, step)
    x, y = (a.reshape(-1) for a in np.meshgrid(xs, ys, indexing="ij"))
    z = slope * x
    if box is not None:
        x0, x1, y0, y1, height = box
        on = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
        z = np.where(on, z + height * ((np.arange(len(z)) % 4) / 3.0), z)           # the sides and the top
    return np.stack([x, y, z], axis=1).astype(np.float32)


def sequence_cases():
    one_rig = np.array([[0.0, 0.0, 0.0], [0.25, -0.25, 0.0], [-0.5, 0.5, 0.25]])
    return {
        "40 x 36, a map per frame, compact": drive(11, 40, 36, 3, "compact"),
        "40 x 36, one rig, bare xyz": drive(12, 40, 36, 1, "bare", shared_pose=True, sensor=one_rig, centre=np.array([2.0, 0.0, 0.0]), masked=False),
        "40 x 36, a map per frame, organised": drive(13, 40, 36, 3, "organised", centre=np.array([[1.0, 0.0, 0.0]] * 3), w_max=15),
        "5 x 7, a map per frame, organised": drive(14, 5, 7, 3, "organised", max_range=3.0),
        "5 x 7, one rig, compact": drive(15, 5, 7, 1, "compact", sensor=one_rig, max_range=3.0, min_points=1),
        "5 x 7, one frame, bare xyz": drive(16, 5, 7, 1, "bare", B=1, shared_pose=True, max_range=3.0, headroom=0.0, step_max=0.0, slope_max=0.0),
    }


def all_cases():
    return dict(sequence_cases(), **{"planted edges": planted(), "range edge": range_edge(), "contention": contention(), "runs": runs(), "rig": rig(), "no rows": nothing(),
                                     "saturation": saturation(), "bad poses": bad_poses(), "skipped first": skipped_first()})
