"""Inputs for the bird's-eye-view tests, as NumPy arrays and plain numbers: the keyword arguments of tests/bev_ref.py's bev_grid.  Shared
by tests/test_bev_ref_cpu.py (restatement against a per-point loop) and tests/test_gpu_bev.py (kernels against the restatement)."""
import numpy as np

NAN, INF = float("nan"), float("inf")


def pose(rs, B=None):
    """A rotation and a translation as [3,4] (B None) or one per frame [B,3,4]."""
    def one():
        return np.concatenate([np.linalg.qr(rs.normal(size=(3, 3)))[0], rs.uniform(-1, 1, size=(3, 1))], axis=1)
    return one() if B is None else np.stack([one() for _ in range(B)])


def planted(**changes):
    """Three frames, the middle one empty, on a 5 x 7 grid of 0.5 m cells from (-1, 2); five more rows lie beyond frame_offsets[B].
    Cell (i, j) covers -1 + i / 2 <= x < .. + 0.5 and 2 + j / 2 <= y < .. + 0.5: every edge is an exact float."""
    rows = [
        # frame 0 -- cell (0, 0): equal heights at rows 1 and 3, below them row 0 and above nothing: row 1 wins
        (-0.9, 2.1, 1.0), (-0.8, 2.2, 1.5), (-0.7, 2.3, 1.25), (-0.6, 2.4, 1.5),
        # cell (1, 1): -0.0 at row 4 against +0.0 at row 5 and a negative height: rows 4 and 5 are equal, row 4 wins, z_max is +0.0
        (-0.3, 2.6, -0.0), (-0.2, 2.7, 0.0), (-0.4, 2.8, -2.0),
        # cell (2, 2): only negative heights, two of them equal
        (0.1, 3.2, -1.5), (0.2, 3.3, -0.5), (0.3, 3.4, -0.5), (0.4, 3.1, -3.0),
        # exactly on lower edges: x = 0.0 is the edge of i = 2, y = 2.0 that of j = 0; x = -1.0 and y = 2.0 the grid's own corner
        (0.0, 2.0, 0.75), (-1.0, 2.0, 0.5), (0.5, 4.5, 2.0),
        # exactly on the upper edges x = 1.5 and y = 5.5: outside; just below them: inside
        (1.5, 3.0, 9.0), (0.0, 5.5, 9.0), (1.4999999, 5.4999995, 3.0),
        # outside, non-finite coordinates, a height at fp32's largest value
        (-1.0000001, 3.0, 9.0), (0.2, 1.9999999, 9.0), (NAN, 3.0, 1.0), (0.2, INF, 1.0), (0.2, 3.0, NAN), (0.2, 3.0, -INF), (-INF, 3.0, 1.0),
        (1.2, 2.2, 3.4028235e38), (1.2, 2.3, -3.4028235e38),
        # frame 2 -- the same cells again in another frame, one row masked out by valid
        (-0.9, 2.1, 4.0), (-0.9, 2.1, 7.0), (-0.9, 2.1, 4.0), (0.6, 5.4, -0.0), (0.6, 5.4, -1e-30), (1.1, 2.1, 0.3), (1.1, 2.2, 0.3),
        (1.1, 2.3, 0.3),
        # beyond frame_offsets[B]: in no frame
        (-0.9, 2.1, 50.0), (0.0, 3.0, 50.0), (0.5, 4.0, 50.0), (1.0, 5.0, 50.0), (1.2, 2.2, 50.0),
    ]
    xyz = np.array(rows, dtype=np.float32)
    n = len(rows)
    valid = np.ones(n, dtype=np.uint8)
    valid[[2, 27]] = 0                                           # row 27 is frame 2's highest point of cell (0, 0)
    case = dict(xyz=xyz, B=3, x_min=-1.0, y_min=2.0, cell=0.5, nx=5, ny=7, frame_offsets=np.array([0, 26, 26, n - 5], dtype=np.int32),
                valid=valid, label=(np.arange(n) * 7 % 251).astype(np.uint8), T=None, z_lo=-INF, z_hi=INF, min_points=1, flip_x=False,
                flip_y=False)
    case.update(changes)
    return case


def planted_cases():
    rs = np.random.RandomState(3)
    shift = np.array([[1.0, 0, 0, 0.25], [0, 1.0, 0, -0.5], [0, 0, -1.0, 0.5]])          # exact: edges stay edges, heights change sign
    return {
        "plain": planted(),
        "no mask, no labels": planted(valid=None, label=None),
        "min_points 3": planted(min_points=3),
        "flip x": planted(flip_x=True),
        "flip y": planted(flip_y=True, min_points=3),
        "both flips": planted(flip_x=True, flip_y=True),
        "z band": planted(z_lo=-0.5, z_hi=1.5),
        "z_lo == z_hi": planted(z_lo=0.0, z_hi=0.0),
        "z_lo == z_hi == 0.3f": planted(z_lo=float(np.float32(0.3)), z_hi=float(np.float32(0.3)), min_points=3),
        "half-infinite band": planted(z_lo=-INF, z_hi=-0.5),
        "shared transform": planted(T=shift),
        "shared pose": planted(T=pose(rs), x_min=-2.0, y_min=-2.0, cell=0.8, nx=5, ny=7),
        "per-frame poses": planted(T=pose(rs, 3), x_min=-3.0, y_min=-3.0, cell=0.2, nx=16, ny=12, flip_x=True),
        "all frames empty": planted(frame_offsets=np.array([4, 4, 4, 4], dtype=np.int32)),
    }


def random_case(seed, B, n, nx, ny, cell=0.2, transform=None, organised=False):
    """n rows scattered over a little more than the grid; about a tenth masked out, a few non-finite, heights quantised so that equal
    heights meet in a cell.  organised: frames of n // B rows each (rows_per_frame) in place of frame_offsets; the rest belongs to no
    frame."""
    rs = np.random.RandomState(seed)
    x_min, y_min = -1.3, 0.7
    xyz = np.stack([rs.uniform(x_min - cell, x_min + (nx + 1) * cell, n), rs.uniform(y_min - cell, y_min + (ny + 1) * cell, n),
                    np.round(rs.normal(0.0, 2.0, n) * 4) / 4], axis=1).astype(np.float32)
    xyz[rs.randint(0, n, 5), rs.randint(0, 3, 5)] = [NAN, INF, -INF, NAN, INF]
    xyz[rs.randint(0, n, 6), 2] = [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0]
    case = dict(xyz=xyz, B=B, x_min=x_min, y_min=y_min, cell=cell, nx=nx, ny=ny, valid=(rs.uniform(size=n) > 0.1).astype(np.uint8),
                label=rs.randint(0, 256, n).astype(np.uint8), z_lo=-4.0, z_hi=5.0, min_points=2, flip_x=bool(seed & 1), flip_y=bool(seed & 2),
                T={None: None, "shared": pose(rs), "per frame": pose(rs, B)}[transform])
    if organised:
        case.update(frame_offsets=None, rows_per_frame=max(1, (n - 3) // B))
    else:
        cuts = np.sort(rs.randint(0, n - 10, B + 1))
        if B == 3:
            cuts[2] = cuts[1]                                    # an empty frame
        case.update(frame_offsets=cuts.astype(np.int32))
    if transform:
        case.update(x_min=-3.0, y_min=-3.0, cell=6.0 / max(nx, ny))
    return case


def random_cases():
    out = {}
    seed = 20
    for B in (1, 3):
        for (nx, ny), n in (((2, 2), 500), ((5, 7), 2000), ((16, 12), 1500)):
            for transform in (None, "shared", "per frame"):
                seed += 1
                out[f"B {B}, {nx} x {ny}, transform {transform}"] = random_case(seed, B, n, nx, ny, transform=transform)
            seed += 1
            out[f"B {B}, {nx} x {ny}, organised"] = random_case(seed, B, n, nx, ny, organised=True)
    return out


def all_cases():
    return dict(planted_cases(), **random_cases())
