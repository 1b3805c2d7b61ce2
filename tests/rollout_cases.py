"""The shared cases of the local planner's tests: small scenes (a costmap from tests/field_ref.py, a cost-to-go from tests/nav_ref.py,
track tables with free and non-counting slots between the counting ones) and the restatement's outputs for them, made once and left
unchanged.  The shapes are the smallest that still reach every path of the kernels: windows 37 x 53 and 64 x 65 with negative origins;
K 1, 5 and 4095 (the largest that n_v <= 64 and an odd n_w reach under the cap of 4096); P 1, 63, 64, 65 and 256 (a lane's last pose, its second, its fourth); T 1, 64, 65 and 1024 (a wave's ballot, the
second segment, every chunk of the compaction); M 1 and 3."""
import math

import numpy as np

from tests import field_ref, nav_ref, rollout_ref

OCCUPIED_MASK, R = 1 << 2, 3
_CASES, _WANT = {}, {}


def pose(x, y, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, 0.0]])


def scene(seed, M, nx, ny, cell, origin, density=0.01, free_rows=3):
    """A state map with a few obstacle and unknown cells, free around the vehicle's row, and its distance field."""
    rng = np.random.default_rng(seed)
    state = np.ones((M, nx, ny), np.uint8)
    draw = rng.random((M, nx, ny))
    state[draw < density] = 2
    state[draw > 0.97] = 0
    i0, j0 = int(nx * 0.3), ny // 2
    state[:, max(i0 - free_rows, 0):i0 + free_rows + 1, max(j0 - free_rows, 0):j0 + free_rows + 1] = 1
    clear, cost_table = field_ref.tables(cell, R, inscribed=cell, inflation=R * cell, scale=2.0)
    f = field_ref.distance_field(state, OCCUPIED_MASK, R, 0, clear, cost_table)
    origin = np.tile(np.asarray(origin, np.int64), (M, 1)) + np.arange(M, dtype=np.int64)[:, None] * np.array([3, -2])
    return dict(state=state, dist2=f["dist2"], cost=f["cost"], origin=origin, cell=cell, M=M, nx=nx, ny=ny)


def vehicle(sc, seed, where=(0.3, 0.5)):
    """A pose per map: in the free patch, heading along +x with a small yaw."""
    rng = np.random.default_rng(seed)
    out = []
    for m in range(sc["M"]):
        ox, oy = sc["origin"][m]
        out.append(pose((ox + sc["nx"] * where[0] + 0.37) * sc["cell"], (oy + sc["ny"] * where[1] + 0.21) * sc["cell"], rng.uniform(-0.3, 0.3)))
    return np.stack(out)


def cost_to_go(sc, blocked_at=200):
    """nav_ref's togo towards a goal ahead; cells of cost blocked_at .. 252 are UNREACHED there and passable for a rollout."""
    goals = np.stack([[((ox + sc["nx"] * 0.85) * sc["cell"], (oy + sc["ny"] * 0.5) * sc["cell"])] for ox, oy in sc["origin"]])
    return nav_ref.nav_field(sc["cost"], goals, None, sc["origin"], sc["cell"], neutral=50, blocked_at=blocked_at, max_rounds=64,
                             with_next=False)["togo"]


def track_tables(sc, poses, seed, T, reach, nan_track=True):
    """tracks int32 [M,T,8], pos and vel fp64 [M,T,2]: free slots (NaN), tentative and confirmed ones, large and slow objects between
    the counting ones, positions within `reach` metres ahead of the vehicle."""
    rng = np.random.default_rng(seed)
    M = sc["M"]
    tracks = np.zeros((M, T, 8), np.int32)
    tracks[..., 4] = -1
    status = rng.choice([0, 1, 2], size=(M, T), p=[0.2, 0.2, 0.6])
    tracks[..., 0] = status
    tracks[..., 5] = np.where(status > 0, rng.integers(1, 100, size=(M, T)), 0)
    pos = poses[:, None, :2, 3] + rng.uniform(-0.2, 1.0, size=(M, T, 2)) * reach * np.array([1.0, 0.5]) - np.array([0.0, 0.2 * reach])
    vel = rng.uniform(-0.3, 0.3, size=(M, T, 2))
    vel[rng.random((M, T)) < 0.15] *= 0.05                                 # slow ones
    free = status == 0
    pos[free], vel[free] = np.nan, np.nan
    if nan_track:
        live = np.argwhere(status[0] == 2)
        if live.size:
            pos[0, live[len(live) // 2, 0], 1] = np.nan                   # a confirmed slot whose pos is not finite
    return tracks, pos, vel


def make(seed, M, nx, ny, origin, v, w, P, T=0, nav=False, accel=None, outside_blocks=True, dt=0.1, keep_out=0.6, where=(0.3, 0.5),
         weights=None, min_status=2, nan_pose=None, nan_twist=None, cell=0.5, band=None):
    sc = scene(seed, M, nx, ny, cell, origin)
    if band is not None:            # cells (i0, i1, j0, j1) raised to cost 220: passable for a rollout (< 253), impassable for cost_to_go (>= 200)
        i0, i1, j0, j1 = band
        sc["cost"] = sc["cost"].copy()
        sc["cost"][:, i0:i1, j0:j1] = np.maximum(sc["cost"][:, i0:i1, j0:j1], 220)
    poses = vehicle(sc, seed + 1, where)
    s = rollout_ref.spec(v=v, w=w, dt=dt, n_poses=P, track_dt=0.25, keep_out=keep_out, min_speed=0.05, max_object_cells=64,
                         min_status=min_status, accel=accel, outside_blocks=outside_blocks, weights=weights, cell=cell)
    case = dict(spec=s, scene=sc, pose=poses, togo=cost_to_go(sc) if nav else None, tracks=None, pos=None, vel=None, twist=None)
    if T:
        case["tracks"], case["pos"], case["vel"] = track_tables(sc, poses, seed + 2, T, reach=v[1] * dt * P + 1.0)
    if accel is not None:
        rng = np.random.default_rng(seed + 3)
        case["twist"] = np.stack([rng.uniform(v[0], v[1], M), rng.uniform(-w[0], w[0], M)], axis=1)
    if nan_pose is not None:
        case["pose"][nan_pose, 1, 3] = np.nan
    if nan_twist is not None:
        case["twist"][nan_twist, 0] = np.nan
    return case


def all_cases():
    """name -> case.  Made once."""
    if not _CASES:
        c = _CASES
        c["37 x 53, K 5, P 63, no tracks, no nav"] = make(1, 1, 37, 53, (-20, -30), (1.0, 1.0, 1), (0.8, 5), 63)
        c["64 x 65, 3 maps, K 45, P 64, T 64, nav, twist"] = make(2, 3, 64, 65, (-70, 11), (0.5, 2.5, 5), (0.9, 9), 64, T=64, nav=True,
                                                                 accel=(8.0, 6.0), weights=dict(togo=1, max_cost=3, sum_cost=2, slow=7, turn=5))
        c["K 1, P 1, T 1"] = make(3, 1, 37, 53, (5, -60), (1.5, 1.5, 1), (0.0, 1), 1, T=1, nav=True)
        # 4095 = 63 x 65 is the largest K that n_v <= 64 and an odd n_w <= 129 reach below the cap of 4096; 4096 itself has no such factors
        c["K 4095, P 5, T 65"] = make(4, 1, 37, 53, (-20, -30), (0.2, 6.0, 63), (1.5, 65), 5, T=65, nav=True, dt=0.3, keep_out=1.0,
                                      weights=dict(slow=1, turn=1))
        c["K 5, P 65, T 1024"] = make(5, 1, 64, 65, (-33, -32), (1.0, 2.0, 1), (0.6, 5), 65, T=1024, keep_out=0.15, min_status=1)
        c["3 maps, K 15, P 256, T 65, leaves the window, outside passes"] = make(6, 3, 37, 53, (-20, -30), (0.5, 2.0, 3), (0.7, 5), 256, T=65,
                                                                                nav=True, outside_blocks=False, dt=0.08, keep_out=0.3)
        c["K 15, P 65, no tracks, leaves the window, outside blocks"] = make(7, 1, 37, 53, (-20, -30), (0.5, 3.0, 3), (0.7, 5), 65,
                                                                            where=(0.7, 0.5))
        c["3 maps, a NaN pose and a NaN twist"] = make(8, 3, 37, 53, (-20, -30), (0.5, 2.0, 3), (0.7, 5), 20, T=5, accel=(50.0, 50.0),
                                                      outside_blocks=False, nan_pose=0, nan_twist=1)
        c["K 9, P 128, T 256, nav"] = make(9, 1, 64, 65, (-33, -32), (0.5, 1.5, 3), (0.5, 3), 128, T=256, nav=True, keep_out=0.25)
        # rollouts that are clear and end on cells of cost 220, where the cost-to-go is UNREACHED: not valid with a togo weight, valid without
        for name, weights in (("ends UNREACHED, togo weight 1", dict(togo=1, sum_cost=0)), ("ends UNREACHED, togo weight 0", dict(togo=0, sum_cost=0, slow=1))):
            c[name] = make(10, 1, 37, 53, (-20, -30), (0.5, 3.0, 6), (0.3, 5), 30, nav=True, band=(18, 25, 18, 36), weights=weights)
    return _CASES


def arguments(case):
    """The keyword arguments of rollout_ref.plan_rollouts and plan_rollouts_loop."""
    sc = case["scene"]
    return dict(pose=case["pose"], origin=sc["origin"], cell=sc["cell"], cost=sc["cost"], togo=case["togo"], tracks=case["tracks"],
                pos=case["pos"], vel=case["vel"], twist=case["twist"])


def want_of(name):
    """The restatement's outputs of a case, computed once and left unchanged."""
    if name not in _WANT:
        case = all_cases()[name]
        _WANT[name] = rollout_ref.plan_rollouts(case["spec"], **arguments(case))
    return _WANT[name]
