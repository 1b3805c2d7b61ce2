"""CPU: tests/rollout_ref.py, the NumPy restatement of crd_plan_rollouts (include/camradepth_hip.h), held to a plain Python loop over
candidates, poses and tracks, to the closed form and to a numerical integration of the unicycle for its host tables, to the behaviour
a local planner owes (the fastest straight rollout on empty ground, a turn before a wall, a stop when nothing is left, a crossing track
met where the two meet, the dynamic window, symmetry) and to the restatements of the stages it reads (field_ref.check_paths on its 'xy',
nav_ref's cells on its ends)."""
import math

import numpy as np
import pytest

from tests import field_ref, nav_ref, rollout_cases, rollout_ref
from tests.rollout_ref import ADMISSIBLE, CLEAR, CLEAR_STATIC, NO_CANDIDATE, NOT_FINITE, UNREACHED, VALID

EPS = float(np.finfo(np.float64).eps)
CELL, NX, NY, ORIGIN = 0.5, 60, 60, np.array([[-30, -30]], np.int64)          # the window is [-15, 15) x [-15, 15) metres


def ground(walls=()):
    """A costmap of zeros with lethal cells at the (i, j) ranges given."""
    cost = np.zeros((1, NX, NY), np.uint8)
    for i0, i1, j0, j1 in walls:
        cost[0, i0:i1, j0:j1] = 254
    return cost


def towards(cost, x, y, blocked_at=253):
    return nav_ref.nav_field(cost, np.array([[[x, y]]]), None, ORIGIN, CELL, blocked_at=blocked_at, with_next=False)["togo"]


def run(s, cost, pose=None, **kw):
    pose = rollout_cases.pose(-10.0, 0.25, 0.0)[None] if pose is None else pose
    return rollout_ref.plan_rollouts(s, pose, ORIGIN, CELL, cost, **kw)


def one_track(pos, vel, status=2, n_cells=10, slot=3, T=6):
    tracks = np.zeros((1, T, 8), np.int32)
    tracks[..., 4] = -1
    p, v = np.full((1, T, 2), np.nan), np.full((1, T, 2), np.nan)
    tracks[0, slot, 0], tracks[0, slot, 5] = status, n_cells
    p[0, slot], v[0, slot] = pos, vel
    return dict(tracks=tracks, pos=p, vel=v)


# ---- the restatement against the plain loop ---------------------------------------------------------------------------------

SMALL = {
    "2 maps, nav, tracks, twist": lambda: rollout_cases.make(21, 2, 37, 53, (-20, -30), (0.5, 2.5, 3), (0.9, 5), 20, T=12, nav=True,
                                                            accel=(8.0, 6.0), weights=dict(togo=1, max_cost=3, sum_cost=2, slow=7, turn=5)),
    "outside passes, tentative tracks": lambda: rollout_cases.make(22, 1, 37, 53, (-20, -30), (0.5, 3.0, 3), (0.7, 5), 40, T=9,
                                                                  outside_blocks=False, min_status=1, where=(0.7, 0.5)),
    "a NaN pose and a NaN twist": lambda: rollout_cases.all_cases()["3 maps, a NaN pose and a NaN twist"],
    "K 1, P 1, T 1": lambda: rollout_cases.all_cases()["K 1, P 1, T 1"],
}


@pytest.mark.parametrize("name", list(SMALL))
def test_the_restatement_equals_the_plain_loop(name):
    case = SMALL[name]()
    kw = rollout_cases.arguments(case)
    fast, slow = rollout_ref.plan_rollouts(case["spec"], **kw), rollout_ref.plan_rollouts_loop(case["spec"], **kw)
    for k, v in slow.items():
        assert fast[k].dtype == v.dtype and fast[k].shape == v.shape and fast[k].tobytes() == v.tobytes(), (name, k, fast[k], v)


def test_the_shared_cases_reach_every_branch():
    want = {n: rollout_cases.want_of(n) for n in rollout_cases.all_cases()}
    flat = lambda k: np.concatenate([w[k].reshape(-1) for w in want.values()])              # noqa: E731
    assert (flat("best") >= 0).any() and (flat("best") < 0).any()
    assert {1, 2, 3} <= set(flat("info").reshape(-1, 8)[:, 4].tolist()) | {1, 2} and 0 in flat("info").reshape(-1, 8)[:, 4]
    assert (flat("first_track") >= 0).any() and (flat("first_track") < 0).any() and (flat("first_blocked") > 0).any()
    assert (flat("end_togo") == UNREACHED).any() and (flat("end_togo") != UNREACHED).any()
    flags = flat("flags")
    assert ((flags & CLEAR_STATIC) != 0).any() and (((flags & CLEAR_STATIC) != 0) & ((flags & CLEAR) == 0)).any()       # a track alone blocks
    assert ((flags & ADMISSIBLE) == 0).any() and (((flags & CLEAR) != 0) & ((flags & VALID) == 0)).any()
    # the third clause of VALID decides: admissible and clear rollouts that end where the cost-to-go is UNREACHED
    for name, n_lost in (("ends UNREACHED, togo weight 1", 8), ("ends UNREACHED, togo weight 0", 0)):
        w = want[name]
        f, end = w["flags"][0], w["end_togo"][0]
        open_end = ((f & ADMISSIBLE) != 0) & ((f & CLEAR) != 0) & (end == UNREACHED)
        assert open_end.sum() == 8 and w["info"][0, 2] - w["info"][0, 3] == n_lost and ((f[open_end] & VALID) != 0).all() == (n_lost == 0), name
        assert w["best"][0] >= 0 and (n_lost == 0 or not open_end[w["best"][0]]), name
    shapes = {(c["spec"]["v"][2] * c["spec"]["w"][1], c["spec"]["n_poses"], 0 if c["tracks"] is None else c["tracks"].shape[1], c["scene"]["M"])
              for c in rollout_cases.all_cases().values()}
    assert {1, 5, 4095} <= {s[0] for s in shapes} and {1, 63, 64, 65, 256} <= {s[1] for s in shapes}
    assert {0, 1, 64, 65, 1024} <= {s[2] for s in shapes} and {1, 3} <= {s[3] for s in shapes}


# ---- the host tables --------------------------------------------------------------------------------------------------------

TABLE_SPECS = (dict(v=(0.0, 2.0, 8), w=(1.0, 17), dt=0.1, n_poses=32), dict(v=(0.3, 6.0, 5), w=(2.5, 9), dt=0.05, n_poses=256),
               dict(v=(1.5, 1.5, 1), w=(0.01, 3), dt=0.25, n_poses=64))


@pytest.mark.parametrize("changes", TABLE_SPECS)
def test_host_tables(changes):
    s = rollout_ref.spec(**changes)
    vw, arc, tau = rollout_ref.host_tables(s)
    (v_min, v_max, n_v), (w_max, n_w), dt, P = s["v"], s["w"], s["dt"], s["n_poses"]
    c = (n_w - 1) // 2
    assert vw.shape == (n_v * n_w, 2) and arc.shape == (n_v * n_w, P, 2) and tau.tolist() == [(p + 1) * dt / dt for p in range(P)]
    assert vw[0, 0] == v_min and vw[c::n_w, 1].tobytes() == np.zeros(n_v).tobytes()           # the centre column is exactly +0.0
    assert (vw[:, 1].reshape(n_v, n_w) == -vw[:, 1].reshape(n_v, n_w)[:, ::-1]).all()         # and the others mirror each other exactly
    t64 = np.array([(p + 1) * dt for p in range(P)])
    for k in range(n_v * n_w):
        v, w = vw[k]
        if w == 0.0:                                                                          # straight rows are exact
            assert arc[k, :, 0].tobytes() == (np.float64(v) * t64).tobytes() and arc[k, :, 1].tobytes() == np.zeros(P).tobytes()
            continue
        # The closed form in long double from the same fp64 v, w and dt.  With u = EPS / 2, reach = |v| t (the length driven, which
        # bounds |x| and |y|) and r = v / w, so that |r| |w t| = reach:  fl(t) and fl(w t) each err by u relatively, which moves the
        # argument by 2 u |w t| and the sine or cosine by no more; libm's sin and cos and the subtraction 1 - cos add u each, absolutely
        # (|sin|, |cos| <= 1, 1 - cos <= 2); the quotient r and the last product add u relatively each.  Hence
        #   |x error| <= |r| (2 u |w t| + u) + 2 u |x| <= u (4 reach + |r|)   and   |y error| <= |r| (2 u |w t| + 3 u) + 2 u |y| <= u (4 reach + 3 |r|)
        # -- the |r| term is the cancellation in 1 - cos(w t) for small w t, which eps * reach alone does not cover.
        ld = np.longdouble
        t = ld(np.arange(1, P + 1)) * ld(dt)
        x_ref, y_ref = ld(v) / ld(w) * np.sin(ld(w) * t), ld(v) / ld(w) * (1 - np.cos(ld(w) * t))
        reach, r = abs(v) * t64, abs(v / w)
        bound = EPS / 2 * (4 * reach + 3 * r) + 8 * float(np.finfo(ld).eps) * (reach + r)    # + the long double's own rounding
        assert (np.abs(arc[k, :, 0] - x_ref) <= bound).all() and (np.abs(arc[k, :, 1] - y_ref) <= bound).all(), k
        # The unicycle x' = v cos(th), y' = v sin(th), th = w t integrated by the composite midpoint rule with step h = dt / n: its
        # error over [0, t] is at most t h^2 / 24 max|f''| = t h^2 |v| w^2 / 24 for either component (+ the rounding of n P terms).
        n = 8
        h = dt / n
        mids = (np.arange(n * P) + 0.5) * h
        x_mid = np.cumsum(v * np.cos(w * mids) * h).reshape(P, n)[:, -1]
        y_mid = np.cumsum(v * np.sin(w * mids) * h).reshape(P, n)[:, -1]
        rule = t64 * h * h * abs(v) * w * w / 24 + 4 * EPS * n * P * reach
        assert (np.abs(arc[k, :, 0] - x_mid) <= rule + bound).all() and (np.abs(arc[k, :, 1] - y_mid) <= rule + bound).all(), k
    assert rollout_ref.host_tables(rollout_ref.spec(track_dt=0.25, **changes))[2].tolist() == [(p + 1) * dt / 0.25 for p in range(P)]


# ---- behaviour --------------------------------------------------------------------------------------------------------------

PLAN = dict(v=(0.5, 2.0, 4), w=(0.8, 5), dt=0.1, n_poses=30)


def test_empty_ground_with_a_goal_ahead_drives_straight_at_full_speed():
    cost = ground()
    out = run(rollout_ref.spec(**PLAN), cost, togo=towards(cost, 12.0, 0.25))
    assert out["best"][0] == 3 * 5 + 2 and out["command"][0].tolist() == [2.0, 0.0]
    assert out["info"][0, :5].tolist() == [20, 20, 20, 20, 0] and out["score"][0] == out["scores"][0].min()


def test_a_wall_ahead_blocks_every_straight_rollout_and_a_turn_is_picked():
    cost = ground([(12, 14, 20, 41)])                                          # x in [-9, -8), y in [-5, 5.5): 1 m ahead of the vehicle
    out = run(rollout_ref.spec(**PLAN), cost, togo=towards(cost, 12.0, 0.25))
    assert (out["first_blocked"][0, 2::5] >= 0).all() and (out["first_track"][0] == -1).all()
    assert out["best"][0] >= 0 and out["best"][0] % 5 != 2 and out["first_blocked"][0, out["best"][0]] == -1
    assert out["command"][0, 1] != 0.0 and out["info"][0, 4] == 0


def test_a_crossing_track_blocks_where_the_two_meet():
    """The vehicle drives +x at 1 m/s from (-10, 0), the track +y at 1 m/s (0.25 m per update of 0.25 s) from (-7, -3): at time t they
    are sqrt(2) |t - 3| apart, within keep_out = 0.3 from t = 2.8 on, which is pose 27."""
    s = rollout_ref.spec(v=(1.0, 1.0, 1), w=(0.0, 1), dt=0.1, n_poses=40, track_dt=0.25, keep_out=0.3)
    pose = rollout_cases.pose(-10.0, 0.0, 0.0)[None]
    assert [p for p in range(40) if math.sqrt(2.0) * abs((p + 1) * 0.1 - 3.0) <= 0.3][0] == 27
    out = run(s, ground(), pose, **one_track((-7.0, -3.0), (0.0, 0.25)))
    assert out["first_blocked"][0].tolist() == [27] and out["first_track"][0].tolist() == [3]
    assert out["info"][0, :5].tolist() == [1, 1, 0, 0, NO_CANDIDATE] and out["best"][0] == -1
    away = run(s, ground(), pose, **one_track((-7.0, -3.0), (0.0, -0.25)))
    assert away["first_blocked"][0].tolist() == [-1] and away["first_track"][0].tolist() == [-1] and away["best"][0] == 0


@pytest.mark.parametrize("what, track, changes", [
    ("below min_speed", dict(vel=(0.001, 0.0)), dict(min_speed=0.05)),
    ("above max_object_cells", dict(vel=(-0.01, 0.0), n_cells=65), dict()),
    ("not confirmed", dict(vel=(-0.01, 0.0), status=1), dict())])
def test_a_track_that_does_not_count_is_ignored(what, track, changes):
    base = dict(v=(1.0, 1.0, 1), w=(0.0, 1), dt=0.1, n_poses=40, keep_out=0.3)
    pose = rollout_cases.pose(-10.0, 0.0, 0.0)[None]
    ignored = run(rollout_ref.spec(**dict(base, **changes)), ground(), pose, **one_track((-8.0, 0.0), **track))
    assert ignored["first_track"][0].tolist() == [-1] and ignored["best"][0] == 0, what
    loose = dict(min_speed=0.0, max_object_cells=100, min_status=1)           # the same track counts once the spec lets it
    counted = run(rollout_ref.spec(**dict(base, **loose)), ground(), pose, **one_track((-8.0, 0.0), **track))
    assert counted["first_track"][0].tolist() == [3] and counted["first_blocked"][0, 0] >= 0 and counted["best"][0] == -1, what


def test_a_clear_rollout_that_ends_without_a_route_to_the_goal_is_not_valid():
    """A patch of cost 220 where the fastest straight rollout ends: below blocked_at 253, so the rollout is clear, but impassable for a
    cost-to-go made with blocked_at 200, so its end is UNREACHED.  With a togo weight it is not valid and another is picked; with the
    weight 0 it stays valid and, being the fastest and straight, is the pick."""
    cost = ground()
    cost[0, 20:24, 26:35] = 220                                              # x in [-5, -3), y in [-2, 2.5); the rollout ends at (-4, 0.25)
    togo = towards(cost, 12.0, 0.25, blocked_at=200)
    fast = 3 * 5 + 2
    out = run(rollout_ref.spec(weights=dict(togo=1, sum_cost=0), **PLAN), cost, togo=togo)
    assert out["first_blocked"][0, fast] == -1 and out["max_cost"][0, fast] == 220 and out["end_togo"][0, fast] == UNREACHED
    assert out["flags"][0, fast] == ADMISSIBLE | CLEAR_STATIC | CLEAR and out["info"][0, 3] < out["info"][0, 2] == 20
    assert out["best"][0] not in (-1, fast) and out["end_togo"][0, out["best"][0]] != UNREACHED
    assert (out["end_togo"][0][(out["flags"][0] & VALID) != 0] != UNREACHED).all()
    free = run(rollout_ref.spec(weights=dict(togo=0, sum_cost=0, slow=1), **PLAN), cost, togo=togo)
    assert free["end_togo"][0, fast] == UNREACHED and free["flags"][0, fast] & VALID and free["info"][0, 3] == 20 and free["best"][0] == fast
    none = run(rollout_ref.spec(weights=dict(togo=1, sum_cost=0), **PLAN), cost)          # without a cost-to-go the clause is off as well
    assert none["info"][0, 3] == 20 and (none["end_togo"][0] == UNREACHED).all()


def test_everything_blocked_stops_the_vehicle():
    out = run(rollout_ref.spec(**PLAN), ground([(0, NX, 0, NY)]))
    assert out["best"][0] == -1 and out["score"][0] == 0 and out["info"][0, :5].tolist() == [20, 0, 0, 0, NO_CANDIDATE]
    assert out["command"][0].tobytes() == np.zeros(2).tobytes()               # +0.0 twice, bit for bit


def test_the_dynamic_window_excludes_as_stated():
    s = rollout_ref.spec(accel=(2.0, 4.0), **PLAN)                              # a_v dt = 0.2, a_w dt = 0.4
    vw = rollout_ref.host_tables(s)[0]
    twist = np.array([[1.1, 0.1]])
    cost = ground()
    out = run(s, cost, togo=towards(cost, 12.0, 0.25), twist=twist)
    inside = (np.abs(vw[:, 0] - 1.1) <= 2.0 * 0.1) & (np.abs(vw[:, 1] - 0.1) <= 4.0 * 0.1)
    assert inside.tolist() == [k in (5 + 2, 5 + 3) for k in range(20)]          # v = 1.0 alone; w = -0.4 lies 0.5 away, w = 0 and 0.4 inside
    assert ((out["flags"][0] & ADMISSIBLE) != 0).tolist() == inside.tolist() and out["info"][0, 0] == 2 and out["info"][0, 3] == 2
    assert out["best"][0] == 5 + 2                                            # not the fastest: that one is out of reach
    free = run(s, cost, togo=towards(cost, 12.0, 0.25))
    assert free["info"][0, 0] == 20 and free["best"][0] == 17


def test_a_mirror_symmetric_scene_drives_straight():
    cost = ground([(24, 26, 22, 25), (24, 26, 36, 39)])                       # two blocks, mirror images about the row of cells j = 30
    s = rollout_ref.spec(v=(0.5, 2.0, 4), w=(0.8, 9), dt=0.1, n_poses=60, weights=dict(togo=1, sum_cost=1))
    out = run(s, cost, togo=towards(cost, 12.0, 0.25))
    table = out["scores"][0].reshape(4, 9)
    assert (table == table[:, ::-1]).all() and (out["flags"][0].reshape(4, 9) == out["flags"][0].reshape(4, 9)[:, ::-1]).all()
    assert out["best"][0] % 9 == 4 and out["command"][0, 1] == 0.0
    tied = run(rollout_ref.spec(v=(0.5, 2.0, 4), w=(0.8, 9), dt=0.1, n_poses=60, weights=dict(togo=0, sum_cost=0)), cost)
    assert tied["best"][0] == 3 * 9 + 4                                       # every score 0: the least turn, then the larger speed


def test_a_nan_pose_is_reported_and_stops_the_vehicle():
    pose = rollout_cases.pose(-10.0, 0.25, 0.0)[None]
    pose[0, 2, 1] = np.nan                                                    # an entry the rollouts do not even read
    out = run(rollout_ref.spec(**PLAN), ground(), pose)
    assert out["info"][0, 4] == NOT_FINITE and out["info"][0, 3] == 20 and out["best"][0] == -1
    assert out["command"][0].tobytes() == np.zeros(2).tobytes()
    pose[0, 0, 3] = np.inf
    out = run(rollout_ref.spec(**PLAN), ground(), pose)
    assert out["info"][0, 4] == NOT_FINITE | NO_CANDIDATE and (out["first_blocked"][0] == 0).all()


# ---- against the restatements of the neighbouring stages --------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, c in rollout_cases.all_cases().items() if c["spec"]["v"][2] * c["spec"]["w"][1] <= 64])
def test_xy_through_check_paths_and_the_ends_through_nav_ref(name):
    case, want = rollout_cases.all_cases()[name], rollout_cases.want_of(name)
    sc, s = case["scene"], case["spec"]
    static = rollout_ref.plan_rollouts(s, **dict(rollout_cases.arguments(case), tracks=None, pos=None, vel=None))
    assert static["xy"].tobytes() == want["xy"].tobytes() and static["max_cost"].tobytes() == want["max_cost"].tobytes()
    for m in range(sc["M"]):
        K = want["scores"].shape[1]
        got = field_ref.check_paths(want["xy"][m], None, np.full(K, m, np.int32), sc["origin"], sc["cell"], sc["state"], sc["dist2"], sc["cost"],
                                    rollout_cases.R, blocked_at=s["blocked_at"], outside_blocks=s["outside_blocks"])
        assert got["first_blocked"].tolist() == static["first_blocked"][m].tolist(), (name, m)
        assert got["max_cost"].astype(np.int32).tolist() == want["max_cost"][m].tolist(), (name, m)
        assert ((want["flags"][m] & CLEAR_STATIC) != 0).tolist() == (got["first_blocked"] == -1).tolist(), (name, m)
        if case["togo"] is not None:
            cells = nav_ref.window_cells(want["xy"][m][:, -1], sc["origin"][m], sc["cell"], sc["nx"], sc["ny"])
            ends = np.where(cells >= 0, case["togo"][m].reshape(-1)[np.maximum(cells, 0)], UNREACHED)
            assert ends.tolist() == want["end_togo"][m].tolist(), (name, m)
        else:
            assert (want["end_togo"][m] == UNREACHED).all()
