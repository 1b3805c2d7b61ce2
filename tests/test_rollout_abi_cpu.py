"""CPU: the C ABI of the local planner without a GPU.  crd_plan_rollouts is declared, exported and bound with the same argument count;
it refuses every bad argument the header lists before any GPU call, with the documented status and a crd_last_error text that names
the entry and the argument; the workspace formula of the binding equals the header's; the Python interface refuses host tensors, bad
numbers, workspaces of another shape, unknown option names and rollout= without field=, and its host tables are the restatement's."""
import ctypes
import os
import re

import pytest

from tests import rollout_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "crd_plan_rollouts"
ORDER = ("pose", "vw", "arc", "tau", "M", "n_v", "n_w", "P", "origin", "cell", "cost", "togo", "nx", "ny", "blocked_at", "outside_blocks", "tracks",
         "pos", "vel", "T", "min_status", "max_object_cells", "min_speed2", "keep_out2", "twist", "a_v_dt", "a_w_dt", "w_togo", "w_max_cost",
         "w_sum_cost", "w_slow", "w_turn", "workspace", "workspace_bytes", "best", "command", "score", "info", "scores", "first_blocked",
         "first_track", "max_cost", "end_togo", "xy")
BITS = ("cell", "min_speed2", "keep_out2", "a_v_dt", "a_w_dt")
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_the_new_symbol_is_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, h), f"{ENTRY} is not declared"
    assert hasattr(raw, ENTRY), f"{ENTRY} is not exported"
    assert ENTRY in built._SIGS and getattr(L, ENTRY).argtypes is not None, f"{ENTRY} is not bound"
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % ENTRY, h, flags=re.S).group(1)
    assert len(args.split(",")) == len(built._SIGS[ENTRY]) == len(ORDER) + 1 == 45
    assert not [a for a in args.split(",") if "double" in a and "*" not in a]                  # fp64 through memory or as bit patterns
    assert built._SIGS[ENTRY].count("L") == len(BITS) == len([a for a in args.split(",") if "_f64_bits" in a])
    assert L.crd_version() == 13 and built.ABI_VERSION == 13                                   # no struct, no changed signature
    assert re.search(r"#define\s+CRD_ABI_VERSION\s+13\b", h)


def test_plan_rollouts_refuses_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    need = rollout_ref.workspace_bytes(3, 45)
    base = dict(pose=a, vw=a, arc=a, tau=a, M=3, n_v=5, n_w=9, P=64, origin=a, cell=0.5, cost=a, togo=a, nx=40, ny=36, blocked_at=253,
                outside_blocks=1, tracks=a, pos=a, vel=a, T=64, min_status=2, max_object_cells=64, min_speed2=0.01, keep_out2=0.25, twist=a,
                a_v_dt=0.2, a_w_dt=0.4, w_togo=1, w_max_cost=0, w_sum_cost=1, w_slow=0, w_turn=0, workspace=a, workspace_bytes=need, best=a,
                command=a, score=a, info=a, scores=a, first_blocked=a, first_track=a, max_cost=a, end_togo=a, xy=a)
    assert set(base) == set(ORDER)

    def call(**kw):
        v = dict(base, **kw)
        return getattr(L, ENTRY)(*[built.f64_bits(v[k]) if k in BITS else v[k] for k in ORDER], None)

    required = ("pose", "vw", "arc", "tau", "origin", "cost", "workspace", "best", "command", "score", "info", "pos", "vel")
    refusals = [(dict({k: None}), b"null") for k in required]
    refusals += [(dict({k: None}), b"all or none") for k in ("scores", "first_blocked", "first_track", "max_cost", "end_togo")]
    eight = ("pose", "vw", "arc", "tau", "origin", "pos", "vel", "twist", "command", "score", "scores", "xy")
    four = ("togo", "tracks", "best", "info", "first_blocked", "first_track", "max_cost", "end_togo")
    refusals += [(dict({k: a + 4}), k.encode()) for k in eight] + [(dict({k: a + 2}), k.encode()) for k in four]
    refusals += [
        (dict(workspace=a + 8), b"16-byte aligned"), (dict(M=0), b"M 0"), (dict(M=65536), b"M 65536"), (dict(n_v=0), b"n_v 0"), (dict(n_v=65), b"n_v 65"),
        (dict(n_w=0), b"n_w 0"), (dict(n_w=8), b"n_w 8"), (dict(n_w=131), b"n_w 131"), (dict(n_v=64, n_w=65, workspace_bytes=2 ** 40), b"4160 candidates"),
        (dict(P=0), b"P 0"), (dict(P=257), b"P 257"), (dict(nx=0), b"nx 0"), (dict(nx=65536), b"nx 65536"), (dict(ny=0), b"ny 0"),
        (dict(ny=65536), b"ny 65536"), (dict(nx=65535, ny=65535), b"cells"), (dict(blocked_at=0), b"blocked_at 0"), (dict(blocked_at=256), b"blocked_at 256"),
        (dict(outside_blocks=2), b"outside_blocks 2"), (dict(cell=0.0), b"cell"), (dict(cell=-0.5), b"cell"), (dict(cell=INF), b"cell"),
        (dict(cell=NAN), b"cell"), (dict(min_speed2=-1.0), b"min_speed2"), (dict(min_speed2=INF), b"min_speed2"), (dict(min_speed2=NAN), b"min_speed2"),
        (dict(keep_out2=-1.0), b"keep_out2"), (dict(keep_out2=INF), b"keep_out2"), (dict(keep_out2=NAN), b"keep_out2"),
        (dict(a_v_dt=-0.1), b"a_v_dt"), (dict(a_v_dt=NAN), b"a_v_dt"), (dict(a_w_dt=-0.1), b"a_w_dt"), (dict(a_w_dt=NAN), b"a_w_dt"),
        (dict(T=0), b"T 0"), (dict(T=-1), b"T -1"), (dict(T=1025), b"T 1025"), (dict(tracks=None), b"T 64"), (dict(min_status=-1), b"min_status -1"),
        (dict(min_status=3), b"min_status 3"), (dict(max_object_cells=-1), b"max_object_cells -1"),
        (dict(w_togo=-1), b"togo -1"), (dict(w_max_cost=32768), b"max_cost 32768"), (dict(w_sum_cost=-2), b"sum_cost -2"), (dict(w_slow=40000), b"slow 40000"),
        (dict(w_turn=-5), b"turn -5"), (dict(workspace_bytes=need - 1), b"workspace holds"), (dict(workspace_bytes=0), b"workspace holds"),
        (dict(M=4), b"workspace holds"), (dict(n_v=6), b"workspace holds")]
    for kw, word in refusals:
        rc = call(**kw)
        msg = L.crd_last_error()
        assert rc == -1 and ENTRY.encode() in msg and word in msg, (kw, rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, ENTRY)
    # what may be left out is not refused for being NULL: the refusal that comes is the workspace's
    for kw in (dict(togo=None), dict(twist=None, a_v_dt=NAN), dict(tracks=None, pos=None, vel=None, T=0), dict(xy=None),
               dict(scores=None, first_blocked=None, first_track=None, max_cost=None, end_togo=None)):
        assert call(workspace_bytes=0, **kw) == -1 and b"workspace holds" in L.crd_last_error(), kw


def test_the_workspace_formula_equals_the_headers(built):
    from camradepth_amd import rollout
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    assert "workspace_bytes >= 32 * M * K" in h
    for M, K in ((1, 1), (3, 45), (8, 4095), (65535, 4095)):
        assert rollout.workspace_bytes(M, K) == rollout_ref.workspace_bytes(M, K) == 32 * M * K and rollout.workspace_bytes(M, K) % 16 == 0


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import rollout, tracks
    from camradepth_amd.live import ROLLOUT_OPTIONS, LivePipeline
    spec = rollout.RolloutSpec(device="cpu")
    assert set(rollout.SPEC_OPTIONS) == set(rollout_ref.SPEC) and rollout.SPEC_OPTIONS == rollout_ref.SPEC
    assert rollout.SPEC_OPTIONS["min_status"] == tracks.CONFIRMED and rollout.UNREACHED == rollout_ref.UNREACHED
    assert ROLLOUT_OPTIONS == dict({k: v for k, v in rollout.SPEC_OPTIONS.items() if k != "cell"}, tables=False, xy=False)
    assert (rollout.NOT_FINITE, rollout.NO_CANDIDATE) == (1, 2) and (spec.K, spec.n_poses, spec.weights) == (8 * 17, 32, rollout_ref.WEIGHTS)
    for changes in (dict(), dict(v=(0.3, 6.0, 5), w=(2.5, 9), dt=0.05, n_poses=256, track_dt=0.25), dict(v=(1.5, 1.5, 1), w=(0.0, 1), n_poses=1),
                    dict(v=(-1.0, 2.0, 64), w=(3.0, 63), dt=0.3, n_poses=5)):
        s = rollout.RolloutSpec(device="cpu", **changes)
        vw, arc, tau = rollout_ref.host_tables(rollout_ref.spec(**changes))
        assert s.vw.dtype == s.arc.dtype == s.tau.dtype == torch.float64
        assert s.vw.numpy().tobytes() == vw.tobytes() and s.arc.numpy().tobytes() == arc.tobytes() and s.tau.numpy().tobytes() == tau.tobytes()
        assert tuple(s.arc.shape) == (s.K, s.n_poses, 2)
    s = rollout.RolloutSpec(keep_out=0.3, min_speed=0.1, accel=(2.0, 4.0), dt=0.1, weights=dict(slow=3), device="cpu")
    n = rollout_ref.numbers(rollout_ref.spec(keep_out=0.3, min_speed=0.1, accel=(2.0, 4.0), dt=0.1))
    assert (s.keep_out2, s.min_speed2, s.a_v_dt, s.a_w_dt) == (n["keep_out2"], n["min_speed2"], n["a_v_dt"], n["a_w_dt"])
    assert s.weights == dict(rollout_ref.WEIGHTS, slow=3)
    for kw, word in ((dict(v=(0.0, 1.0)), "v ="), (dict(v=(0.0, 1.0, 0)), "n_v"), (dict(v=(0.0, 1.0, 65)), "n_v"), (dict(v=(0.0, 1.0, 2.5)), "n_v"),
                     (dict(v=(2.0, 1.0, 3)), "v_min"), (dict(v=(NAN, 1.0, 3)), "v_min"), (dict(v=(0.0, INF, 3)), "v_max"), (dict(v=("x", 1.0, 3)), "v_min"),
                     (dict(w=(1.0,)), "w ="), (dict(w=(1.0, 4)), "n_w"), (dict(w=(1.0, 131)), "n_w"), (dict(w=(1.0, 0)), "n_w"), (dict(w=(-1.0, 3)), "w_max"),
                     (dict(w=(INF, 3)), "w_max"), (dict(v=(0.0, 1.0, 64), w=(1.0, 65)), "candidates"), (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"),
                     (dict(dt=NAN), "dt"), (dict(dt=INF), "dt"), (dict(dt=True), "dt"), (dict(n_poses=0), "n_poses"), (dict(n_poses=257), "n_poses"),
                     (dict(n_poses=1.5), "n_poses"), (dict(track_dt=0.0), "track_dt"), (dict(track_dt=NAN), "track_dt"), (dict(keep_out=-0.1), "keep_out"),
                     (dict(keep_out=1e200), "keep_out"), (dict(keep_out=NAN), "keep_out"), (dict(min_speed=-1.0), "min_speed"), (dict(min_speed=INF), "min_speed"),
                     (dict(max_object_cells=-1), "max_object_cells"), (dict(max_object_cells=2.5), "max_object_cells"), (dict(min_status=0), "min_status"),
                     (dict(min_status=3), "min_status"), (dict(accel=(1.0,)), "accel"), (dict(accel=(-1.0, 1.0)), "accel"), (dict(accel=(1.0, NAN)), "accel"),
                     (dict(accel=5.0), "accel"), (dict(blocked_at=0), "blocked_at"), (dict(blocked_at=256), "blocked_at"), (dict(weights=dict(speed=1)), "weights"),
                     (dict(weights=[1]), "weights"), (dict(weights=dict(togo=-1)), "togo"), (dict(weights=dict(turn=32768)), "turn"),
                     (dict(weights=dict(slow=0.5)), "slow"), (dict(cell=0.0), "cell"), (dict(cell=NAN), "cell")):
        with pytest.raises(built.CrdError, match=word):
            rollout.RolloutSpec(device="cpu", **kw)
    ws = rollout.RolloutWorkspace(spec, 2, tables=True, xy=True)
    assert ws.buf.numel() == rollout_ref.workspace_bytes(2, spec.K)
    assert {k: (tuple(v.shape), v.dtype) for k, v in ws.out.items()} == {
        "best": ((2,), torch.int32), "command": ((2, 2), torch.float64), "score": ((2,), torch.int64), "info": ((2, 8), torch.int32),
        "scores": ((2, 136), torch.int64), "first_blocked": ((2, 136), torch.int32), "first_track": ((2, 136), torch.int32),
        "max_cost": ((2, 136), torch.int32), "end_togo": ((2, 136), torch.int32), "xy": ((2, 136, 32, 2), torch.float64)}
    assert set(rollout.RolloutWorkspace(spec, 2).out) == set(rollout_ref.OUT)
    for bad in (dict(M=0), dict(M=65536), dict(M=1.5), dict(spec=None)):
        with pytest.raises(built.CrdError, match="RolloutWorkspace"):
            rollout.RolloutWorkspace(**dict(dict(spec=spec, M=2), **bad))
    pose = torch.eye(3, 4, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(built.CrdError, match="cuda"):                             # host tensors
        rollout.plan_rollouts(spec, pose, {"cost": torch.zeros(2, 9, 7, dtype=torch.uint8)}, (None, torch.zeros(2, 2, dtype=torch.int64)))
    with pytest.raises(built.CrdError, match="RolloutSpec"):
        rollout.plan_rollouts(None, pose, {}, None)
    with pytest.raises(built.CrdError, match="rollout= needs field="):
        LivePipeline(None, 2, cloud={}, occupancy={}, rollout={})                 # the argument check comes before the model is looked at
    with pytest.raises(built.CrdError, match="rollout="):
        LivePipeline(None, 2, cloud={}, occupancy={}, field={}, rollout=dict(n_posez=4))
    with pytest.raises(built.CrdError, match="rollout="):
        LivePipeline(None, 2, cloud={}, occupancy={}, field={}, rollout=[4])
    with pytest.raises(built.CrdError, match="rollout="):
        LivePipeline(None, 2, cloud={}, occupancy={}, field={}, rollout=dict(cell=0.5))     # the cell is the map's, not an option
