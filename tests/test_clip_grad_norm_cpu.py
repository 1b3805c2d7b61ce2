"""CPU: max_grad_norm's control flow without a GPU.  The TrainStep segment order is unchanged without the switch; with it, the norm
pass and ONE commit follow the whole backward (sharing skip_nonfinite's tail when both are on); the refusals come before anything
is built; and in a gloo world of two both ranks take the clipped path in the same order with the collectives of the default step,
no more (the HIP pieces replaced by stand-ins as in tests/test_skip_nonfinite_cpu.py)."""
import os
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from camradepth_amd import lib as L
from camradepth_amd.optim import check_max_grad_norm, diffGradNorm
from camradepth_amd.trainer import GradSync, TrainStep


def _stand_in(m, skip, clip, dist_active, k=1, world=1):
    ts = object.__new__(TrainStep)
    ts.state = types.SimpleNamespace(max_grad_norm=clip)
    ts.model, ts.sync = m, GradSync(m)
    ts.dist_active, ts.world, ts.update_interval, ts.use_graph, ts.graphs = dist_active, world, k, False, None
    ts.schedule, ts.lr, ts.betas, ts.eps, ts.wd = None, 1e-3, (0.9, 0.999), 1e-8, 0.0
    ts.iter_count = ts.epoch_iter = ts.sched_steps = ts.step_count = 0
    ts._window_open, ts._window_pos, ts._zero, ts._opt = False, 0, True, True
    ts.hp, ts.hp_ring, ts.acc = torch.zeros(16), [torch.zeros(16) for _ in range(4)], torch.zeros(16, dtype=torch.int64)
    ts.gate = torch.zeros(8, dtype=torch.int32) if skip else None
    ts.skip_nonfinite = skip
    ts.plan = types.SimpleNamespace(ensure_packed=lambda: None, packed_version=None, split_late=False, backward=lambda tags=None: None)
    ts._params, ts._frozen_sig = [], ()
    return ts


def _model():
    from camradepth_amd.model import CamRaDepth
    m = CamRaDepth(input_channels=7, depths=(1, 1, 1, 1))
    m._ensure_grad_views()
    return m


def _record(ts, calls):
    ts._forward_and_loss_partials = lambda: calls.append("fwd")
    ts._loss_backward = lambda: calls.append("loss_bwd")
    ts.plan.backward = lambda tags=None: calls.append("bwd:" + "+".join(tags))
    ts._capture_flags = lambda window: calls.append("capture:%s" % ("window" if window else "start"))
    ts._norm_gated = lambda key=None: calls.append("norm_gated:%s" % (key,))
    ts._commit_gated = lambda: calls.append("commit_gated")
    ts._norm_clip = lambda key=None: calls.append("norm_clip:%s" % (key,))
    ts._commit_clip = lambda: calls.append("commit_clip")
    ts._optimizer = lambda key=None: calls.append("optimizer:%s" % (key,))


def _order(ts):
    calls = []
    _record(ts, calls)
    for fn, _ in ts._segments():
        fn()
    return calls


BWD = ["bwd:dec", "bwd:enc3+enc2", "bwd:enc1", "bwd:enc0"]


def test_segment_order_without_and_with_the_switch():
    m = _model()
    for dist_active in (False, True):
        ts = _stand_in(m, False, None, dist_active)
        assert [a for _, a in ts._segments()] == ["loss"] + list(GradSync.ORDER) + [None]
        assert ts._segments()[-1][0] == ts._optimizer
        assert _order(ts) == ["fwd", "loss_bwd"] + BWD + ["optimizer:None"]
        ts = _stand_in(m, False, 1.0, dist_active)
        segs = ts._segments()
        assert [a for _, a in segs] == ["loss"] + list(GradSync.ORDER) + [None, None]
        assert segs[-2][0] == ts._norm_clip and segs[-1][0] == ts._commit_clip
        assert ts._optimizer not in [f for f, _ in segs]
        assert _order(ts) == ["fwd", "loss_bwd"] + BWD + ["norm_clip:None", "commit_clip"]
        ts._opt = False                                  # an accumulating iteration: no norm, no commit -- the default segments
        assert [a for _, a in ts._segments()] == ["loss"] + [None] * len(GradSync.ORDER)
        assert _order(ts) == ["fwd", "loss_bwd"] + BWD
        # both switches: skip_nonfinite's tail (flag capture, gated norm, agreement point) runs the clipping pieces
        ts = _stand_in(m, True, float("inf"), dist_active)
        segs = ts._segments()
        assert [a for _, a in segs] == ["loss"] + list(GradSync.ORDER) + (["gate"] if dist_active else [None]) + [None]
        assert segs[-1][0] == ts._commit_clip
        assert _order(ts) == ["fwd", "capture:start", "loss_bwd"] + BWD + ["capture:window", "norm_clip:None", "commit_clip"]
        # skip_nonfinite alone is unchanged
        ts = _stand_in(m, True, None, dist_active)
        assert _order(ts) == ["fwd", "capture:start", "loss_bwd"] + BWD + ["capture:window", "norm_gated:None", "commit_gated"]


def test_max_grad_norm_values_are_checked():
    assert check_max_grad_norm(None, "x") is None
    assert check_max_grad_norm(2, "x") == 2.0 and check_max_grad_norm(float("inf"), "x") == float("inf")
    for bad in (0, 0.0, -1.0, float("nan"), float("-inf"), "a"):
        with pytest.raises(L.CrdError, match="max_grad_norm"):
            check_max_grad_norm(bad, "x")


def test_optimizer_refuses_before_anything_is_built():
    ps = [torch.nn.Parameter(torch.randn(5)) for _ in range(3)]
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(L.CrdError, match="max_grad_norm"):
            diffGradNorm(ps, max_grad_norm=bad)
    with pytest.raises(L.CrdError, match="one param group"):
        diffGradNorm([{"params": ps[:1]}, {"params": ps[1:]}], max_grad_norm=1.0)
    diffGradNorm([{"params": ps[:1]}, {"params": ps[1:]}])          # several groups without clipping: as before
    opt = diffGradNorm(ps[:1], max_grad_norm=1.0)
    assert opt.max_grad_norm == 1.0 and opt.grad_norm is None
    assert "max_grad_norm" not in opt.param_groups[0]              # an attribute: state_dicts interchange with the reference's
    opt.add_param_group({"params": ps[1:]})
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(L.CrdError, match="one param group"):       # (before the flat layout and any launch: CPU tensors here)
        opt.step()
    assert opt._groups is None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import camradepth_amd.trainer as T
        m = _model()
        res = {}
        for clip in (None, 0.5):
            ts = _stand_in(m, False, clip, True, k=2, world=world)
            calls, colls = [], []
            _record(ts, calls)
            real = dist.all_reduce

            def counted(t, *a, **kw):
                colls.append(tuple(t.shape))
                return real(t, *a, **kw)
            ts._forward_and_loss_partials = lambda: (calls.append("fwd"), ts.acc.zero_(), ts.acc.__setitem__(1, 1))
            T.dist.all_reduce = counted
            try:
                ran = [ts.step() for _ in range(4)]
            finally:
                T.dist.all_reduce = real
            res[clip] = (ran, calls, colls)
        ran0, calls0, colls0 = res[None]
        ran1, calls1, colls1 = res[0.5]
        tail = ["norm_clip:None", "commit_clip"]
        ok = ran0 == ran1 == [False, True, False, True] and colls1 == colls0 and not ts.sync.pending
        ok = ok and [c for c in calls1 if not c.startswith(("norm_clip", "commit_clip"))] == \
            [c for c in calls0 if not c.startswith("optimizer")]
        ok = ok and calls1.count("commit_clip") == 2 and calls1[-2:] == tail and calls1[calls1.index("commit_clip") - 1] == tail[0]
        q.put((rank, bool(ok), calls1))
    finally:
        dist.destroy_process_group()


def test_both_ranks_take_the_clipped_path_with_no_extra_collective_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda r: r[0])
    assert [(r, ok) for r, ok, _ in res] == [(0, True), (1, True)]
    assert res[0][2] == res[1][2]                        # the same pieces in the same order on both ranks
