"""CPU: skip_nonfinite's control flow without a GPU.  The gated segment order of a TrainStep iteration (flag captures around
the backward, the gated norm, then ONE commit behind the last bucket) appears only with the switch on; and in a gloo world of
two, one rank's local dropped-partial verdict makes BOTH ranks skip (trainer.TrainStep._agree), with the HIP pieces replaced
by stand-ins as in tests/test_ddp_cpu.py."""
import os
import socket
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from camradepth_amd.trainer import GradSync, TrainStep


def _stand_in(m, skip, dist_active, k=1, world=1):
    ts = object.__new__(TrainStep)
    ts.state = types.SimpleNamespace()
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


def test_gated_segment_order_only_with_the_switch():
    m = _model()
    for dist_active in (False, True):
        ts = _stand_in(m, False, dist_active)
        segs = ts._segments()
        assert [a for _, a in segs] == ["loss"] + list(GradSync.ORDER) + [None]
        assert segs[-1][0] == ts._optimizer
        ts = _stand_in(m, True, dist_active)
        segs = ts._segments()
        assert [a for _, a in segs] == ["loss"] + list(GradSync.ORDER) + (["gate"] if dist_active else [None]) + [None]
        assert segs[-1][0] == ts._commit_gated and ts._optimizer not in [f for f, _ in segs]
        ts._opt = False                                  # an accumulating iteration: capture, but no norm and no commit
        segs = ts._segments()
        assert [a for _, a in segs] == ["loss"] + [None] * len(GradSync.ORDER) + [None]
    # the pieces run in this order: capture(backward start) -> backward -> capture(window) -> gated norm -> commit
    ts = _stand_in(m, True, False)
    calls = []
    ts._forward_and_loss_partials = lambda: calls.append("fwd")
    ts._loss_backward = lambda: calls.append("loss_bwd")
    ts.plan.backward = lambda tags=None: calls.append("bwd:" + "+".join(tags))
    ts._capture_flags = lambda window: calls.append("capture:%s" % ("window" if window else "start"))
    ts._norm_gated = lambda key=None: calls.append("norm:%s" % (key,))
    ts._commit_gated = lambda: calls.append("commit")
    for fn, _ in ts._segments():
        fn()
    assert calls == ["fwd", "capture:start", "loss_bwd", "bwd:dec", "bwd:enc3+enc2", "bwd:enc1", "bwd:enc0", "capture:window",
                     "norm:None", "commit"]


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
        m = _model()
        ts = _stand_in(m, True, True, k=2, world=world)
        decisions = []

        def fwd():
            if ts._zero:
                m.flat_grad.zero_()
                ts.gate[:2].zero_()
            ts.acc.zero_()
            ts.acc[1] += 1

        def capture(window):
            if window and rank == 1 and ts.iter_count == 2:      # rank 1 only: a dropped partial in window 2's first backward
                ts.gate[1] = 1

        def commit():
            bad = int(ts.gate[0] | ts.gate[1])
            decisions.append(bad)
            ts.gate[4] = bad
            ts.gate[3 if bad else 2] += 1
        ts._forward_and_loss_partials = fwd
        ts._loss_backward = lambda: None
        ts._capture_flags = capture
        ts._norm_gated = lambda key=None: None
        ts._commit_gated = commit
        ran = [ts.step() for _ in range(6)]
        ok = ran == [False, True] * 3 and decisions == [0, 1, 0]
        ok = ok and ts.gate[2].item() == 2 and ts.gate[3].item() == 1 and not ts.sync.pending
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_one_ranks_dropped_partial_makes_every_rank_skip_world2():
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
    assert sorted(res) == [(0, True), (1, True)]
