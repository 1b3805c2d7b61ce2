"""CPU: skip_nonfinite's control flow without a GPU.  The gated segment order of a TrainStep iteration (flag captures around
the backward, the gated norm, then ONE commit behind the last bucket) appears only with the switch on; and in a gloo world of
two, one rank's local dropped-partial verdict makes BOTH ranks skip (trainer.TrainStep._agree), with the HIP pieces replaced
by stand-ins as in tests/test_ddp_cpu.py."""
import os
import socket
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from camradepth_amd.trainer import GradSync
from tests.trainstep_stub import eager_order, stub_model as _model, stub_trainstep


def _stand_in(m, skip, dist_active, k=1, world=1):
    return stub_trainstep(m, skip=skip, dist_active=dist_active, k=k, world=world)


BWD = ["bwd:dec", "bwd:enc3+enc2", "bwd:enc1", "bwd:enc0"]


def test_gated_segment_order_only_with_the_switch():
    m = _model()
    for dist_active in (False, True):
        def expect(first, tail, opt=True):               # the host's collectives of a distributed run between the pieces
            if not dist_active:
                return ["fwd"] + first + BWD + [c for c in tail if c != "gate"]
            out = ["fwd", "loss"] + first
            for b, key in zip(BWD, GradSync.ORDER):
                out += [b, key] if opt else [b]
            return out + (["wait"] if opt else []) + tail
        ts = _stand_in(m, False, dist_active)
        assert eager_order(ts) == expect(["loss_bwd"], ["optimizer:None"])
        assert ts._iteration(late=False).tail == ([ts._optimizer], [])
        ts = _stand_in(m, True, dist_active)
        # the pieces run in this order: capture(backward start) -> backward -> capture(window) -> gated norm -> commit
        assert eager_order(ts) == expect(["capture:start", "loss_bwd"], ["capture:window", "norm:None", "gate", "commit"])
        before, after = ts._iteration(late=False).tail
        assert (before + after)[-1] == ts._commit and ts._optimizer not in before + after
        assert after == ([ts._commit] if dist_active else [])           # the ranks agree before a commit of its own
        ts._opt = False                                  # an accumulating iteration: capture, but no norm and no commit
        assert eager_order(ts) == expect(["capture:start", "loss_bwd"], ["capture:window"], opt=False)


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
        ts._norm = lambda key=None: None
        ts._commit = commit
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
