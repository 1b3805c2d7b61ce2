"""CPU: max_grad_norm's control flow without a GPU.  The TrainStep segment order is unchanged without the switch; with it, the norm
pass and ONE commit follow the whole backward (sharing skip_nonfinite's tail when both are on); the refusals come before anything
is built; and in a gloo world of two both ranks take the clipped path in the same order with the collectives of the default step,
no more (the HIP pieces replaced by stand-ins as in tests/test_skip_nonfinite_cpu.py)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from camradepth_amd import lib as L
from camradepth_amd.optim import check_max_grad_norm, diffGradNorm
from camradepth_amd.trainer import GradSync
from tests.trainstep_stub import eager_order, record_pieces as _record, stub_model as _model, stub_trainstep


def _stand_in(m, skip, clip, dist_active, k=1, world=1):
    return stub_trainstep(m, skip=skip, clip=clip, dist_active=dist_active, k=k, world=world)


BWD = ["bwd:dec", "bwd:enc3+enc2", "bwd:enc1", "bwd:enc0"]


def _pieces(calls):
    return [c for c in calls if isinstance(c, str) and c not in ("loss", "wait", "gate")]


def test_segment_order_without_and_with_the_switch():
    m = _model()
    for dist_active in (False, True):
        # the host's collectives of a distributed run: the loss all-reduce, each bucket's launch, the wait, the agreement point
        def hosts(calls):
            return [c for c in calls if c not in _pieces(calls)]
        closing = ["loss"] + list(GradSync.ORDER) + ["wait"] if dist_active else []
        ts = _stand_in(m, False, None, dist_active)
        calls = eager_order(ts)
        assert hosts(calls) == closing
        assert ts._iteration(late=False).tail == ([ts._optimizer], [])
        assert _pieces(calls) == ["fwd", "loss_bwd"] + BWD + ["optimizer:None"]
        ts = _stand_in(m, False, 1.0, dist_active)
        calls = eager_order(ts)
        assert hosts(calls) == closing
        assert ts._iteration(late=False).tail == ([ts._norm, ts._commit], [])
        assert _pieces(calls) == ["fwd", "loss_bwd"] + BWD + ["norm:None", "commit"] and calls[-2:] == ["norm:None", "commit"]
        ts._opt = False                                  # an accumulating iteration: no norm, no commit -- the default segments
        calls = eager_order(ts)
        assert hosts(calls) == (["loss"] if dist_active else []) and ts._iteration(late=False).tail == ([], [])
        assert _pieces(calls) == ["fwd", "loss_bwd"] + BWD
        # both switches: skip_nonfinite's tail (flag capture, gated norm, agreement point) runs the clipping pieces
        ts = _stand_in(m, True, float("inf"), dist_active)
        calls = eager_order(ts)
        assert hosts(calls) == (closing + ["gate"] if dist_active else [])
        assert calls[-3:] == (["norm:None", "gate", "commit"] if dist_active else ["capture:window", "norm:None", "commit"])
        assert _pieces(calls) == ["fwd", "capture:start", "loss_bwd"] + BWD + ["capture:window", "norm:None", "commit"]
        # skip_nonfinite alone is unchanged
        ts = _stand_in(m, True, None, dist_active)
        assert _pieces(eager_order(ts)) == ["fwd", "capture:start", "loss_bwd"] + BWD + ["capture:window", "norm:None", "commit"]


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
        tail = ["norm:None", "commit"]
        ok = ran0 == ran1 == [False, True, False, True] and colls1 == colls0 and not ts.sync.pending
        ok = ok and [c for c in calls1 if not c.startswith(("norm", "commit"))] == \
            [c for c in calls0 if not c.startswith("optimizer")]
        ok = ok and calls1.count("commit") == 2 and calls1[-2:] == tail and calls1[calls1.index("commit") - 1] == tail[0]
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
