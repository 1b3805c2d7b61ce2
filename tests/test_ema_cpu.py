"""CPU: ema_decay's control flow and host arithmetic without a GPU.  The values are checked before anything is built; the host's
(d_n, w_n) is the kernels' fp32 expression; the new entry points are declared and bound; the TrainStep records the same segments
with the EMA as without (the update kernel carries it: no new segment) and a gloo world of two performs the same collectives
(the HIP pieces replaced by stand-ins as in tests/test_clip_grad_norm_cpu.py).  Also on the CPU: the recurrence on random data
moves by far more than the tolerance the GPU tests derive, so a missing update cannot pass them."""
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from camradepth_amd import lib as L
from camradepth_amd.optim import check_ema_decay, diffGradNorm, ema_weight
from camradepth_amd.trainer import GradSync, TrainStep
from tests.trainstep_stub import eager_order, record_pieces as _record, stub_model as _model, stub_trainstep

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crd_diffgradnorm_norm", "crd_diffgradnorm_commit", "crd_diffgradnorm_step", "crd_swap_f32")


def test_ema_decay_values_are_checked():
    assert check_ema_decay(None, "x") is None
    assert check_ema_decay(0, "x") == 0.0 and check_ema_decay(0.9999, "x") == 0.9999 and check_ema_decay("0.5", "x") == 0.5
    for bad in (1, 1.0, 1.5, -0.1, float("nan"), float("inf"), float("-inf"), "a", [0.5], object(), True):
        with pytest.raises(L.CrdError, match="ema_decay"):
            check_ema_decay(bad, "x")


def test_refusals_come_before_anything_is_built():
    from camradepth_amd.runner import Trainer
    ps = [torch.nn.Parameter(torch.randn(5)) for _ in range(3)]
    for bad in (1.0, -0.5, float("nan"), "a"):
        with pytest.raises(L.CrdError, match="ema_decay"):
            diffGradNorm(ps, ema_decay=bad)
        # a model stand-in that would fail on first use: the value is refused before the step or the runner touches it
        m = types.SimpleNamespace(training=True, flat=types.SimpleNamespace(is_cuda=True))
        with pytest.raises(L.CrdError, match="ema_decay"):
            TrainStep(m, 2, 64, 96, ema_decay=bad)
        with pytest.raises(L.CrdError, match="ema_decay"):
            Trainer(m, ema_decay=bad)
    opt = diffGradNorm([{"params": ps[:1]}, {"params": ps[1:]}], ema_decay=0.99, ema_warmup=False)      # several groups are fine
    assert opt.ema_decay == 0.99 and opt.ema_warmup is False and opt._groups is None
    assert all("ema_decay" not in g and "ema_warmup" not in g for g in opt.param_groups)   # attributes: state_dict() stays the reference's
    assert set(opt.state_dict()["param_groups"][0]) == {"params", "lr", "betas", "eps", "weight_decay"}
    with pytest.raises(L.CrdError, match="without ema_decay"):
        diffGradNorm(ps).ema_state()


@pytest.mark.parametrize("decay", [0.9, 0.9999, 0.5, 0.0, 1.0 / 3.0])
def test_host_weights_are_the_fp32_expression(decay):
    f = np.float32
    for n in range(1, 51):
        for warm in (True, False):
            d_ref = min(f(decay), f(1 + n) / f(10 + n)) if warm else f(decay)
            w_ref = f(1.0) - d_ref
            d, w = ema_weight(decay, warm, n)
            assert isinstance(d, float) and isinstance(w, float)
            assert f(d) == d_ref and d == float(d_ref) and f(w) == w_ref and w == float(w_ref), (decay, n, warm)
    # the warm-up is timm's: (1 + n) / (10 + n) until it reaches the decay
    assert ema_weight(0.9999, True, 1)[0] == float(f(2) / f(11)) and ema_weight(0.5, True, 50)[0] == 0.5
    # what reaches the device as a float32 tensor element is that value exactly
    hp = torch.zeros(16)
    hp[5] = ema_weight(0.9999, True, 7)[1]
    assert hp.numpy()[5] == f(1.0) - f(8) / f(17)


def test_new_symbols_are_declared_and_bound():
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in L._SIGS and name in L.EXPORTS, name
    assert int(re.search(r"#define\s+CRD_ABI_VERSION\s+(\d+)", h).group(1)) == L.ABI_VERSION >= 9
    # the optimizer's entry points take one descriptor and the stream; the EMA is part of the descriptor -- its buffer with the other
    # pointers, then decay, warm-up, and the update number and the base as two separate ints -- and of no signature
    for name in NEW[:3]:
        assert L._SIGS[name] == "pp"
    assert not [n for n in L._SIGS if n.startswith("crd_diffgradnorm_") and n not in NEW]
    body = re.search(r"typedef\s+struct\s+crd_dgn_desc\s*\{(.*?)\}\s*crd_dgn_desc\s*;", h, flags=re.S).group(1)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?=,|$)", decl.strip())]     # the field names, in order
    assert declared == [n for n, _ in L.DgnDesc._fields_]
    assert {"ema", "ema_decay", "ema_warmup", "ema_n", "ema_base", "gate", "clip", "max_norm"} <= set(declared)


# ---------------------------------------------------------------------------------------------- control flow (stand-ins)
def _stand_in(m, skip, clip, ema, dist_active, k=1, world=1):
    return stub_trainstep(m, skip=skip, clip=clip, ema=ema, dist_active=dist_active, k=k, world=world)


def test_segment_order_is_the_same_with_and_without_ema():
    m = _model()
    for dist_active in (False, True):
        for skip, clip in ((False, None), (True, None), (False, 1.0), (True, float("inf"))):
            for opt in (True, False):
                off, on = _stand_in(m, skip, clip, None, dist_active), _stand_in(m, skip, clip, 0.9, dist_active)
                off._opt = on._opt = opt
                names = [[[getattr(f, "__name__", None) or f.func.__name__ for f in piece] for piece in (it.head, *it.tail)]
                         for it in (on._iteration(late=False), off._iteration(late=False))]
                assert names[0] == names[1] and names[0][0] == ["_forward_and_loss_partials"]
                assert eager_order(on) == eager_order(off)             # the pieces and the host's collectives between them
    ts = _stand_in(m, False, None, 0.9, False)
    it = ts._iteration(late=False)
    assert it.tail == ([ts._optimizer], []) and len(it.chain) == len(GradSync.ORDER)


def test_step_uploads_the_weight_and_refuses_inside_the_swap():
    m = _model()
    ts = _stand_in(m, False, None, 0.9, False, k=2)
    calls = []
    _record(ts, calls)
    ran = [ts.step() for _ in range(6)]
    assert ran == [False, True] * 3 and ts.ema_n == 3 and ts.ema_updates == 3          # accumulate-only iterations do not count
    assert ts.hp.numpy()[5] == np.float32(1.0) - np.float32(4) / np.float32(13)         # w_3 with the warm-up (decay 0.9 > 4/13)
    ts._ema_swapped = True
    with pytest.raises(L.CrdError, match="ema_weights"):
        ts.step()
    assert ts.ema_n == 3 and ts.iter_count == 6
    # gated: the device counts; the host uploads decay, base and warm-up for it and does not count itself
    ts = _stand_in(m, True, None, 0.75, False)
    ts.state.ema_base = 5
    _record(ts, calls)
    ts.step()
    assert ts.ema_n == 0 and ts.hp.numpy()[6] == np.float32(0.75)
    assert int(ts.hp.view(torch.int32)[7]) == 5 and int(ts.hp.view(torch.int32)[15]) == 1
    ts.gate[2] = 7
    assert ts.ema_updates == 2
    assert _stand_in(m, False, None, None, False).ema_updates is None


# ---------------------------------------------------------------------------------------------- gloo world of two
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
        for ema in (None, 0.9):
            ts = _stand_in(m, False, None, ema, True, k=2, world=world)
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
            res[ema] = (ran, calls, colls, ts.ema_updates)
        ran0, calls0, colls0, _ = res[None]
        ran1, calls1, colls1, n1 = res[0.9]
        ok = ran0 == ran1 == [False, True, False, True] and colls1 == colls0 and len(colls0) > 0 and calls1 == calls0 and n1 == 2
        q.put((rank, bool(ok), calls1, colls1))
    finally:
        dist.destroy_process_group()


def test_same_collectives_with_ema_world2():
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
    assert [(r, ok) for r, ok, _, _ in res] == [(0, True), (1, True)]
    assert res[0][2:] == res[1][2:]


# ---------------------------------------------------------------------------------------------- the GPU tests' tolerance
def ema_bound(M, ws):
    """|e_dev - e_fp64| per element after the updates with weights ws: one update is two roundings (p - e, then the fma), each at most
    u max(|p|, |e|)-sized (3 u M with the product's share), older error shrinks by d_n = 1 - w_n."""
    u = 2.0 ** -24
    return 3 * u * M * min(len(ws), 1.0 / min(ws))


def test_the_recurrence_moves_far_more_than_the_bound():
    """The setting of the GPU tests (decay 0.9 without warm-up, 12 Adam-sized sign steps of 6e-5 on values of scale 0.05): the fp32
    recurrence (numpy, one rounding per fma emulated through fp64) stays inside the bound and the fp64 EMA moves > 100x the bound."""
    rng = np.random.default_rng(0)
    p = (0.05 * rng.standard_normal(200000)).astype(np.float32)
    e32, e64 = p.copy(), p.astype(np.float64)
    e0 = e64.copy()
    ws = []
    for n in range(1, 13):
        p = (p + np.float32(6e-5) * np.sign(rng.standard_normal(p.size)).astype(np.float32)).astype(np.float32)
        w = np.float32(ema_weight(0.9, False, n)[1])
        ws.append(float(w))
        diff = (p - e32).astype(np.float32)
        e32 = (np.float64(w) * diff.astype(np.float64) + e32.astype(np.float64)).astype(np.float32)   # exact product + one rounding
        e64 = e64 + np.float64(w) * (p.astype(np.float64) - e64)
    M = max(np.abs(p).max(), np.abs(e64).max())
    bound = ema_bound(M, ws)
    assert np.abs(e32 - e64).max() <= bound
    assert np.abs(e64 - e0).max() > 100 * bound
