"""The hand-made TrainStep of the CPU control-flow tests: the object without its constructor (no HIP library, no plan, no device
buffers), holding what step() and the capture code read.  The tests replace the pieces that enqueue kernels by stand-ins of their
own; everything between them -- the order of an iteration, the collectives, the bookkeeping -- is the trainer's code."""
import types

import torch

from camradepth_amd.trainer import GradSync, TrainStep


def stub_model():
    from camradepth_amd.model import CamRaDepth
    m = CamRaDepth(input_channels=7, depths=(1, 1, 1, 1))       # parameters live in one flat CPU buffer
    m._ensure_grad_views()
    return m


def stub_trainstep(m, skip=False, clip=None, ema=None, dist_active=False, k=1, world=1, late=False):
    """skip / clip / ema: skip_nonfinite, max_grad_norm, ema_decay.  late: a captured step (use_graph; the test supplies the stand-ins
    for graphs and streams), else an eager one.  dist_active without a process group: the test stands in for the collectives."""
    ts = object.__new__(TrainStep)
    z = lambda: torch.zeros(4)                                    # noqa: E731  (optimizer state the capture saves and restores)
    ts.state = types.SimpleNamespace(                             # the shape-independent half (trainer.TrainState)
        m=z(), v=z(), pg=z(), egn=z(), fac=z(), nsq=z(), hp=torch.zeros(16), hp_ring=[torch.zeros(16) for _ in range(4)],
        gate=torch.zeros(8, dtype=torch.int32) if skip else None,
        max_grad_norm=clip, parts=z() if clip is not None else None, clip=torch.zeros(2) if clip is not None else None,
        ema=z() if ema is not None else None, ema_decay=ema, ema_warmup=True, ema_n=0, ema_base=0, _ema_swapped=False,
        lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, update_interval=k, schedule=None,
        iter_count=0, epoch_iter=0, sched_steps=0, step_count=0, _window_open=False, _window_pos=0)
    ts.model, ts.sync = m, GradSync(m)
    ts.sync.active = ts.dist_active = dist_active
    ts.world, ts.skip_nonfinite = world, skip
    ts.use_graph = ts.late_wgrad = late
    ts.graphs, ts._zero, ts._opt = None, True, True
    ts.acc = torch.zeros(16, dtype=torch.int64)
    ts.plan = types.SimpleNamespace(ensure_packed=lambda: None, packed_version=None, split_late=False, fp8_grad_layers=[], fp8_jit=False,
                                    backward=lambda tags=None: None, run_late=lambda key: None, pack=lambda lo=None, hi=None: None)
    ts._params, ts._frozen_sig = [], ()
    return ts


def record_pieces(ts, calls):
    """The kernel-enqueuing pieces of `ts` replaced by recorders into `calls`."""
    ts._forward_and_loss_partials = lambda: calls.append("fwd")
    ts._loss_backward = lambda: calls.append("loss_bwd")
    ts.plan.backward = lambda tags=None: calls.append("bwd:" + "+".join(tags))
    ts._capture_flags = lambda window: calls.append("capture:%s" % ("window" if window else "start"))
    ts._norm = lambda key=None: calls.append("norm:%s" % (key,))
    ts._commit = lambda: calls.append("commit")
    ts._optimizer = lambda key=None: calls.append("optimizer:%s" % (key,))


def eager_order(ts):
    """What one eager iteration of `ts` (current _zero / _opt) does, through TrainStep._run: the recorded pieces and, between them,
    the host's collectives as markers -- "loss" (the loss all-reduce), a bucket key (the launch of its gradient all-reduce), "wait"
    (for those), "gate" (the ranks' agreement on skip_nonfinite's verdict)."""
    calls = []
    record_pieces(ts, calls)
    ts._reduce_loss_partials = lambda: calls.append("loss")
    ts.sync.launch, ts.sync.wait = calls.append, lambda: calls.append("wait")
    ts._agree = lambda: calls.append("gate")
    ts._run(ts._iteration(late=False))
    return calls
