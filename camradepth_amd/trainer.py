"""Training-step driver: the counterpart of `Trainer.train_one_epoch`'s inner iteration
(reference: src/main/runner.py:179-270) for one process per GPU.  TrainStep._iteration states what one iteration runs and in
which order, for the eager and the captured step alike.

Data parallelism replaces nn.DataParallel (runner.py:135-136): batch-sharded replicas, gradients SUM-all-reduced with RCCL in four
buckets that become ready in backward order (decoder, stages 4+3, stage 2, stage 1 + patch embeds), each launched as soon as its
backward segment is enqueued so the transfer overlaps the remaining backward.
"""
import collections
import contextlib
import ctypes as C
import functools
import math
import os

import torch
import torch.distributed as dist

from . import lib as L
from . import trace
from .losses import CRITERIA
from .optim import _CHUNK, check_ema_decay, check_max_grad_norm, dgn_desc, ema_weight

LOSS_W = (1.0, 1.0, 1.0, 0.2, 0.2)   # runner.py:213


def _at(t, offset):
    """Address `offset` bytes into t, None for no tensor."""
    return None if t is None else t.data_ptr() + offset


def depth_criterion_mode(criterion):
    """criterion dict -> (depth mode, BerHu thresh) of the captured step, or CrdError.  The step records the kernels of the depth
    criteria of camradepth_amd.losses that train (smooth-L1, Huber = smooth-L1 with beta 1, L1, RMSE, BerHu) and MaskedFocalLoss for
    the segmentation; MaskedMSELoss is a detached metric, SmoothnessLoss takes an image, and other modules have no kernels here."""
    from . import losses as HL
    if criterion is None:
        return "smooth_l1", None
    if not isinstance(criterion, dict) or set(criterion) != {"depth", "seg"}:
        raise L.CrdError("TrainStep(criterion=...) takes a dict {'depth': <loss>, 'seg': <loss>} of camradepth_amd.losses objects, got "
                         f"{criterion!r}")
    d, sg = criterion["depth"], criterion["seg"]
    if type(sg) is not HL.MaskedFocalLoss:
        raise L.CrdError(f"TrainStep(criterion=...): the seg criterion must be camradepth_amd.losses.MaskedFocalLoss, got {type(sg).__name__}")
    mode = {cls: cls.mode for cls in HL.DepthCriterion.__subclasses__()}.get(type(d))
    if mode is None:
        raise L.CrdError(f"TrainStep(criterion=...): unsupported depth criterion {type(d).__name__}; the captured step supports "
                         "MaskedSmoothL1Loss, MaskedHuberLoss, MaskedL1Loss, MaskedRMSELoss and MaskedBerHuLoss from camradepth_amd.losses")
    thresh = None
    if CRITERIA[mode].two_phase:             # BerHu: c = thresh * max |d|
        try:
            thresh = float(d.thresh)
        except (TypeError, ValueError):
            thresh = float("nan")
        if not (thresh > 0.0 and math.isfinite(thresh)):
            raise L.CrdError(f"TrainStep(criterion=...): MaskedBerHuLoss needs a finite thresh > 0, got {d.thresh!r}")
    return mode, thresh


def one_cycle(total_steps, max_lr, div_factor=2.0, pct_start=0.15, final_div_factor=1e4, base_m=0.85, max_m=0.95):
    """(lr, beta1) schedule of torch OneCycleLR(anneal='cos', cycle_momentum=True) as configured in runner.py:151-152."""
    initial, up_end = max_lr / div_factor, float(pct_start * total_steps) - 1
    min_lr = initial / final_div_factor

    def cos(a, b, pct):
        return b + (a - b) / 2.0 * (math.cos(math.pi * pct) + 1)
    out = []
    for s in range(total_steps):
        if s <= up_end:
            pct = s / up_end if up_end > 0 else 1.0
            out.append((cos(initial, max_lr, pct), cos(max_m, base_m, pct)))
        else:
            pct = (s - up_end) / (total_steps - 1 - up_end)
            out.append((cos(max_lr, min_lr, pct), cos(base_m, max_m, pct)))
    return out


class GradSync:
    """Bucketed gradient all-reduce (SUM) over the flat gradient buffer, RCCL over xGMI."""

    ORDER = (("dec",), ("enc3", "enc2"), ("enc1",), ("enc0",))

    def __init__(self, model, group=None):
        self.model, self.group = model, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # CRD_FORCE_DIST=1: run the collectives even in a group of one (exercises the multi-GPU control flow on one GPU)
        self.active = self.world > 1 or (dist.is_initialized() and os.environ.get("CRD_FORCE_DIST") is not None)
        names, offs = model._names, model._offsets
        total = model.flat.numel()

        def first(prefix):
            return offs[next(i for i, n in enumerate(names) if n.startswith(prefix))]
        b2, b3, dec = first("dest_encoder.block2."), first("dest_encoder.block3."), first("from_encoder_1.")
        # flat layout: [patch embeds | block1 | block2 | block3 | block4 | decoder, heads, seg]
        self.ranges = {("dec",): (dec, total), ("enc3", "enc2"): (b3, dec), ("enc1",): (b2, b3), ("enc0",): (0, b2)}
        self.pending = []

    def bucket(self, key):
        lo, hi = self.ranges[key]
        return self.model.flat_grad[lo:hi]

    def launch(self, key):
        if self.active:
            self.pending.append(dist.all_reduce(self.bucket(key), op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def wait(self):
        for w in self.pending:
            w.wait()
        self.pending = []

    def after_backward(self):
        """Eager-autograd path (model._grad_sync): reduce everything once the whole backward is enqueued."""
        for key in self.ORDER:
            self.launch(key)
        self.wait()


# An iteration (TrainStep._iteration), described or captured.  FROZEN: bench.py, tools/exp_defer_dec.py and tools/exp_cumask.py read
# ts.graphs[(zero, opt)][0][0] as the 4-tuple ("late", head graph | None, chain, _) and every chain entry as the 4-tuple (main graph,
# late graph, key, slice graph | None) -- hence these field orders, the one-pair list around the Iteration, and no fifth field: whether
# a bucket's all-reduce follows is the same for all of them (a closing iteration of a multi-GPU run) and TrainStep._run derives it.
# They also read ts.tail_probe, late_stream, late_stream_factory, late_wgrad, sync, dist_active, plan, _forward_and_loss_partials and
# _loss_backward; tests/test_gpu_dropout.py reads set(ts.graphs).
Iteration = collections.namedtuple("Iteration", "kind head chain tail")
Bucket = collections.namedtuple("Bucket", "main late key slice")


class _Piece(list):
    """Calls that enqueue kernels back to back on one stream.  An eager iteration replays them as they are, a captured one replays
    the graph made from them."""

    def replay(self):
        for fn in self:
            fn()


class TrainState:
    """What a training run carries from one iteration to the next, independent of the batch shape: diffGradNorm's state over the
    flat parameter buffer (exp_avg, exp_avg_sq, previous_grad, exp_grad_norm: diffGradNorm.py:62-71), the per-tensor block tables
    of the multi-tensor optimizer launch, the hyper-parameter upload ring, the (lr, beta1) schedule with its position, the
    optimizer step count of the bias corrections and the open accumulation window.  A TrainStep is the shape-specific half
    (plan, static input buffers, captured graphs); the reference's DataLoader has no drop_last (src/data/dataloader.py:40), so
    the last batch of an epoch is smaller and a second TrainStep for that shape must continue THIS state, not restart it."""

    def __init__(self, model, lr, betas, eps, weight_decay, update_interval, schedule, max_grad_norm=None, ema_decay=None,
                 ema_warmup=True):
        dev = model.flat.device
        n = model.flat.numel()
        self.m, self.v, self.pg = (torch.zeros(n, device=dev) for _ in range(3))
        nt = len(model._names)
        self.egn, self.fac = (torch.zeros(nt, device=dev) for _ in range(2))
        seg, b2s, b2c = [], [], []
        for t, (name, o) in enumerate(zip(model._names, model._offsets)):
            numel = model._param(name).numel()
            seg.append([o, o + numel])
            for c in range((numel + _CHUNK - 1) // _CHUNK):
                b2s.append(t)
                b2c.append(c)
        self.seg_host, self.b2s_host = seg, b2s
        self.seg = torch.tensor(seg, dtype=torch.int64, device=dev)
        self.b2s = torch.tensor(b2s, dtype=torch.int32, device=dev)
        self.b2c = torch.tensor(b2c, dtype=torch.int32, device=dev)
        self.nt, self.nblk = nt, len(b2s)
        self.nsq = torch.zeros(self.nblk, device=dev)        # per-workgroup parts of ||g||^2 (summed in a fixed order)
        # hyper-parameters of the next optimizer step: [0..4] read by every optimizer kernel, [8..14] by the gated one only (fp64 lr,
        # beta1, beta2 and the host's step number: include/camradepth_hip.h, crd_dgn_desc)
        self.hp = torch.zeros(16, device=dev)
        self.hp_ring = [torch.zeros(16).pin_memory() for _ in range(64)]
        self.gate = None             # skip_nonfinite: int32[8] verdict words and step counters on the device (TrainStep._gate)
        # max_grad_norm: the norm pass's 4 rows of per-workgroup parts and [total, coef] of the last closed window
        # (include/camradepth_hip.h, crd_dgn_desc: parts, clip)
        self.max_grad_norm = max_grad_norm
        self.parts = torch.zeros(4 * self.nblk, device=dev) if max_grad_norm is not None else None
        self.clip = torch.zeros(2, device=dev) if max_grad_norm is not None else None
        # ema_decay: the exponential moving average of the parameters (layout of model.flat, seeded with them), updated by the optimizer's
        # update kernel on every committed step.  ema_n: the updates so far as the host counts them; with skip_nonfinite the device
        # counts (gate[2] - ema_base: TrainStep.ema_updates).  _ema_swapped: inside TrainStep.ema_weights()
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema = model.flat.detach().clone() if ema_decay is not None else None
        self.ema_n, self.ema_base, self._ema_swapped = 0, 0, False
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.update_interval = update_interval
        self.schedule = schedule
        self.iter_count = 0          # iterations (micro-batches) seen
        self.epoch_iter = 0          # ... in the current epoch (scheduler lag, runner.py:269)
        self.sched_steps = 0         # scheduler.step() calls so far = index into `schedule`
        self.step_count = 0          # optimizer steps taken (skip_nonfinite: attempted; the device counts the committed ones)
        self._window_open, self._window_pos = False, 0


_STATE_FIELDS = ("m", "v", "pg", "egn", "fac", "seg", "b2s", "b2c", "nt", "nblk", "nsq", "hp", "hp_ring", "lr", "betas", "eps", "wd",
                 "update_interval", "schedule", "iter_count", "epoch_iter", "sched_steps", "step_count", "_window_open", "_window_pos", "gate",
                 "max_grad_norm", "parts", "clip", "ema", "ema_decay", "ema_warmup", "ema_n", "ema_base", "_ema_swapped")


class TrainStep:
    """One training ITERATION per step() call (runner.py:179-270).  With update_interval = k the gradients of k
    iterations accumulate in the flat gradient buffer (zeroed on the first, runner.py:175,266), the gradient all-reduce
    and diffGradNorm run on the k-th (runner.py:222,264), each loss is divided by k (runner.py:218).  The schedule
    entry used by an optimizer step follows the reference's scheduler lag: `scheduler.step()` is only called from the
    (k+1)-th iteration of an epoch on (runner.py:269-270); start_epoch() marks the epoch boundary.  Parameters with
    requires_grad=False are frozen: no weight-gradient launch is recorded for them and the optimizer skips them
    (diffGradNorm.py:54-55).

    criterion: {"depth": <loss>, "seg": MaskedFocalLoss()} of camradepth_amd.losses (runner.py:149; None = smooth-L1 + focal).  The
    three depth levels record the chosen criterion's kernels; losses() reports its values.  BerHu's c is a function of the max |d|
    over the GATHERED batch: the ranks reduce their maxima (MAX) at the loss point, with the sums, before any gradient is formed.

    skip_nonfinite=True: GradScaler.step's guard (runner.py:264).  An accumulation window whose gradients hold a NaN / inf element,
    or whose backward dropped a non-finite partial from a fixed-point sum, commits nothing: parameters and optimizer state stay
    as they were, the schedule advances, training goes on.  The decision is taken on the device, after the whole backward, so
    the optimizer of every bucket runs behind the last one (nothing is committed early); found_inf / skipped_steps read it.

    max_grad_norm=c: torch.nn.utils.clip_grad_norm_(params, c) between the backward and diffGradNorm, once per accumulation window
    (after the SUM all-reduce): every gradient is scaled by min(1, c / (||g|| + 1e-6)), ||g|| over the trainable tensors, before
    the weight decay is added.  The scaling happens on the fly (the flat gradient buffer keeps the unclipped values).  The global
    norm needs every bucket, so -- as with skip_nonfinite, and sharing its tail when both are on -- the buckets' late-stream
    slices only write norm parts and the commit of all of them follows the last one.  grad_norm: the window's ||g||, on the
    device; float('inf') computes it without clipping (the bits of the default step).

    ema_decay=d (0 <= d < 1): an exponential moving average of the weights, the set one evaluates and checkpoints (timm ModelEmaV2/V3,
    torch.optim.swa_utils.AveragedModel).  `ema` is a flat fp32 buffer laid out as model.flat and seeded with the parameters; every
    COMMITTED optimizer step n = 1, 2, ... does e <- e + w_n (p_new - e) in fp32 (one fma), w_n = 1 - d_n, d_n = min(d, (1 + n) / (10 + n))
    with ema_warmup (timm's rule: without it d = 0.9999 averages nothing useful for the first 10^4 steps), else d.  The update
    kernel does it where it stores the new parameter: no launch, no pass of its own, no collective (the EMA is a function of the
    all-reduced parameters), and the training itself keeps its bits.  Frozen tensors, accumulate-only iterations and windows
    skipped by skip_nonfinite leave it untouched.  ema_state_dict() / ema_updates read it; `with ts.ema_weights():` makes it the
    model's weights for evaluation.  model.load_state_dict() alone does not touch the EMA (checkpoint.load_checkpoint restores or
    re-seeds it; reseed_ema() by hand)."""

    def __init__(self, model, B, H, W, lr=6e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, update_interval=1,
                 use_graph=True, schedule=None, group=None, state=None, skip_nonfinite=False, criterion=None, max_grad_norm=None,
                 ema_decay=None, ema_warmup=True):
        """state: the TrainState of another TrainStep of the same model (another batch shape of the same run) to continue;
        lr / betas / eps / weight_decay / update_interval / schedule / max_grad_norm / ema_decay / ema_warmup are then taken from it."""
        assert model.training, "TrainStep drives the training path: call model.train() first"
        self._depth_mode, self._berhu_thresh = depth_criterion_mode(criterion)      # refused here, before anything is allocated
        assert update_interval >= 1
        if skip_nonfinite and getattr(model, "fp8_grad", False):
            # delayed fp8 scaling records each backward's amax for the next one: a skipped window would leave a NaN amax behind
            raise L.CrdError("TrainStep(skip_nonfinite=True) does not support fp8 data gradients (model.fp8_grad): a skipped step "
                             "would poison the delayed scales")
        self.skip_nonfinite = bool(skip_nonfinite)
        max_grad_norm = check_max_grad_norm(max_grad_norm, "TrainStep")
        ema_decay = check_ema_decay(ema_decay, "TrainStep")
        if state is not None and state.m.numel() != model.flat.numel():
            raise L.CrdError("TrainStep(state=...): the state belongs to a model with a different parameter count")
        self.state = state if state is not None else TrainState(model, lr, betas, eps, weight_decay, update_interval, schedule,
                                                                max_grad_norm, ema_decay, ema_warmup)
        self.model, self.B, self.H, self.W = model, B, H, W
        self.dev = model.flat.device
        self.lib = L.load()
        x = torch.zeros((B, model.cfg.input_channels, H, W), device=self.dev)
        self.sync = GradSync(model, group)
        self.world = self.sync.world
        self.dist_active = self.sync.active
        model.rng_rank = dist.get_rank(group) if dist.is_initialized() else 0
        # a captured step always uses the late stream (_iteration), an eager step never: there the decoder's streaming weight-gradient
        # kernels run with fewer workgroups (the plan sizes their partial-copy buffers accordingly)
        from .engine import W3_LATE_WGS
        self.late_wgrad = bool(use_graph)
        model.w3_total_wgs = W3_LATE_WGS if self.late_wgrad else None
        model.__dict__["_need_grad"] = True
        self.plan = model._plan_for(x)
        model._ensure_grad_views()
        self.sup = model.cfg.supervised_seg
        self.gt = {"full": torch.zeros((B, 1, H, W), device=self.dev), "half": torch.zeros((B, 1, H // 2, W // 2), device=self.dev),
                   "quarter": torch.zeros((B, 1, H // 4, W // 4), device=self.dev),
                   "seg": torch.zeros((B, H, W), dtype=torch.int64, device=self.dev)}
        self.acc = torch.zeros(16, dtype=L.SUM_DTYPE, device=self.dev)     # crd_sum_t: 4 x (sum, count, sum sq, -) for full/half/quarter/ce (ce: sum, count, #labels out of range, -)
        if CRITERIA[self._depth_mode].two_phase:
            self.maxbits = torch.zeros(4, dtype=torch.int32, device=self.dev)     # per level: fp32 bits of max |d| (MAX-reduced)
            self.berhu_acc = torch.zeros(8, dtype=L.SUM_DTYPE, device=self.dev)   # per level: (sum part1, sum part2 numerators)
        seg, b2s, nt = self.state.seg_host, self.state.b2s_host, self.state.nt
        trainable = torch.tensor([1 if model._param(n_).requires_grad else 0 for n_ in model._names], dtype=torch.uint8)
        self.frozen_names = [n_ for n_ in model._names if not model._param(n_).requires_grad]
        self._params = [model._param(n_) for n_ in model._names]
        self._frozen_sig = tuple(p.requires_grad for p in self._params)      # fixed at construction: the plan records no weight
                                                                             # gradients for frozen tensors (checked in step())
        self.trainable_mask = trainable.to(self.dev) if self.frozen_names else None
        # per gradient bucket: its tensors' slice of the block tables and an `active` mask (the optimizer of a bucket can run
        # as soon as that bucket's gradients are final -- on the late stream, behind their un-packing)
        self.opt_parts = {}
        for key, (lo, hi) in self.sync.ranges.items():
            ts_ = [t for t, (a, _) in enumerate(seg) if lo <= a < hi]
            blks = [i for i, t in enumerate(b2s) if lo <= seg[t][0] < hi]
            assert ts_ == list(range(ts_[0], ts_[-1] + 1)) and blks == list(range(blks[0], blks[-1] + 1))
            mask = torch.zeros(nt, dtype=torch.uint8)
            mask[ts_[0]:ts_[-1] + 1] = 1
            self.opt_parts[key] = (blks[0], len(blks), (mask & trainable).to(self.dev))
        self.use_graph = use_graph
        self.graphs = None
        self._zero, self._opt = True, True
        if self.skip_nonfinite and self.state.gate is None:
            self.state.gate = torch.zeros(8, dtype=torch.int32, device=self.dev)
            self.state.gate[2] = self.state.step_count          # committed steps so far (a continued TrainState)
            if self.state.ema is not None:
                self.state.ema_base = self.state.step_count - self.state.ema_n

    # ------------------------------------------------------------------ skip_nonfinite: what the device decided (one sync per read)
    @property
    def found_inf(self):
        """True if the last closed accumulation window was skipped."""
        return bool(self.gate is not None and int(self.gate[4]) != 0)

    @property
    def skipped_steps(self):
        return 0 if self.gate is None else int(self.gate[3])

    @property
    def committed_steps(self):
        """Optimizer steps that changed the parameters: the bias-correction count, and the per-parameter `step` of a checkpoint."""
        return self.step_count if self.gate is None else int(self.gate[2])

    @property
    def grad_norm(self):
        """max_grad_norm: ||g|| of the last closed accumulation window before clipping (clip_grad_norm_'s return value), a 0-d fp32
        device tensor taken in stream order (no sync); None without max_grad_norm."""
        return None if self.clip is None else self.clip[0].clone()

    # ------------------------------------------------------------------ ema_decay: the averaged weights
    @property
    def ema_updates(self):
        """EMA updates since it was created or restored = the optimizer steps committed since then (skip_nonfinite: read from the
        device, one sync, as committed_steps); None without ema_decay."""
        if self.ema is None:
            return None
        return self.ema_n if self.gate is None else int(self.gate[2]) - self.ema_base

    def ema_state_dict(self):
        """name -> view of the EMA buffer, with model.state_dict()'s keys and shapes (inside ema_weights() the buffers are
        exchanged: this is then the raw weights' dict)."""
        if self.ema is None:
            raise L.CrdError("TrainStep.ema_state_dict(): the step was built without ema_decay")
        return {name: self.ema[a:b].view(self.model._param(name).shape) for name, (a, b) in zip(self.model._names, self.state.seg_host)}

    def reseed_ema(self, updates=0):
        """EMA <- the current parameters, with `updates` as the count the warm-up continues from (a restart from weights alone)."""
        if self.ema is None:
            raise L.CrdError("TrainStep.reseed_ema(): the step was built without ema_decay")
        self.ema.copy_(self.model.flat.detach())
        self._set_ema_updates(updates)

    def _set_ema_updates(self, n):
        self.ema_n = int(n)
        self.ema_base = self.committed_steps - self.ema_n

    def _swap_ema(self):
        L.check(self.lib.crd_swap_f32(self.model.flat.data_ptr(), self.ema.data_ptr(), self.ema.numel(), L.stream()), "crd_swap_f32")
        self.model.mark_params_changed()       # TrainStep / InferenceGraph re-pack (and re-quantise fp8 weights) before their next replay

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model's parameters ARE the averaged weights (and `ema` holds the raw ones): model.forward,
        InferenceGraph, state_dict() and save_checkpoint see them.  An in-place exchange of the two flat buffers (crd_swap_f32, no
        temporary) and back on exit, so the raw bits are restored exactly.  step() refuses to run inside; not re-entrant."""
        if self.ema is None:
            raise L.CrdError("TrainStep.ema_weights(): the step was built without ema_decay")
        if self._ema_swapped:
            raise L.CrdError("TrainStep.ema_weights() is not re-entrant: the averaged weights are already in place")
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._ema_swapped = False

    def optimizer_state(self):
        """diffGradNorm's state in the reference's per-parameter form (diffGradNorm.py:63-71), with `step` = committed steps: what
        the reference's optimizer.state_dict() holds (runner.py:369).  Tensors are views of the device buffers."""
        step = self.committed_steps
        out = {}
        for t, (name, (a, b)) in enumerate(zip(self.model._names, self.state.seg_host)):
            shape = self.model._param(name).shape
            out[name] = {"step": step, "exp_avg": self.m[a:b].view(shape), "exp_avg_sq": self.v[a:b].view(shape),
                         "previous_grad": self.pg[a:b].view(shape), "exp_grad_norm": self.egn[t]}
        return out

    def start_epoch(self):
        """Epoch boundary of the reference loop: the batch index restarts (scheduler lag) and pending accumulated
        gradients were flushed by step(last_of_epoch=True)."""
        self.epoch_iter = 0

    # ------------------------------------------------------------------ pieces of one step
    # (class defaults of what is optional: the CPU control-flow tests build the object by hand, tests/trainstep_stub.py)
    _depth_mode, _berhu_thresh, skip_nonfinite = "smooth_l1", None, False
    maxbits = berhu_acc = None     # BerHu's per-level buffers: no other criterion has them
    grad_hook = None               # tests: called with each bucket's key where that bucket's gradients have become final
    tail_probe = None              # bench.py: a list to collect the main stream's (start, end) events of its wait for the late stream
    late_stream_factory = None     # tools: what makes the late stream instead of torch.cuda.Stream

    def _depth_fwd(self, pred, tgt, i):
        """Level i's loss partials into acc[4i:4i+3] = (sum, count, sum d^2) -- BerHu: (-, count, sum d^2) and maxbits[i]."""
        CRITERIA[self._depth_mode].partials(self.lib, (pred.data_ptr(), tgt.data_ptr(), pred.numel()), self.acc.data_ptr() + 32 * i,
                                            _at(self.maxbits, 4 * i))

    def _depth_bwd(self, pred, tgt, d, i, gmul):
        """Level i's gradient (BerHu: the loss sums of phase b come with it into berhu_acc[2i:2i+2]: losses() reads them)."""
        CRITERIA[self._depth_mode].grad(self.lib, (pred.data_ptr(), tgt.data_ptr(), pred.numel()), self.acc.data_ptr() + 32 * i,
                                        _at(self.maxbits, 4 * i), self._berhu_thresh, _at(self.berhu_acc, 16 * i), None, gmul,
                                        d.data_ptr())

    def _reduce_loss_partials(self):
        """The loss point of a multi-GPU step (between the forward and the backward): the global sums and counts -- and BerHu's
        global max |d| per level, which its c and therefore every gradient depend on."""
        dist.all_reduce(self.acc, group=self.sync.group)
        if self.maxbits is not None:
            dist.all_reduce(self.maxbits, op=dist.ReduceOp.MAX, group=self.sync.group)

    def _forward_and_loss_partials(self):
        p, st = self.plan, L.stream
        if self._zero:
            self.model.flat_grad.zero_()
            if self.skip_nonfinite:
                self.gate[:2].zero_()          # a new window: no verdict yet
        self.acc.zero_()
        if self.maxbits is not None:
            self.maxbits.zero_()
            self.berhu_acc.zero_()
        p.forward(pack=False)                  # step() keeps the packed weights current (ensure_packed / _optimizer)
        for i, (j, key) in enumerate(((5, "full"), (4, "half"), (3, "quarter"))):
            self._depth_fwd(p.out_depth[j].t, self.gt[key], i)
        if self.sup:
            L.check(self.lib.crd_ce_fwd(p.seg_out.data_ptr(), self.gt["seg"].data_ptr(), self.B, self.model.cfg.num_classes,
                                        self.H * self.W, self.acc.data_ptr() + 96, st()), "crd_ce_fwd")

    def _loss_backward(self):
        p, st = self.plan, L.stream
        scale = 1.0 / sum(LOSS_W) / self.update_interval
        for i, (j, key) in enumerate(((5, "full"), (4, "half"), (3, "quarter"))):
            self._depth_bwd(p.out_depth[j].t, self.gt[key], p.out_depth[("grad", j)].t, i, LOSS_W[i] * scale)
        if self.sup:
            L.check(self.lib.crd_ce_focal_bwd(p.seg_out.data_ptr(), self.gt["seg"].data_ptr(), self.B, self.model.cfg.num_classes,
                                              self.H * self.W, self.acc.data_ptr() + 96, None, LOSS_W[3] * scale,
                                              p.seg_grad_in.data_ptr(), st()), "crd_ce_focal_bwd")

    def _dgn(self, key=None):
        """crd_dgn_desc of one optimizer call (by reference, for the library).  key: only the tensors of that gradient bucket (its slice
        of the norm parts and block tables + its `active` mask; the per-tensor buffers stay whole).  With the verdict words under
        skip_nonfinite and the clipping buffers under max_grad_norm.  Always under hp: the scalar hyper-parameters stay 0, the kernels
        read w_n / decay / base / warm-up of the EMA from it."""
        m = self.model
        b0, nb, mask = (0, self.nblk, self.trainable_mask) if key is None else self.opt_parts[key]
        gated, clipped, ema = self.skip_nonfinite, self.max_grad_norm is not None, self.ema
        return C.byref(dgn_desc(
            p=m.flat, g=m.flat_grad, exp_avg=self.m, exp_avg_sq=self.v, prev_grad=self.pg, exp_grad_norm=self.egn, factor=self.fac,
            parts=(self.parts if clipped else self.nsq).data_ptr() + 4 * b0, parts_stride=self.nblk if clipped else 0, seg_off=self.seg,
            blk2seg=self.b2s.data_ptr() + 4 * b0, blk2chunk=self.b2c.data_ptr() + 4 * b0, n_tensors=self.nt, n_blocks=nb, active=mask,
            hp_dev=self.hp, gate=self.gate if gated else None, clip=self.clip if clipped else None,
            max_norm=self.max_grad_norm if clipped else 0.0, ema=ema, ema_decay=self.ema_decay if ema is not None else 0.0,
            ema_warmup=int(self.ema_warmup) if ema is not None else 0, ema_base=self.ema_base if ema is not None and gated else 0))

    def _optimizer(self, key=None):
        """The default step's whole optimizer.  key: only the tensors of that gradient bucket (block-table slice + `active` mask)."""
        L.check(self.lib.crd_diffgradnorm_step(self._dgn(key), L.stream()), "crd_diffgradnorm_step")
        # the bucket's new weights in the kernels' bf16 layouts, right behind its update (late stream: under the encoder's
        # backward) instead of one 169-us launch at the head of the next forward
        lo, hi = (None, None) if key is None else self.sync.ranges[key]
        self.plan.pack(lo, hi)

    def _capture_flags(self, window):
        """skip_nonfinite: the flag captures around the backward."""
        L.check(self.lib.crd_nonfinite_capture(self.gate.data_ptr() + 4 if window else None, L.stream()), "crd_nonfinite_capture")

    @property
    def _deferred(self):
        """The optimizer step waits for a global decision -- skip_nonfinite's verdict, max_grad_norm's norm: a norm pass (per bucket
        or all) and one commit behind the last bucket, instead of the default step's buckets that update as soon as their gradients
        are final."""
        return self.skip_nonfinite or self.max_grad_norm is not None

    def _norm(self, key=None):
        """The deferred step's norm pass: finiteness test included under skip_nonfinite, the parts of the global norm written under
        max_grad_norm."""
        L.check(self.lib.crd_diffgradnorm_norm(self._dgn(key), L.stream()), "crd_diffgradnorm_norm")

    def _commit(self):
        """max_grad_norm: total + coefficient; then every tensor's scalar and update, or -- skip_nonfinite -- none of them; then the
        re-pack of all weights (of unchanged ones after a skip: the packed forms are a function of the fp32 parameters, so re-packing
        them writes the same bits)."""
        L.check(self.lib.crd_diffgradnorm_commit(self._dgn(), L.stream()), "crd_diffgradnorm_commit")
        self.plan.pack()

    def _iteration(self, late):
        """THE order of one iteration, for the current (self._zero, self._opt): zero the gradients first / all-reduce and run the
        optimizer last.  Every piece is a _Piece: calls that enqueue kernels back to back on one stream.

        One step = zero grads -> forward -> masked losses -> backward -> (gradient all-reduce) -> diffGradNorm, entirely as HIP
        kernels with static buffers, so the step is captured once into HIP graphs and replayed; the host only updates the
        hyper-parameter floats per step (OneCycleLR drives lr and beta1 every iteration, runner.py:151-152,270).

        head   forward + loss partials.  Multi-GPU: the loss all-reduce follows (_reduce_loss_partials), which makes the masked-mean
               denominators global and so reproduces the reference's loss over the gathered batch exactly.
        chain  one Bucket per entry of GradSync.ORDER, the gradient buckets in the order the backward finishes them:
               main   on the first bucket skip_nonfinite's flag capture (what the forward's loss sums dropped is not the window's
                      business) and the loss backward; then the bucket's backward segment.
               late   (late=True: a captured step) the segment's weight gradients, which nothing in the backward waits for, on a
                      second stream next to the following segment's latency-bound chain.
               slice  (late=True, closing iteration of a window) the bucket's optimizer slice behind the late piece, where its
                      gradients are final -- or, deferred, its slice of the norm pass.
               Multi-GPU, closing iteration: the bucket's SUM all-reduce follows the piece that finishes its gradients -- late: on the
               late stream, waited for there, before the slice (the update of the decoder's parameters overlaps the encoder's
               backward, only the last bucket's slice is exposed); eager: launched asynchronously, all waited for behind the last.
        tail   (before, after) on the main stream, behind every bucket: skip_nonfinite's flag capture of the window; the norm pass if
               the slices have not run it; the commit, or the default step's whole optimizer (eager).  Multi-GPU skip_nonfinite: the
               ranks agree on the verdict (_agree) between `before` and the commit, which is then alone in `after`.

        main stream:  [forward, loss] [decoder backward] [enc3+enc2 backward] [enc1] [enc0]                 [tail]
        late stream:                                    [decoder weight grads, slice][enc3+enc2 ...]  ...  [enc0 ...]
        (branches of ONE captured graph do not run concurrently on this stack; separate graphs on two streams do)"""
        skip, deferred, opt = self.skip_nonfinite, self._deferred, self._opt
        bind = functools.partial
        chain = []
        for key in GradSync.ORDER:
            main = _Piece([bind(self.plan.backward, tags=key)])
            if not chain:
                main[:0] = ([bind(self._capture_flags, False)] if skip else []) + [self._loss_backward]
            # tests: grad_hook runs (captured) where this bucket's gradients have become final
            hook = [bind(self.grad_hook, key)] if skip and self.grad_hook is not None else []
            if late:
                chain.append(Bucket(main, _Piece([bind(self.plan.run_late, key)] + hook), key,
                                    _Piece([bind(self._norm if deferred else self._optimizer, key)]) if opt else None))
            else:
                chain.append(Bucket(_Piece(main + hook), None, key, None))
        before, after = _Piece([bind(self._capture_flags, True)] if skip else []), _Piece()
        if opt and deferred:
            if not late:
                before.append(self._norm)
            (after if skip and self.dist_active else before).append(self._commit)
        elif opt and not late:
            before.append(self._optimizer)
        return Iteration("late" if late else "eager", _Piece([self._forward_and_loss_partials]), chain, (before, after))

    def _variants(self):
        k = self.update_interval
        if k == 1:
            return [(True, True)]
        return [(True, False)] + ([(False, False)] if k > 2 else []) + [(False, True)]

    def _capture(self):
        """Captures one set of graphs per (zero gradients, optimizer) variant the accumulation schedule needs.  Capturing
        executes nothing; one eager warm-up iteration runs first (allocator, lazy module loading) and every buffer it
        changes is restored afterwards."""
        self.plan.ensure_packed()
        keep = (self.model.flat, self.m, self.v, self.pg, self.egn, self.nsq, self.fac, self.model.flat_grad) + \
            ((self.gate,) if self.skip_nonfinite else ()) + ((self.parts, self.clip) if self.max_grad_norm is not None else ()) + \
            ((self.ema,) if self.ema is not None else ())
        saved = [t.clone() for t in keep]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        self._zero, self._opt = True, True
        with torch.cuda.stream(s):
            it = self._iteration(late=False)       # (every piece, no collective)
            for piece in [it.head] + [b.main for b in it.chain] + list(it.tail):
                piece.replay()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if self.plan.fp8_grad_layers:
            # fp8 data gradients: the warm-up iteration above ran with just-in-time scaling and left every layer's scale = its dy's
            # amax / 448 on THIS batch (the calibration); the captured graphs use delayed scaling from here on -- each backward pass
            # starts by turning the previous pass's amax into the scales it quantises with (engine: crd_fp8_scale_update)
            self.plan.fp8_jit = False
        self.graphs = {}
        self.plan.split_late = True
        self.late_stream = (self.late_stream_factory or torch.cuda.Stream)()
        for zero, opt in self._variants():
            self._zero, self._opt = zero, opt
            self._capture_iteration()
        torch.cuda.synchronize()
        for t, sv in zip(keep, saved):
            t.copy_(sv)
        self.plan.packed_version = None        # the warm-up iteration packed ITS updated weights

    def _capture_iteration(self):
        """self.graphs[current variant] <- its _iteration with the pieces captured into graphs: the head as a graph of its own only
        where a collective follows it (multi-GPU), else at the front of the first bucket's; per bucket a main graph, a late graph
        and -- where that bucket's all-reduce comes between them (multi-GPU) -- the slice as a graph of its own, else at the end of
        the late graph; the tail's two halves."""
        it = self._iteration(late=True)
        main, late = self._current_stream(), self.late_stream
        head = self._graph(it.head) if self.dist_active else None
        mains = [self._graph(b.main if head is not None or i else it.head + b.main) for i, b in enumerate(it.chain)]
        chain = []
        for gm, b in zip(mains, it.chain):
            own = b.slice is not None and self.dist_active
            self._stream_wait(late, main)
            gl = self._graph(b.late + (b.slice if b.slice is not None and not own else []), late)
            gs = self._graph(b.slice, late) if own else None
            self._stream_wait(main, late)
            chain.append(Bucket(gm, gl, b.key, gs))
        tail = tuple(self._graph(piece) if piece else None for piece in it.tail)
        self.graphs[(self._zero, self._opt)] = [(Iteration("late", head, chain, tail), None)]

    # graphs and streams as methods, so that the CPU control-flow tests run the very same capture and replay with stand-ins for them
    @staticmethod
    def _graph(fns, stream=None):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for fn in fns:
                fn()
        return g

    @staticmethod
    def _current_stream():
        return torch.cuda.current_stream()

    @staticmethod
    def _stream_wait(waiter, on):
        waiter.wait_stream(on)

    @staticmethod
    def _on_stream(stream):
        return torch.cuda.stream(stream)

    def _run(self, it):
        """One iteration, eager (the _iteration itself) or captured (_capture_iteration): the host's side of the order stated in
        _iteration -- the replays, the two streams and the collectives."""
        late, reduce = it.kind == "late", self._opt and self.dist_active
        if it.head is not None:
            it.head.replay()
        if self.dist_active:
            self._reduce_loss_partials()       # global loss denominators (BerHu: and maxima) before the backward
        if late:
            main = self._current_stream()
        for b in it.chain:
            with trace.range("main:" + "+".join(b.key)):
                b.main.replay()
            if late:
                self._stream_wait(self.late_stream, main)
                with self._on_stream(self.late_stream), trace.range("late:" + "+".join(b.key)):
                    b.late.replay()
                    if reduce:
                        self.sync.launch(b.key)    # this bucket's all-reduce, behind the graph that finishes its gradients
                        self.sync.wait()           # (the LATE stream waits for it; the main stream runs on)
                        b.slice.replay()           # ... and the bucket's optimizer slice follows at once
            elif reduce:
                self.sync.launch(b.key)
        if late:
            probe = self.tail_probe
            if probe is not None:              # bench.py: how long the main stream idles behind the late stream at the end of an iteration
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(main)
            self._stream_wait(main, self.late_stream)
            if probe is not None:
                e1.record(main)
                probe.append((e0, e1))
        elif reduce:
            self.sync.wait()
        before, after = it.tail
        if before:
            before.replay()
        if after:
            self._agree()
            after.replay()

    def _agree(self):
        """Multi-GPU skip_nonfinite: every rank skips or commits together.  Non-finite gradient elements reach every rank through
        the SUM all-reduce already; a rank's dropped fixed-point partials do not -- a MAX over the two verdict words spreads them."""
        dist.all_reduce(self.gate[:2], op=dist.ReduceOp.MAX, group=self.sync.group)

    def set_batch(self, batch):
        self.plan.x_in.copy_(batch["image"], non_blocking=True)
        self.gt["full"].copy_(batch["gt_full"], non_blocking=True)
        self.gt["half"].copy_(batch["gt_half"], non_blocking=True)
        self.gt["quarter"].copy_(batch["gt_quarter"], non_blocking=True)
        if "seg" in batch:
            self.gt["seg"].copy_(batch["seg"], non_blocking=True)

    def step(self, last_of_epoch=False):
        """One iteration on the batch currently in the static input buffers (set_batch): forward, losses, backward into
        the accumulating gradient buffer and -- on every update_interval-th iteration or the last of an epoch
        (runner.py:222) -- gradient all-reduce + optimizer step.  Returns True when the optimizer ran."""
        if tuple(p.requires_grad for p in self._params) != self._frozen_sig:
            raise L.CrdError("camradepth_amd.TrainStep: requires_grad of a parameter changed after the step was built (its plan "
                             "and optimizer mask are fixed at construction): build a new TrainStep")
        ema = self.ema is not None
        if ema and self._ema_swapped:
            raise L.CrdError("camradepth_amd.TrainStep.step() inside ema_weights(): the parameters are the averaged weights there; "
                             "leave the context before training on")
        k = self.update_interval
        zero = not self._window_open             # first iteration of an accumulation window: zero the gradients
        pos = self._window_pos if self._window_open else 0
        opt = (pos + 1 == k) or last_of_epoch
        self._zero, self._opt = zero, opt
        if opt:
            self.step_count += 1
            lr, b1 = (self.schedule[min(self.sched_steps, len(self.schedule) - 1)] if self.schedule else (self.lr, self.betas[0]))
            b2 = self.betas[1]
            bc1, bc2 = 1.0 - b1 ** self.step_count, 1.0 - b2 ** self.step_count
            hp_host = self.hp_ring[self.step_count % len(self.hp_ring)]   # ring: the async copy may still be pending
            hp_host[0], hp_host[1], hp_host[2], hp_host[3] = b1, b2, self.eps, self.wd
            hp_host[4] = lr * math.sqrt(bc2) / (bc1 + 1e-8)
            if ema:
                # [5] w_n of this update as the host counts it (the ungated kernels); [6], [7], [15]: decay, base and warm-up, from
                # which the gated commit forms w_n for the device's own count (include/camradepth_hip.h, crd_dgn_desc)
                if not self.skip_nonfinite:
                    self.ema_n += 1
                hp_host[5], hp_host[6] = ema_weight(self.ema_decay, self.ema_warmup, max(self.ema_n, 1))[1], self.ema_decay
                hp_host.view(torch.int32)[7], hp_host.view(torch.int32)[15] = self.ema_base, 1 if self.ema_warmup else 0
            if self.skip_nonfinite:
                hp_host.view(torch.float64)[4:7] = torch.tensor([lr, b1, b2], dtype=torch.float64)
                hp_host.view(torch.int32)[14] = self.step_count
                self.hp.copy_(hp_host, non_blocking=True)
            else:
                self.hp[:8].copy_(hp_host[:8], non_blocking=True)
        if self.use_graph and self.graphs is None:
            self._capture()
            self._zero, self._opt = zero, opt
        self.plan.ensure_packed()              # first step / parameters written from outside since the last one
        if self.use_graph and (zero, opt) not in self.graphs:      # e.g. a flush right after an update (last_of_epoch)
            self._capture_iteration()
        self._run(self.graphs[(zero, opt)][0][0] if self.use_graph else self._iteration(late=False))
        if self.dist_active and self.berhu_acc is not None:
            dist.all_reduce(self.berhu_acc, group=self.sync.group)     # BerHu's loss sums (phase b runs in the backward): losses() only
        if opt:                                # every bucket was re-packed behind its optimizer slice
            self.model.mark_params_changed()
            self.plan.packed_version = self.model._param_version
        # bookkeeping of the reference loop
        self.iter_count += 1
        self.epoch_iter += 1
        self._window_open, self._window_pos = (not opt), (pos + 1)
        if self.epoch_iter > k:                # "to prevent a scheduler step before the optimizer step" (runner.py:269-270)
            self.sched_steps += 1
        return opt

    def _level_losses(self, a):
        """full / half / quarter values of the criterion from the host copy `a` of acc (BerHu: one more copy of its sums and maxima)."""
        b = L.stat_value(self.berhu_acc.cpu()).view(4, 2) if self.berhu_acc is not None else [None] * 3
        mx = self.maxbits.cpu().view(torch.float32).double() if self.maxbits is not None else [None] * 3
        value = CRITERIA[self._depth_mode].value
        return [float(value(a[4 * i:4 * i + 4], b[i], mx[i], self._berhu_thresh)) for i in range(3)]

    def losses(self):
        """Host view of the last iteration's loss terms (synchronises): the criterion's value per depth level; "rmse" is
        sqrt(sum d^2 / count) of the full level whatever the criterion.  Raises CrdError when the iteration's segmentation target
        held a label that is neither a class nor ignore_index 255 (crd_ce_fwd counts them in its acc[2]; torch raises there)."""
        a = L.stat_value(self.acc.cpu())
        dropped = L.nonfinite()
        if self.sup and a[14] != 0:
            raise L.CrdError(f"TrainStep: {int(a[14])} segmentation label(s) of the last iteration are neither in "
                             f"[0, {self.model.cfg.num_classes}) nor ignore_index 255")
        if dropped:
            # a NaN / infinite / out-of-range partial was dropped from a fixed-point sum since the last check (include/camradepth_hip.h:
            # crd_nonfinite_status): the sums are not what the reference would have computed -- it reports NaN here, so do we
            nan = float("nan")
            return {"loss": nan, "full": nan, "half": nan, "quarter": nan, "seg": nan, "rmse": nan}
        full, half, quarter = self._level_losses(a)
        rmse = math.sqrt(float(a[2] / a[1]))
        seg = 0.0
        if self.sup:
            ce = float(a[12] / a[13])
            seg = (1 - math.exp(-ce)) ** 2 * ce
        total = (LOSS_W[0] * full + LOSS_W[1] * half + LOSS_W[2] * quarter + LOSS_W[3] * seg) / sum(LOSS_W) / self.update_interval
        return {"loss": total, "full": full, "half": half, "quarter": quarter, "seg": seg, "rmse": rmse}


def _delegate(name):
    return property(lambda self: getattr(self.state, name), lambda self, v: setattr(self.state, name, v))


for _n in _STATE_FIELDS:
    setattr(TrainStep, _n, _delegate(_n))
