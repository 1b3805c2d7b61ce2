"""diffGradNorm optimizer on one multi-tensor HIP kernel sequence (3 launches per step, no host sync).

Same constructor, `param_groups` and per-parameter `state` keys as the reference
(src/models/diffGradNorm.py:26-37,63-71) so `OneCycleLR(cycle_momentum=True)` can drive `lr` and
`betas[0]` every iteration (src/main/runner.py:151-152,270) and optimizer state_dicts interchange.
"""
import ctypes as C

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import lib as L

_CHUNK = 4096


def check_max_grad_norm(value, who):
    """None (no clipping) or a max_norm of torch.nn.utils.clip_grad_norm_ (> 0; +inf: the norm only) -> float | None, or CrdError."""
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not v > 0.0:                                    # (NaN fails this too)
        raise L.CrdError(f"{who}(max_grad_norm={value!r}): max_grad_norm must be a number > 0 (float('inf') monitors the norm only)")
    return v


def check_ema_decay(value, who):
    """None (no EMA of the weights) or its decay d, 0 <= d < 1 -> float | None, or CrdError."""
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not 0.0 <= v < 1.0:          # (NaN fails this too)
        raise L.CrdError(f"{who}(ema_decay={value!r}): ema_decay must be a number with 0 <= ema_decay < 1")
    return v


def ema_weight(decay, warmup, n):
    """(d_n, w_n) of EMA update n = 1, 2, ... as Python floats holding fp32 values: d_n = min(decay, (1 + n) / (10 + n)) with the
    warm-up (timm's rule), else decay; w_n = 1 - d_n.  The fp32 expression of the kernels (csrc/train_ops.hip: dgn_ema_weight), so
    the w_n the host uploads and the one the gated commit forms on the device are the same bits."""
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + n) / np.float32(10 + n))
    return float(d), float(np.float32(1.0) - d)


def dgn_desc(**fields):
    """crd_dgn_desc (include/camradepth_hip.h) from named values.  A tensor stands for its device address (an int is taken as an
    address already: a slice that starts inside a buffer); fields left out are 0 / NULL, step is 1.  gate / clip / ema = None switch
    the feature off."""
    d = L.DgnDesc(step=1)
    for k, v in fields.items():
        if not hasattr(L.DgnDesc, k):
            raise TypeError(f"crd_dgn_desc has no field {k!r}")
        setattr(d, k, v.data_ptr() if torch.is_tensor(v) else v)
    return d


class diffGradNorm(Optimizer):
    """skip_nonfinite=True: GradScaler.step's guard on the gated kernels -- a step whose gradients hold a NaN / inf element, or whose
    backward dropped a non-finite partial from a fixed-point sum (camradepth_amd.CamRaDepth's backward), writes nothing and does
    not advance any `step` count.  step() then reads the verdict once (one sync, as GradScaler.step does); found_inf holds it.

    max_grad_norm=c: torch.nn.utils.clip_grad_norm_(params, c) fused into the step -- the gradients are scaled by
    min(1, c / (||g|| + 1e-6)), ||g|| over every parameter with a gradient, before the weight decay is added.  The scaling happens
    on the fly: .grad keeps the unclipped values.  grad_norm: the last step's ||g|| as a 0-d device tensor (no sync).  One param
    group only (the norm is global).  An optimizer attribute, not a param_groups key, so state_dicts stay the reference's.

    ema_decay=d (0 <= d < 1): an exponential moving average of the parameters kept by the update kernel itself, one fp32 buffer per
    param group seeded with the parameters when the group is first laid out: every committed step n = 1, 2, ... does
    e <- e + w_n (p_new - e), w_n = 1 - min(d, (1 + n) / (10 + n)) with ema_warmup (timm's rule), else 1 - d.  Parameters without a
    gradient and skipped steps leave it untouched.  ema_state() maps each parameter to its EMA view.  Any number of param groups;
    like max_grad_norm an optimizer attribute, not a param_groups key, and not part of state_dict()."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, skip_nonfinite=False, max_grad_norm=None,
                 ema_decay=None, ema_warmup=True):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        max_grad_norm = check_max_grad_norm(max_grad_norm, "camradepth_amd.diffGradNorm")
        ema_decay = check_ema_decay(ema_decay, "camradepth_amd.diffGradNorm")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._groups = None
        self.skip_nonfinite = bool(skip_nonfinite)
        self.found_inf, self.skipped_steps = False, 0
        self.max_grad_norm, self.grad_norm = max_grad_norm, None
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self._check_groups()

    def _check_groups(self):
        if self.max_grad_norm is not None and len(self.param_groups) > 1:
            raise L.CrdError(f"camradepth_amd.diffGradNorm(max_grad_norm=...) takes one param group, got {len(self.param_groups)}: the "
                             "clipping norm is global (clip per group with torch.nn.utils.clip_grad_norm_ in an eager loop)")

    # ------------------------------------------------------------------ flat layout
    def _build(self, group):
        ps = [p for p in group["params"]]
        dev = ps[0].device
        if not ps[0].is_cuda:
            raise L.CrdError("camradepth_amd.diffGradNorm runs on an MI355X only (no CPU fallback)")
        # parameters that already live in one flat buffer (camradepth_amd.CamRaDepth) are used in place
        base = min(p.data_ptr() for p in ps)
        offs = [(p.data_ptr() - base) // 4 for p in ps]
        order = sorted(range(len(ps)), key=lambda i: offs[i])
        span = max(o + p.numel() for o, p in zip(offs, ps))
        contiguous = span <= 2 * sum(p.numel() for p in ps) + 8 * len(ps) and all(
            offs[order[i]] + ps[order[i]].numel() <= offs[order[i + 1]] for i in range(len(ps) - 1))
        st = {"ps": ps, "adopted": not contiguous}
        if not contiguous:
            # adopt: move the parameters into one flat buffer (their .data become views)
            n, offs = 0, []
            for p in ps:
                offs.append(n)
                n += (p.numel() + 7) // 8 * 8
            flat = torch.zeros(n, dtype=torch.float32, device=dev)
            for p, o in zip(ps, offs):
                flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = flat[o:o + p.numel()].view(p.shape)
            st["flat_p"], span = flat, n
        else:
            st["flat_p"] = None
        st["offs"], st["span"], st["base"] = offs, span, min(p.data_ptr() for p in ps)
        st["flat_g"] = torch.zeros(span, dtype=torch.float32, device=dev)
        st["m"], st["v"], st["pg"] = (torch.zeros(span, dtype=torch.float32, device=dev) for _ in range(3))
        nt = len(ps)
        st["egn"], st["fac"] = (torch.zeros(nt, dtype=torch.float32, device=dev) for _ in range(2))
        seg = torch.tensor([[o, o + p.numel()] for o, p in zip(offs, ps)], dtype=torch.int64)
        # kernel wants seg_off[t], seg_off[t+1]: store begin/end pairs as 2*t, 2*t+1 and index tensors by 2*t
        b2s, b2c = [], []
        for t, p in enumerate(ps):
            for c in range((p.numel() + _CHUNK - 1) // _CHUNK):
                b2s.append(t)
                b2c.append(c)
        st["seg"], st["nblk"] = seg.to(dev), len(b2s)
        st["nsq"] = torch.zeros(len(b2s), dtype=torch.float32, device=dev)      # per-workgroup parts of ||g||^2
        st["b2s"] = torch.tensor(b2s, dtype=torch.int32, device=dev)
        st["b2c"] = torch.tensor(b2c, dtype=torch.int32, device=dev)
        st["active"] = torch.ones(nt, dtype=torch.uint8, device=dev)
        st["step"] = 0
        st["gate"] = None                        # skip_nonfinite: the verdict words (created on the first gated step)
        st["parts"] = st["clip"] = None          # max_grad_norm: 4 rows of norm parts, [total, coef] (created on the first clipped step)
        st["ema"], st["ema_n"] = None, 0         # ema_decay: the group's EMA (layout of the parameters' flat span), its update count
        if self.ema_decay is not None:
            st["ema"] = torch.zeros(span, dtype=torch.float32, device=dev)
            for p, o in zip(ps, offs):
                st["ema"][o:o + p.numel()].copy_(p.detach().reshape(-1))
        for t, (p, o) in enumerate(zip(ps, offs)):
            s = self.state[p]
            s["step"] = 0
            s["exp_avg"] = st["m"][o:o + p.numel()].view(p.shape)
            s["exp_avg_sq"] = st["v"][o:o + p.numel()].view(p.shape)
            s["previous_grad"] = st["pg"][o:o + p.numel()].view(p.shape)
            s["exp_grad_norm"] = st["egn"][t]
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        if self._groups is None:
            self._groups = [self._build(g) for g in self.param_groups]
        lb = L.load()
        for group, st in zip(self.param_groups, self._groups):
            ps, offs = st["ps"], st["offs"]
            # gradient source: in place when the grads are views of one buffer parallel to the params
            act_host = [p.grad is not None for p in ps]
            if not any(act_host):
                continue
            i0 = act_host.index(True)
            g0 = ps[i0].grad
            # The kernel's bias corrections use ONE step count per group (st["step"]).  The reference keeps one per parameter
            # (diffGradNorm.py:66,76-77): they differ only for a parameter that is frozen for some steps and unfrozen later
            # (or a checkpoint with non-uniform steps) -- including the case where the WHOLE active set switches (A frozen after
            # n steps, B unfrozen: B's own count is 0, the group's is n).  Refuse that silently-different case instead of
            # approximating it, BEFORE anything is modified (no kernel launch, no change of st["active"] / st["act_host"]).
            steps = {self.state[p]["step"] + 1 for p, a_ in zip(ps, act_host) if a_}
            if steps != {st["step"] + 1}:
                raise L.CrdError("camradepth_amd.diffGradNorm: the active parameters' step counts "
                                 f"({sorted(steps)}) differ from the group's ({st['step'] + 1}): unfreezing a parameter mid-run (or "
                                 "loading such a checkpoint) needs one param_group per step count")
            # frozen parameters (grad None) are skipped through the `active` mask; the others' grads are used in place
            parallel = all(p.grad is None or (p.grad.data_ptr() - g0.data_ptr()) == 4 * (o - offs[i0]) for p, o in zip(ps, offs))
            if parallel:
                gptr = g0.data_ptr() - 4 * offs[i0]
                if act_host != st.get("act_host"):
                    st["active"].copy_(torch.tensor(act_host, dtype=torch.uint8))
                    st["act_host"] = act_host
            else:
                fg = st["flat_g"]
                for p, o in zip(ps, offs):
                    if p.grad is not None:
                        fg[o:o + p.numel()].copy_(p.grad.reshape(-1))
                gptr = fg.data_ptr()
                st["active"].copy_(torch.tensor(act_host, dtype=torch.uint8))
                st["act_host"] = None
            beta1, beta2 = group["betas"]
            # one call whatever the switches: norm pass, then the commit.  skip_nonfinite: the verdict words; max_grad_norm: 4 rows of
            # norm parts and [total, coef]; ema_decay: ungated the host numbers the update, gated the device counts (gate[2], base 0:
            # the gate and the EMA of a group start together)
            gate = self._gate(st, ps) if self.skip_nonfinite else None
            clipped = self.max_grad_norm is not None
            if clipped and st["parts"] is None:
                st["parts"] = torch.zeros(4 * st["nblk"], dtype=torch.float32, device=ps[0].device)
                st["clip"] = torch.zeros(2, dtype=torch.float32, device=ps[0].device)
            if st["ema"] is not None and gate is None:
                st["ema_n"] += 1
            d = dgn_desc(p=st["flat_p"] if st["flat_p"] is not None else st["base"], g=gptr, exp_avg=st["m"], exp_avg_sq=st["v"],
                         prev_grad=st["pg"], exp_grad_norm=st["egn"], factor=st["fac"], parts=st["parts"] if clipped else st["nsq"],
                         parts_stride=st["nblk"] if clipped else 0, seg_off=st["seg"], blk2seg=st["b2s"], blk2chunk=st["b2c"],
                         n_tensors=len(ps), n_blocks=st["nblk"], active=None if all(act_host) else st["active"], lr=float(group["lr"]),
                         beta1=float(beta1), beta2=float(beta2), eps=float(group["eps"]), weight_decay=float(group["weight_decay"]),
                         step=st["step"] + 1, gate=gate, clip=st["clip"] if clipped else None, max_norm=self.max_grad_norm or 0.0,
                         ema=st["ema"], ema_decay=self.ema_decay or 0.0, ema_warmup=int(self.ema_warmup), ema_n=st["ema_n"])
            L.check(lb.crd_diffgradnorm_step(C.byref(d), L.stream()), "crd_diffgradnorm_step")
            if clipped:
                self.grad_norm = st["clip"][0].clone()        # (enqueued: no sync)
            if gate is not None:
                skipped = bool(int(gate[4]))            # the one read of the step
                gate[:2].zero_()                         # the next window starts without a verdict
                self.found_inf = skipped
                if skipped:
                    self.skipped_steps += 1
                    continue
                if st["ema"] is not None:
                    st["ema_n"] += 1                 # (the device counted it itself: gate[2])
            self._count_step(st, ps, act_host)
            self._mark_changed(ps)
        return loss

    @staticmethod
    def _mark_changed(ps):
        for ow in {getattr(p, "_crd_owner", None) for p in ps}:        # graph-replayed forwards re-pack their weights
            if ow is not None and ow() is not None:
                ow().mark_params_changed()

    def ema_state(self):
        """parameter -> its EMA (a view of the group's EMA buffer, the parameter's shape)."""
        if self.ema_decay is None:
            raise L.CrdError("camradepth_amd.diffGradNorm.ema_state(): the optimizer was built without ema_decay")
        if self._groups is None:
            self._groups = [self._build(g) for g in self.param_groups]
        return {p: st["ema"][o:o + p.numel()].view(p.shape) for st in self._groups for p, o in zip(st["ps"], st["offs"])}

    def _count_step(self, st, ps, act_host):
        st["step"] += 1
        for p, a_ in zip(ps, act_host):
            if a_:
                self.state[p]["step"] += 1

    def _gate(self, st, ps):
        """The group's verdict words; the owning model's backward captures its dropped partials into gate[1] (model._nf_gate)."""
        if st["gate"] is None:
            st["gate"] = torch.zeros(8, dtype=torch.int32, device=ps[0].device)
            for ow in {getattr(p, "_crd_owner", None) for p in ps}:
                if ow is not None and ow() is not None:
                    ow()._nf_gate = st["gate"]
        return st["gate"]

    def load_state_dict(self, state_dict):
        """Restores a checkpoint written by this class or by the reference's diffGradNorm (same per-parameter keys:
        step, exp_avg, exp_avg_sq, previous_grad, exp_grad_norm; runner.py:369).  torch's loader replaces the state
        tensors; the kernels work on flat buffers the state entries are views of, so the loaded values are copied into
        those buffers and the views re-attached."""
        super().load_state_dict(state_dict)
        loaded = {p: dict(self.state[p]) for g in self.param_groups for p in g["params"] if p in self.state}
        if self._groups is None:
            self._groups = [self._build(g) for g in self.param_groups]
        for group, st in zip(self.param_groups, self._groups):
            for t, (p, o) in enumerate(zip(st["ps"], st["offs"])):
                n = p.numel()
                views = {"exp_avg": st["m"][o:o + n].view(p.shape), "exp_avg_sq": st["v"][o:o + n].view(p.shape),
                         "previous_grad": st["pg"][o:o + n].view(p.shape)}
                src = loaded.get(p)
                if src is not None:
                    for k, v in views.items():
                        if k in src:
                            v.copy_(torch.as_tensor(src[k]).to(v.device, v.dtype).reshape(p.shape))
                    if "exp_grad_norm" in src:
                        st["egn"][t] = float(src["exp_grad_norm"])
                    st["step"] = max(st["step"], int(src.get("step", 0)))
                s = self.state[p]
                s.update(views)
                s["exp_grad_norm"] = st["egn"][t]
                s["step"] = st["step"]

    def zero_grad(self, set_to_none=False):
        """Gradients live in one flat buffer that the backward kernels accumulate into; they are zeroed in
        place (the reference's set_to_none=True would detach the views the kernels write through)."""
        for group in self.param_groups:
            owners = {getattr(p, "_crd_owner", None) for p in group["params"]}
            if len(owners) == 1 and None not in owners and next(iter(owners))() is not None:
                next(iter(owners))().zero_grad()          # one fill of the flat gradient buffer
                continue
            for p in group["params"]:
                if p.grad is not None:
                    p.grad.zero_()
