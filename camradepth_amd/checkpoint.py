"""Checkpoint interchange with the reference.

The reference writes `{'state_dict', 'optimizer', 'lr', 'steps'}` with `torch.save` (src/main/runner.py:369-371) and
reads checkpoints through `load_checkpoint_with_shape_match` (src/utils/utils.py:352-370): a 'module.' prefix left by
DataParallel is stripped and only entries whose shape matches the model are taken, which is how a model of one variant
is initialised from a checkpoint of another ("transfer learning", args.py:95-100).  camradepth_amd keeps parameters in
the reference's own names, shapes and NCHW fp32 layout (they are views of one flat buffer; the bf16 packed forms the
kernels read are derived every step), so a checkpoint is interchangeable in both directions without conversion."""
import torch


def strip_module_prefix(state_dict):
    return {k.replace("module.", ""): v for k, v in state_dict.items()}


def load_state_dict_shape_match(model, checkpoint_state_dict):
    """utils.py:352-370.  Returns (missing, mismatched): keys of the model absent from the checkpoint and keys whose
    shapes differ (both keep the model's current values); the reference prints them."""
    ckpt = strip_module_prefix(checkpoint_state_dict)
    own = model.state_dict()
    new, missing, mismatched = {}, [], []
    for key, cur in own.items():
        if key in ckpt and tuple(ckpt[key].shape) == tuple(cur.shape):
            new[key] = ckpt[key]
        else:
            (missing if key not in ckpt else mismatched).append(key)
            new[key] = cur
    model.load_state_dict(new, strict=True)
    return missing, mismatched


def trainstep_optimizer_state_dict(ts):
    """A TrainStep's diffGradNorm state as the reference's optimizer.state_dict() (one param_group over the model's parameters in
    their registration order).  `step` is the count of COMMITTED steps, read from the device: steps that skip_nonfinite skipped
    are not in it, as GradScaler.step's skipped steps are not in the reference's."""
    names = list(ts.model._names)
    per = ts.optimizer_state()
    lr, b1 = ts.schedule[min(ts.sched_steps, len(ts.schedule) - 1)] if ts.schedule else (ts.lr, ts.betas[0])
    return {"state": {i: dict(per[n]) for i, n in enumerate(names)},
            "param_groups": [{"lr": lr, "betas": (b1, ts.betas[1]), "eps": ts.eps, "weight_decay": ts.wd, "params": list(range(len(names)))}]}


def load_trainstep_optimizer_state(ts, osd):
    """The inverse of trainstep_optimizer_state_dict: moments, previous gradients, grad-norm averages and the step count."""
    steps = {int(s["step"]) for s in osd["state"].values()}
    if len(steps) != 1:
        raise ValueError(f"load_trainstep_optimizer_state: non-uniform step counts {sorted(steps)}")
    for i, n in enumerate(ts.model._names):
        src = osd["state"][i]
        a, b = ts.state.seg_host[i]
        ts.m[a:b].copy_(torch.as_tensor(src["exp_avg"]).reshape(-1))
        ts.v[a:b].copy_(torch.as_tensor(src["exp_avg_sq"]).reshape(-1))
        ts.pg[a:b].copy_(torch.as_tensor(src["previous_grad"]).reshape(-1))
        ts.egn[i] = float(src["exp_grad_norm"])
    ts.step_count = steps.pop()
    if ts.gate is not None:
        ts.gate.zero_()
        ts.gate[2] = ts.step_count


def save_checkpoint(path, model, optimizer=None, steps=(0, 0)):
    """Same dictionary as runner.py:369 (tensors moved to the CPU; the model itself stays on its device).  optimizer: a torch
    optimizer (camradepth_amd.diffGradNorm) or a TrainStep (trainstep_optimizer_state_dict).  A TrainStep that keeps an EMA of the
    weights (ema_decay) adds "ema_state_dict" (the averaged weights under the model's keys), "ema_decay" and "ema_updates"; without
    one the key set is the reference's.  Inside ts.ema_weights() the two sets are exchanged, and so are the two entries."""
    state = {"state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, "steps": list(steps)}
    if optimizer is not None:
        osd = trainstep_optimizer_state_dict(optimizer) if hasattr(optimizer, "optimizer_state") else optimizer.state_dict()
        for st in osd["state"].values():
            for k, v in list(st.items()):
                if torch.is_tensor(v):
                    st[k] = v.detach().cpu().clone()
        state["optimizer"] = osd
        state["lr"] = osd["param_groups"][0]["lr"] if hasattr(optimizer, "optimizer_state") else optimizer.param_groups[0]["lr"]
        if hasattr(optimizer, "ema_state_dict") and getattr(optimizer, "ema", None) is not None:
            state["ema_state_dict"] = {k: v.detach().cpu().clone() for k, v in optimizer.ema_state_dict().items()}
            state["ema_decay"], state["ema_updates"] = optimizer.ema_decay, optimizer.ema_updates
    torch.save(state, path)
    return state


def load_checkpoint(path_or_state, model, optimizer=None, shape_match=True):
    """Loads `state_dict` (with the reference's shape-matching rule unless shape_match=False) and, if given and present,
    the optimizer state.  Returns (missing, mismatched, steps).  A TrainStep with ema_decay gets its EMA and update count back from
    "ema_state_dict" / "ema_updates" (entries whose shape matches, the rest keep the loaded weights); from a checkpoint without them
    the EMA is re-seeded from the loaded weights with the count at 0.  (model.load_state_dict() alone does not touch the EMA.)"""
    state = torch.load(path_or_state, map_location="cpu", weights_only=False) if isinstance(path_or_state, str) else path_or_state
    sd = state["state_dict"] if "state_dict" in state else state
    if shape_match:
        missing, mismatched = load_state_dict_shape_match(model, sd)
    else:
        model.load_state_dict(strip_module_prefix(sd))
        missing, mismatched = [], []
    if optimizer is not None and "optimizer" in state:
        if hasattr(optimizer, "optimizer_state"):
            load_trainstep_optimizer_state(optimizer, state["optimizer"])
        else:
            optimizer.load_state_dict(state["optimizer"])
    if optimizer is not None and hasattr(optimizer, "ema_state_dict") and getattr(optimizer, "ema", None) is not None:
        optimizer.reseed_ema(0)
        if "ema_state_dict" in state:
            src = strip_module_prefix(state["ema_state_dict"])
            for k, dst in optimizer.ema_state_dict().items():
                if k in src and tuple(src[k].shape) == tuple(dst.shape):
                    dst.copy_(torch.as_tensor(src[k]))
            optimizer._set_ema_updates(int(state.get("ema_updates", 0)))
    return missing, mismatched, state.get("steps", [0, 0])
