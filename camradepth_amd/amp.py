"""`GradScaler` with the interface of torch.amp.GradScaler, so the reference's loop runs unchanged
(src/main/runner.py:159,219,264-265: `scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()`).

camradepth_amd trains in bf16, whose range is fp32's: there is no loss scaling (the scale is 1, update() changes nothing).  What
remains of GradScaler is its guard, and step() is that guard: the optimizer step runs on the gated kernels
(diffGradNorm(skip_nonfinite=True)) and writes nothing when a gradient is NaN / inf or the backward dropped a non-finite partial."""
from . import lib as L
from .optim import diffGradNorm


class GradScaler:
    def __init__(self, device="cuda", init_scale=1.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._enabled = bool(enabled)

    def is_enabled(self):
        return self._enabled

    def get_scale(self):
        return 1.0

    def scale(self, outputs):
        return outputs

    def unscale_(self, optimizer):
        """Nothing to divide: the gradients are already unscaled."""

    def step(self, optimizer, *args, **kwargs):
        """The gated optimizer step; returns what optimizer.step returned, or None when the step was skipped (as torch's)."""
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if not isinstance(optimizer, diffGradNorm):
            raise L.CrdError("camradepth_amd.amp.GradScaler.step: the optimizer must be camradepth_amd.diffGradNorm (its gated kernels "
                             f"are the guard), not {type(optimizer).__name__}")
        optimizer.skip_nonfinite = True
        out = optimizer.step(*args, **kwargs)
        return None if optimizer.found_inf else out

    def update(self, new_scale=None):
        """The scale stays 1 (bf16 needs no dynamic loss scaling)."""

    def state_dict(self):
        return {"scale": 1.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 0} \
            if self._enabled else {}

    def load_state_dict(self, state_dict):
        pass
