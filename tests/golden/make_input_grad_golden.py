#!/usr/bin/env python3
"""Gradient of the training loss with respect to the model INPUT (x.grad), from the REAL reference in float64.

Golden weights (synth.fill_state_dict seed 0), full depths, batch synth.make_batch(2, 64, 96, seed=77), the loss combination of
Trainer.train_one_epoch (runner.py:197-218), in eval mode and in train mode with the injected DropPath / Dropout2d masks of
synth.make_masks(cfg, 2, seed=4321) -- the settings of make_golden.py's G2t fixture, evaluated in fp64 (make_fp64_golden.py's
reason: an fp32 run is reproducible only on the CPU it was made on).  tests/test_input_grad_cpu.py pins the oracle's autograd x.grad
to it.  Stored per variant and mode: the loss terms, x.grad at a fixed sample of 1024 pixel positions (every channel) and the
per-channel sum and sum of squares of the whole x.grad.

Runs only in the build container (needs the reference; see make_golden.py for the shims).  Output: input_grad_fp64.npz

    python tests/golden/make_input_grad_golden.py       # both variants, one subprocess each
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, install_shims  # noqa: E402

VARIANTS = ["base", "supervised_seg"]
OUT = os.path.join(HERE, "input_grad_fp64.npz")
NPIX = 1024


def sample_positions(B, H, W, n=NPIX, seed=2024):
    """Fixed (b, y, x) sample shared by the generator and the test."""
    g = np.random.default_rng(seed)
    idx = g.choice(B * H * W, size=n, replace=False)
    idx.sort()
    return idx // (H * W), (idx // W) % H, idx % W


def run_variant(variant, part):
    import torch
    import torch.nn as nn
    torch.manual_seed(0)
    torch.set_default_dtype(torch.float64)
    DropPath = install_shims()
    tmp = tempfile.mkdtemp()
    sys.argv = ["x", "--split", f"{REF}/src/data/new_split.npy", "--model", variant, "--output_dir", tmp]
    sys.path.insert(0, f"{REF}/src")
    sys.path.insert(0, REPO)
    from models.CamRaDepth import CamRaDepth  # noqa: E402  (reference)
    from utils.loss_funcs import MaskedFocalLoss, MaskedMSELoss, MaskedSmoothL1Loss  # noqa: E402
    from camradepth_amd import synth
    from camradepth_amd.config import ModelConfig

    cfg = ModelConfig.variant(variant)
    model = CamRaDepth(input_channels=7)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v.numpy().astype(np.float64)) for k, v in synth.fill_state_dict(shapes, seed=0).items()},
                          strict=True)

    def set_masks(masks):
        blocks = [b for s in range(1, 5) for b in getattr(model.dest_encoder, f"block{s}")]
        for i, b in enumerate(blocks):
            if isinstance(b.drop_path, DropPath):
                b.drop_path.injected = None if masks is None else masks["drop_path"][i].double()
        if masks is None:
            model.dropout = nn.Dropout2d(0.2)
            model.dropout.train(model.training)
        else:
            it = iter(masks["dropout2d"])

            class Inject(nn.Module):
                def forward(self, x):
                    return x * next(it).double().view(x.shape[0], x.shape[1], 1, 1)
            model.dropout = Inject()

    crit_d, crit_s, crit_m = MaskedSmoothL1Loss(), MaskedFocalLoss(), MaskedMSELoss()

    def loss_of(out, batch):
        seg = out["seg"]["final_seg"]
        inter = out["depth"]["intermediate_depths"]
        l_seg = (crit_s(seg, batch["seg"]) if seg is not None else 0) * (1 if cfg.supervised_seg else 0)
        l4 = crit_d(inter[-1].squeeze(1), batch["gt_half"].squeeze(1))
        l3 = crit_d(inter[-2].squeeze(1), batch["gt_quarter"].squeeze(1))
        lf = crit_d(out["depth"]["final_depth"], batch["gt_full"])
        w = [1, 1, 1, 0.2, 0.2]
        loss = (w[0] * lf + w[1] * l4 + w[2] * l3 + w[3] * l_seg + w[4] * 0) / sum(w)
        rmse = torch.sqrt(crit_m(out["depth"]["final_depth"], batch["gt_full"]))
        return loss, lf, l4, l3, l_seg, rmse

    batch = synth.make_batch(2, 64, 96, seed=77)
    batch = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    bi, yi, xi = sample_positions(2, 64, 96)
    store = {}
    for mode in ("eval", "train"):
        model.train(mode == "train")
        set_masks(synth.make_masks(cfg, 2, seed=4321) if mode == "train" else None)
        model.zero_grad(set_to_none=True)
        x = batch["image"].clone().requires_grad_(True)
        out = model(x)
        terms = loss_of(out, batch)
        terms[0].backward()
        g = x.grad.detach()
        key = f"{variant}_{mode}_"
        store[key + "loss"] = np.array([float(t) for t in terms], dtype=np.float64)
        store[key + "xgrad_sample"] = g[bi, :, yi, xi].numpy()                          # [NPIX, C]
        store[key + "xgrad_chan_sum"] = g.sum(dim=(0, 2, 3)).numpy()
        store[key + "xgrad_chan_sumsq"] = (g * g).sum(dim=(0, 2, 3)).numpy()
        assert all(v.dtype == np.float64 for v in store.values())
    np.savez(part, **store)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default=None)
    ap.add_argument("--part", default=None)
    a = ap.parse_args()
    if a.variant is None:
        merged = {}
        with tempfile.TemporaryDirectory() as d:
            for v in VARIANTS:
                print("== input-gradient fixture for", v, flush=True)
                part = os.path.join(d, v + ".npz")
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--variant", v, "--part", part])
                merged.update(dict(np.load(part)))
        np.savez_compressed(OUT, **merged)
    else:
        run_variant(a.variant, a.part)
