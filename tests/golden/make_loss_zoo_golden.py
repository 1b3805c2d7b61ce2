#!/usr/bin/env python3
"""Generate tests/golden/loss_zoo.npz by importing the REAL reference's loss_funcs.py on CPU (as make_golden.py's G6 section,
with its stand-ins for the absent third-party packages): loss values and input gradients of MaskedL1Loss, MaskedHuberLoss,
MaskedRMSELoss, MaskedBerHuLoss (thresh 0.2) and SmoothnessLoss on the cases of tests/loss_zoo_cases.py.  Nothing of the
reference is copied: the fixture holds output values only, the inputs are rebuilt from seeds.

    python tests/golden/make_loss_zoo_golden.py [--out PATH]
"""
import argparse
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import REF, install_shims  # noqa: E402

CLASSES = ("l1", "huber", "rmse", "berhu", "smooth")


def generate(out):
    import numpy as np
    import torch
    torch.set_num_threads(1)                 # one summation order: the fixture reproduces bit for bit
    install_shims()
    sys.argv = ["x", "--split", f"{REF}/src/data/new_split.npy", "--output_dir", tempfile.mkdtemp()]
    sys.path.insert(0, f"{REF}/src")
    from utils import loss_funcs as lf       # noqa: E402  (reference)
    from tests.loss_zoo_cases import CASES, depth_pair, grad_view, smooth_pair

    crit = {"l1": lf.MaskedL1Loss(), "huber": lf.MaskedHuberLoss(), "rmse": lf.MaskedRMSELoss(), "berhu": lf.MaskedBerHuLoss(thresh=0.2)}
    smooth = lf.SmoothnessLoss()
    store = {}
    for case in CASES:
        p_np, t_np = depth_pair(case)
        store[f"{case}__inputs_sum"] = np.array([p_np.astype(np.float64).sum(), t_np.astype(np.float64).sum()])
        for name, c in crit.items():
            pred = torch.from_numpy(p_np.copy()).requires_grad_(True)
            loss = c(pred, torch.from_numpy(t_np))
            loss.backward()
            store[f"{case}__{name}__loss"] = np.float64(loss.detach().item())
            store[f"{case}__{name}__grad"] = grad_view(case, pred.grad.numpy())
        sp, im = smooth_pair(case)
        store[f"{case}__smooth__inputs_sum"] = np.array([sp.astype(np.float64).sum(), im.astype(np.float64).sum()])
        pd = torch.from_numpy(sp.copy()).requires_grad_(True)
        loss = smooth(pd, torch.from_numpy(im))
        loss.backward()
        store[f"{case}__smooth__loss"] = np.float64(loss.detach().item())
        store[f"{case}__smooth__grad"] = grad_view(case, pd.grad.numpy())
    np.savez_compressed(out, **store)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "loss_zoo.npz"))
    generate(ap.parse_args().out)
