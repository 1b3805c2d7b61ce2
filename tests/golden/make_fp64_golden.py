#!/usr/bin/env python3
"""fp64 twin of make_golden.py's G2 fixture: the REAL reference's eval forward at 1x7x64x96 (same golden weights, same input)
evaluated in float64, so that tests/test_oracle_golden.py can pin the oracle's arithmetic without depending on how the CPU that
runs the test groups fp32 sums (the fp32 fixture is bit-reproducible only on the thread count / instruction set it was made on).

Runs only in the build container (needs the reference; see make_golden.py for the shims).  Output: forward64x96_fp64_<variant>.npz

    python tests/golden/make_fp64_golden.py       # all variants, one subprocess each
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, VARIANTS, install_shims, sub, t2n  # noqa: E402


def run_variant(variant):
    import torch
    torch.manual_seed(0)
    torch.set_default_dtype(torch.float64)      # parameters and every tensor the reference creates inside its forward
    install_shims()
    tmp = tempfile.mkdtemp()
    sys.argv = ["x", "--split", f"{REF}/src/data/new_split.npy", "--model", variant, "--output_dir", tmp]
    sys.path.insert(0, f"{REF}/src")
    sys.path.insert(0, REPO)
    from models.CamRaDepth import CamRaDepth  # noqa: E402  (reference)
    from camradepth_amd import synth
    model = CamRaDepth(input_channels=7)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v.numpy().astype(np.float64)) for k, v in synth.fill_state_dict(shapes, seed=0).items()},
                          strict=True)
    model.eval()
    x = synth.make_batch(1, 64, 96, seed=1234)["image"].double()
    with torch.no_grad():
        enc, _ = model.dest_encoder(x)
        out = model(x)
    store = {f"eval_enc{i + 1}": t2n(e) for i, e in enumerate(enc)}
    store["eval_final_depth"] = t2n(out["depth"]["final_depth"])
    store["eval_depth_quarter"] = t2n(out["depth"]["intermediate_depths"][2])
    store["eval_depth_half"] = t2n(out["depth"]["intermediate_depths"][3])
    if out["seg"]["final_seg"] is not None:
        store["eval_final_seg"] = sub(out["seg"]["final_seg"], 32768)
    if out["seg"]["unsup_map"] is not None:
        store["eval_unsup_map"] = t2n(out["seg"]["unsup_map"])
    assert all(v.dtype == np.float64 for k, v in store.items() if k != "eval_unsup_map")
    np.savez_compressed(os.path.join(HERE, f"forward64x96_fp64_{variant}.npz"), **store)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default=None)
    a = ap.parse_args()
    if a.variant is None:
        for v in VARIANTS:
            print("== fp64 fixture for", v, flush=True)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--variant", v])
    else:
        run_variant(a.variant)
