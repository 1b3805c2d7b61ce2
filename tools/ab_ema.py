"""A/B of TrainStep(ema_decay=...) against the default step at bench.py's config C2 (base model, batch 8, 7 x 256 x 416,
captured graphs), both variants in ONE process, timed in alternating blocks so that clock drift hits both alike.  Prints one
JSON line: median ms per step of each and the difference.  --skip-nonfinite / --max-grad-norm put BOTH variants on the deferred
commit, where the whole update kernel (and the EMA's share of it) lies in the exposed tail."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--ema-decay", type=float, default=0.9999)
    ap.add_argument("--skip-nonfinite", action="store_true")
    ap.add_argument("--max-grad-norm", type=float, default=None)
    a = ap.parse_args()
    from camradepth_amd import synth
    from camradepth_amd.model import CamRaDepth
    from camradepth_amd.trainer import TrainStep, one_cycle
    batch = {k: v.cuda() for k, v in synth.make_batch(8, 256, 416, seed=1234).items()}
    total = a.warmup + a.blocks * a.steps + 8
    steps = {}
    for on in (False, True):
        model = CamRaDepth(input_channels=7, seed=0).cuda().train()
        ts = TrainStep(model, 8, 256, 416, lr=6e-5, schedule=one_cycle(total, 6e-5), ema_decay=a.ema_decay if on else None,
                       skip_nonfinite=a.skip_nonfinite, max_grad_norm=a.max_grad_norm)
        ts.set_batch(batch)
        for _ in range(a.warmup):
            ts.step()
        steps[on] = ts
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for blk in range(a.blocks):
        for on in ((False, True) if blk % 2 == 0 else (True, False)):
            ts = steps[on]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                ts.step()
            e1.record()
            torch.cuda.synchronize()
            times[on].append(e0.elapsed_time(e1) / a.steps)
    off, on = statistics.median(times[False]), statistics.median(times[True])
    print(json.dumps({"metric": "ab_ema_c2_step_ms", "skip_nonfinite": a.skip_nonfinite, "max_grad_norm": a.max_grad_norm, "off_ms": round(off, 4), "on_ms": round(on, 4),
                      "delta_ms": round(on - off, 4), "off_blocks": [round(t, 4) for t in times[False]],
                      "on_blocks": [round(t, 4) for t in times[True]], "ema_updates": steps[True].ema_updates}))


if __name__ == "__main__":
    main()
