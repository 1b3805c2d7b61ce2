"""Times crd_depth_eval (the standard depth-evaluation sums, every distance cap from one pass) at 8 x 256 x 416 and 1 x 928 x 1600
under HIP events, with its achieved GB/s against the 8 bytes per pixel it has to read, for ground truth at the synthetic batches'
20 % density, at 5 % (a lidar sweep projected into the image) and with every pixel valid.  For context, in the same process: what
two distance caps cost before it -- two crd_test_metrics calls with the torch.where between them (Trainer.test).

Each figure is the median over --rounds rounds of --reps back-to-back calls between two events (the accumulator is zeroed once
per round, outside the timed region; adding into a non-zero accumulator costs the same).  Idle-GPU numbers: run it alone.

    python tools/bench_depth_eval.py [--reps 200] [--rounds 7]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import lib  # noqa: E402

HBM_TBS = 6.3


def timed(fn, reps, rounds):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    L = lib.load()
    st = lib.stream()
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds of {a.reps} calls, median (min .. max) us per call", flush=True)
    for (B, H, W) in ((8, 256, 416), (1, 928, 1600)):
        n = H * W
        g = torch.Generator(device="cuda").manual_seed(0)
        d = torch.rand(B, 1, H, W, device="cuda", generator=g) * 98.0 + 1.0
        pred = 1.0 - d * (1.0 + 0.3 * (2.0 * torch.rand(B, 1, H, W, device="cuda", generator=g) - 1.0)) / 100.0
        keep = torch.rand(B, 1, H, W, device="cuda", generator=g)
        acc = torch.zeros(B, 10, 12, dtype=lib.SUM_DTYPE, device="cuda")
        acc4 = torch.zeros(2, B, 4, dtype=lib.SUM_DTYPE, device="cuda")
        floor_us = 8.0 * B * n / HBM_TBS / 1e6
        for density in (0.05, 0.2, 1.0):
            gt = torch.where(keep < density, 1.0 - d / 100.0, torch.zeros_like(d)).contiguous()

            def run():
                lib.check(L.crd_depth_eval(pred.data_ptr(), gt.data_ptr(), B, n, 100.0, 1e-3, 10.0, 10, acc.data_ptr(), st), "crd_depth_eval")

            def before():
                lib.check(L.crd_test_metrics(pred.data_ptr(), gt.data_ptr(), B, n, 100.0, 100.0, acc4[0].data_ptr(), st), "crd_test_metrics")
                gt50 = torch.where(gt * 100.0 < 50.0, torch.zeros_like(gt), gt)
                lib.check(L.crd_test_metrics(pred.data_ptr(), gt50.data_ptr(), B, n, 100.0, 100.0, acc4[1].data_ptr(), st), "crd_test_metrics")

            acc.zero_()
            us, lo, hi = timed(run, a.reps, a.rounds)
            acc4.zero_()
            us2, lo2, hi2 = timed(before, a.reps, a.rounds)
            print(f"crd_depth_eval B{B} {H}x{W} hits {density:4.0%}: {us:6.1f} ({lo:6.1f} .. {hi:6.1f}) us | {8.0 * B * n / us / 1e3:6.0f} GB/s of "
                  f"8 B/pixel ({8.0 * B * n / 1e6:5.1f} MB, floor {floor_us:4.1f} us at {HBM_TBS} TB/s) | two crd_test_metrics + torch.where "
                  f"(two caps before): {us2:6.1f} ({lo2:6.1f} .. {hi2:6.1f}) us", flush=True)
        if lib.nonfinite():
            raise SystemExit("a partial was dropped: the timed inputs were meant to be finite")


if __name__ == "__main__":
    main()
