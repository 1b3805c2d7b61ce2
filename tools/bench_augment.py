"""Times the fused augmented batch assembly -- assemble_batch(augment=...): draw + image table + crd_augment_assemble + the pyramid from
the augmented full map -- for 8 frames 416 x 800 cropped to 256 x 416, under HIP events, against what a user writes without it:
assemble_batch on the full frames, torch indexing for crop and flip (with the mirrored u channel), the pyramid rebuilt with
synth.min_pool_ignore_zero.  Both produce the same tensors (checked once before timing; photometric jitter is off in the comparison,
because the baseline cannot do it, and timed on top for the fused path alone).

Also printed: the fused kernel on its own and its achieved GB/s against the launch's algorithmic bytes -- per output pixel 3 + 12 + 4 + 4
bytes read (image, radar, radial velocity, LiDAR) and 7 x 4 + 4 written, + 1 read and 8 + 2 written with labels.

Each figure is the median over --rounds rounds of --reps back-to-back calls between two events.  Idle-GPU numbers: run it alone.

    python tools/bench_augment.py [--reps 100] [--rounds 7]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import lib, synth  # noqa: E402
from camradepth_amd.batch import Augment, assemble_batch  # noqa: E402

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


def baseline(raw, rows, h, w, levels=3):
    """The parent commit's way: assemble everything, then index.  rows: host list of (y0, x0, flip)."""
    full = assemble_batch(raw["img"], raw["radar"], raw["rv"], raw["depth"], levels=0)
    xs, gs = [], []
    for b, (y0, x0, flip) in enumerate(rows):
        x, g = full["image"][b, :, y0:y0 + h, x0:x0 + w], full["gt_full"][b, :, y0:y0 + h, x0:x0 + w]
        if flip:
            x, g = x.flip(-1), g.flip(-1)
            x[4] = torch.where(x[4] == 0, x[4], -x[4])
        xs.append(x)
        gs.append(g)
    out = {"image": torch.stack(xs), "gt_full": torch.stack(gs)}
    cur = out["gt_full"]
    for name in ("gt_half", "gt_quarter", "gt_eighth")[:levels]:
        cur = synth.min_pool_ignore_zero(cur)
        out[name] = cur
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    B, H, W, h, w = 8, 416, 800, 256, 416
    g = torch.Generator(device="cuda").manual_seed(0)
    hit = torch.rand(B, H, W, device="cuda", generator=g) < 0.05
    raw = {"img": torch.randint(0, 256, (B, H, W, 3), device="cuda", generator=g, dtype=torch.uint8),
           "radar": torch.randn(B, H, W, 3, device="cuda", generator=g) * hit[..., None],
           "rv": (torch.rand(B, H, W, device="cuda", generator=g) < 0.5).float() * hit,
           "depth": torch.rand(B, H, W, device="cuda", generator=g) * 100.0 * (torch.rand(B, H, W, device="cuda", generator=g) < 0.05),
           "seg": torch.randint(0, 21, (B, H, W), device="cuda", generator=g, dtype=torch.uint8)}
    raw["radar"][..., 0] = raw["radar"][..., 0].abs() * 60.0
    aug = Augment(crop=(h, w), hflip=0.5, seed=1)
    jitter = Augment(crop=(h, w), hflip=0.5, gamma=(0.9, 1.1), brightness=(0.75, 1.25), colour=(0.9, 1.1), seed=1)
    params = aug.draw(B, H, W, counter=0)
    rows = [tuple(int(v) for v in r[:3]) for r in params.cpu().tolist()]
    print(f"device: {torch.cuda.get_device_name(0)}; {B} frames {H}x{W} -> {h}x{w}, offsets / flips {rows}", flush=True)
    fused = assemble_batch(raw["img"], raw["radar"], raw["rv"], raw["depth"], augment=aug, params=params)
    want = baseline(raw, rows, h, w)
    for k in want:
        assert torch.equal(fused[k], want[k]), k
    print("fused path == baseline on every tensor", flush=True)

    def run_fused():
        assemble_batch(raw["img"], raw["radar"], raw["rv"], raw["depth"], augment=aug)

    def run_jitter():
        assemble_batch(raw["img"], raw["radar"], raw["rv"], raw["depth"], augment=jitter)

    def run_labels():
        assemble_batch(raw["img"], raw["radar"], raw["rv"], raw["depth"], augment=aug, seg=raw["seg"])

    def run_baseline():
        baseline(raw, rows, h, w)

    lut = aug.lut(params)
    x, full = torch.empty(B, 7, h, w, device="cuda"), torch.empty(B, 1, h, w, device="cuda")
    L, st = lib.load(), lib.stream()

    def run_kernel():
        lib.check(L.crd_augment_assemble(raw["img"].data_ptr(), raw["radar"].data_ptr(), raw["rv"].data_ptr(), raw["depth"].data_ptr(), None,
                                         params.data_ptr(), lut.data_ptr(), B, H, W, h, w, 100.0, x.data_ptr(), full.data_ptr(), None, None,
                                         st), "crd_augment_assemble")

    nbytes = B * h * w * (3 + 12 + 4 + 4 + 7 * 4 + 4)
    for name, fn in (("baseline: assemble_batch + torch crop / flip + min_pool_ignore_zero", run_baseline),
                     ("fused: assemble_batch(augment=), draw included", run_fused),
                     ("fused with photometric jitter", run_jitter), ("fused with labels", run_labels)):
        us, lo, hi = timed(fn, a.reps, a.rounds)
        print(f"{name}: {us:7.1f} ({lo:7.1f} .. {hi:7.1f}) us per batch", flush=True)
    us, lo, hi = timed(run_kernel, a.reps, a.rounds)
    print(f"crd_augment_assemble alone: {us:6.1f} ({lo:6.1f} .. {hi:6.1f}) us | {nbytes / us / 1e3:6.0f} GB/s of {nbytes / 1e6:.1f} MB algorithmic "
          f"bytes (floor {nbytes / HBM_TBS / 1e6:.1f} us at {HBM_TBS} TB/s)", flush=True)


if __name__ == "__main__":
    main()
