#!/usr/bin/env python3
"""Time the visualisation back end (camradepth_amd.viz) at the two shapes the project runs: 1 x 416 x 800 (a full frame) and
8 x 256 x 416 (a training batch).  HIP events, 20 warm-up and 100 timed calls, every call with workspace= and out=; per shape and
entry the median microseconds beside the call's algorithmic bytes and the bytes per second they make.  Algorithmic bytes per pixel:
crd_viz_range reads the map (4; labels 1); with the radar transform it also writes the dilated map (4 + 4); crd_viz_draw reads the
map (4; labels 1), the image where it has one (3) and writes the picture (3); crd_seg_labels reads C logits (4 C) and writes a label
(1).  The partials, the ranges and the 768-byte table are not in these floors.

    python tools/time_viz.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_viz.py          # the per-launch split (k_viz_*, k_seg_labels)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import viz  # noqa: E402

SHAPES = {"1x416x800": (1, 416, 800), "8x256x416": (8, 256, 416)}
CLASSES = 21


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_viz: no GPU (a time measured anywhere else says nothing)")
    for name, (B, h, w) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(5)
        depth = torch.rand(B, 1, h, w, device="cuda", generator=g)
        radar = torch.rand(B, h, w, device="cuda", generator=g) * (torch.rand(B, h, w, device="cuda", generator=g) < 0.002)
        image = torch.randint(0, 256, (B, h, w, 3), device="cuda", generator=g, dtype=torch.uint8)
        logits = torch.randn(B, CLASSES, h, w, device="cuda", generator=g)
        labels = torch.randint(0, CLASSES, (B, h, w), device="cuda", generator=g, dtype=torch.uint8)
        x = torch.zeros(B, 7, h, w, device="cuda")
        x[:, 3] = radar
        ws = viz.VizWorkspace(B, h, w)
        out = torch.empty(B, h, w, 3, dtype=torch.uint8, device="cuda")
        lab_out = torch.empty(B, h, w, dtype=torch.uint8, device="cuda")
        rng = viz.frame_range(depth).clone()
        vz = viz.Visualizer(B, h, w)
        pred = {"depth": {"final_depth": depth}, "seg": {"final_seg": logits, "unsup_map": None}}
        n = B * h * w
        calls = {
            "crd_viz_range (float)": (lambda: viz.frame_range(depth, workspace=ws), 4 * n),
            "crd_viz_range (labels)": (lambda: viz.frame_range(labels, workspace=ws), n),
            "crd_viz_draw (colorize, fixed range)": (lambda: viz.colorize(depth, vmin=rng, out=out, workspace=ws), 7 * n),
            "crd_viz_draw (labels, fixed range)": (lambda: viz.colorize_labels(labels, vmin=rng, out=out, workspace=ws), 4 * n),
            "crd_viz_draw (blend, fixed range)": (lambda: viz.overlay(image, depth, "blend", vmin=rng, out=out, workspace=ws), 10 * n),
            "colorize = range + draw": (lambda: viz.colorize(depth, out=out, workspace=ws), 11 * n),
            "overlay paste = range + draw": (lambda: viz.overlay(image, depth, "paste", out=out, workspace=ws), 14 * n),
            "radar_overlay = range (dilate 5) + draw": (lambda: viz.radar_overlay(image, radar, out=out, workspace=ws), 18 * n),
            "crd_seg_labels (C 21)": (lambda: viz.seg_labels(logits, out=lab_out), (4 * CLASSES + 1) * n),
            "Visualizer.render (all panels)": (lambda: vz.render(image, x, pred, gt_full=depth, seg=labels), None),
        }
        for entry, (fn, nbytes) in calls.items():
            med, lo, hi = timed(fn, a.warmup, a.runs)
            print(json.dumps({"shape": name, "entry": entry, "pixels": n, "us_median": round(med, 2), "us_min_max": [round(lo, 2), round(hi, 2)],
                              "algorithmic_bytes": nbytes, "GB_per_s": None if nbytes is None else round(nbytes / med * 1e-3, 1), "runs": a.runs}))


if __name__ == "__main__":
    main()
