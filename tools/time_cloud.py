#!/usr/bin/env python3
"""Time the point-cloud back end (camradepth_amd.cloud) at the two shapes the project runs: 1 x 416 x 800 (a full frame) and
8 x 256 x 416 (a training batch), inverse depth with about half of the pixels masked out, one out_from_cam per frame.  HIP events,
20 warm-up and 100 timed calls; per shape and entry the median microseconds beside the call's algorithmic bytes and the bytes per
second they make.  Algorithmic bytes: crd_depth_unproject reads depth (4) and mask (1) and writes points (12) and valid (1) per pixel;
crd_point_cloud reads depth and mask once per candidate and writes xyz (12) per point and frame_offsets -- its second read of depth
and mask in the scatter launch and the tile counts are not in that floor.

    python tools/time_cloud.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_cloud.py        # the per-launch split (k_cloud_*)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import cloud  # noqa: E402

SHAPES = {"1x416x800": (1, (900, 1600), 2, 34), "8x256x416": (8, (512, 832), 2, 0)}


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
        raise SystemExit("time_cloud: no GPU (a time measured anywhere else says nothing)")
    for name, (B, size, s, cut) in SHAPES.items():
        h, w = cloud.map_shape(size, s, cut)
        g = torch.Generator(device="cuda").manual_seed(5)
        depth = torch.rand(B, 1, h, w, device="cuda", generator=g)
        mask = (torch.rand(B, h, w, device="cuda", generator=g) < 0.5).to(torch.uint8)
        K = torch.tensor([[1266.4, 0.0, 816.3], [0.0, 1270.9, 491.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
        T = torch.eye(4, dtype=torch.float64, device="cuda")[:3].expand(B, 3, 4).contiguous()
        ws = cloud.CloudWorkspace(B, size, s, cut)
        grid = {"points": torch.empty(B, h, w, 3, device="cuda"), "valid": torch.empty(B, h, w, dtype=torch.uint8, device="cuda")}
        kw = dict(image_size=size, downsample_scale=s, y_cutoff=cut, out_from_cam=T, mask=mask)
        n_pix = B * h * w
        n = int(cloud.point_cloud(depth, K, workspace=ws, out=ws.out, **kw)["frame_offsets"][-1])
        assert n == int(cloud.unproject_depth(depth, K, out=grid, **kw)["valid"].sum())
        calls = {"crd_depth_unproject": (lambda: cloud.unproject_depth(depth, K, out=grid, **kw), 17 * n_pix),
                 "crd_point_cloud": (lambda: cloud.point_cloud(depth, K, workspace=ws, out=ws.out, **kw), 5 * n_pix + 12 * n + 4 * (B + 1))}
        for entry, (fn, nbytes) in calls.items():
            med, lo, hi = timed(fn, a.warmup, a.runs)
            print(json.dumps({"shape": name, "entry": entry, "pixels": n_pix, "valid_share": round(n / n_pix, 4), "us_median": round(med, 2),
                              "us_min_max": [round(lo, 2), round(hi, 2)], "algorithmic_bytes": nbytes,
                              "GB_per_s": round(nbytes / med * 1e-3, 1), "runs": a.runs}))


if __name__ == "__main__":
    main()
