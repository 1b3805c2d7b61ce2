#!/usr/bin/env python3
"""Time the bird's-eye-view back end (camradepth_amd.bev) on the compact cloud of the two shapes the project runs, 1 x 416 x 800 (a
full frame) and 8 x 256 x 416 (a training batch), into an 80 m x 80 m grid of 0.5 m and of 0.2 m cells.  The depth map is a road
scene -- a ground plane 1.5 m under the camera up to walls at 10 .. 80 m -- so the cloud has what a real one has: image rows that fall
into the same few cells near the camera.  HIP events, 20 warm-up and 100 timed calls; per shape and cell size the median microseconds
of crd_bev_grid (workspace= and out=, four launches) beside the equivalent torch chain in the same process: transform, floor, a mask,
scatter_reduce amax / amin and bincount -- which allocates, waits for the host and gives neither the winning row nor the same bits
every run.

    python tools/time_bev.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_bev.py --skip-torch      # the per-launch split (k_bev_*)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import bev, cloud  # noqa: E402

SHAPES = {"1x416x800": (1, (900, 1600), 2, 34), "8x256x416": (8, (512, 832), 2, 0)}
CELLS = (0.5, 0.2)
X_RANGE, Y_RANGE = (0.0, 80.0), (-40.0, 40.0)
K_FULL = [[1266.4, 0.0, 816.3], [0.0, 1270.9, 491.5], [0.0, 0.0, 1.0]]


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


def road_scene(B, h, w, s, cut, size, g):
    """Normalised inverse depth [B,1,h,w]: the ground 1.5 m under the camera, cut off by walls of 16 columns at 10 .. 80 m."""
    fy, cy = K_FULL[1][1] * size[0] / 900.0, K_FULL[1][2] * size[0] / 900.0
    yf = (torch.arange(h, device="cuda", dtype=torch.float64) + cut + 0.5) * s - 0.5
    ground = torch.where(yf > cy, 1.5 * fy / (yf - cy).clamp(min=1e-3), torch.full_like(yf, 1e9)).view(1, h, 1)
    wall = 10.0 + 70.0 * torch.rand(B, 1, -(-w // 16), device="cuda", generator=g, dtype=torch.float64).repeat_interleave(16, dim=2)[:, :, :w]
    metres = torch.minimum(ground.expand(B, h, w), wall.expand(B, h, w))
    return (1.0 - metres / 100.0).float().view(B, 1, h, w)


def torch_chain(xyz, off, n, B, T, cell, nx, ny):
    """What a user writes without the back end: the same grids (count, z_max, z_min) from torch operations."""
    p = xyz[:n].double()
    P = p @ T[:, :3].T + T[:, 3]
    b = torch.bucketize(torch.arange(n, device=xyz.device, dtype=torch.int32), off[1:], right=True)
    qx, qy = torch.floor((P[:, 0] - X_RANGE[0]) / cell), torch.floor((P[:, 1] - Y_RANGE[0]) / cell)
    keep = torch.isfinite(P).all(dim=1) & (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
    at = ((b * nx + qx.long()) * ny + qy.long())[keep]
    z = P[:, 2][keep].float()
    cells = B * nx * ny
    z_max = torch.full((cells,), float("-inf"), device=xyz.device).scatter_reduce(0, at, z, "amax")
    z_min = torch.full((cells,), float("inf"), device=xyz.device).scatter_reduce(0, at, z, "amin")
    return torch.bincount(at, minlength=cells), z_max, z_min


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--skip-torch", action="store_true", help="crd_bev_grid alone, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bev: no GPU (a time measured anywhere else says nothing)")
    T = bev.CAM_TO_BEV.cuda()
    K = torch.tensor(K_FULL, dtype=torch.float64, device="cuda")
    for name, (B, size, s, cut) in SHAPES.items():
        h, w = cloud.map_shape(size, s, cut)
        g = torch.Generator(device="cuda").manual_seed(5)
        K_shape = K * torch.tensor([[size[1] / 1600.0], [size[0] / 900.0], [1.0]], dtype=torch.float64, device="cuda")
        pts = cloud.point_cloud(road_scene(B, h, w, s, cut, size, g), K_shape, image_size=size, downsample_scale=s, y_cutoff=cut)
        n = int(pts["frame_offsets"][-1])
        for cell in CELLS:
            nx, ny = bev.grid_shape(X_RANGE, Y_RANGE, cell)
            ws = bev.BevWorkspace(B, nx, ny)
            kw = dict(x_range=X_RANGE, y_range=Y_RANGE, cell=cell, grid_from_points=T, workspace=ws, out=ws.out)
            grid = bev.bev_grid(pts, **kw)
            line = {"shape": name, "cell_m": cell, "grid": [B, nx, ny], "points": n, "points_in_grid": int(grid["count"].sum()),
                    "cells_occupied": int((grid["count"] > 0).sum()), "max_points_in_a_cell": int(grid["count"].max())}
            med, lo, hi = timed(lambda: bev.bev_grid(pts, **kw), a.warmup, a.runs)
            line.update(crd_bev_grid_us_median=round(med, 2), crd_bev_grid_us_min_max=[round(lo, 2), round(hi, 2)])
            if not a.skip_torch:
                count, z_max, z_min = torch_chain(pts["xyz"], pts["frame_offsets"], n, B, T, cell, nx, ny)
                same = grid["count"].view(-1) > 0
                line["torch_chain_agrees"] = bool(torch.equal(count.int(), grid["count"].view(-1)) and
                                                  torch.equal(z_max[same], grid["z_max"].view(-1)[same]) and
                                                  torch.equal(z_min[same], grid["z_min"].view(-1)[same]))
                med, lo, hi = timed(lambda: torch_chain(pts["xyz"], pts["frame_offsets"], n, B, T, cell, nx, ny), a.warmup, a.runs)
                line.update(torch_chain_us_median=round(med, 2), torch_chain_us_min_max=[round(lo, 2), round(hi, 2)])
            print(json.dumps(dict(line, runs=a.runs)), flush=True)


if __name__ == "__main__":
    main()
