#!/usr/bin/env python3
"""Time the terrain map (camradepth_amd.terrain) on the clouds of tools/time_occupancy.py -- the road scene of tools/time_bev.py, a
ground plane 1.5 m under the camera up to walls at 10 .. 80 m, driven straight ahead through 20 poses one metre apart: the compact
cloud of 1 x 416 x 800 (a full frame, one map) and of 8 x 256 x 416 (a batch, one map per frame) into a window of 80 m x 80 m of 0.5 m
(160 x 160) and of 0.2 m (400 x 400) cells.  Each entry is captured once in a graph with workspace= and out= and a pose buffer that
is refilled between replays; HIP events around every replay, 20 warm-up and 100 timed replays that go round the poses; per shape and
cell size the median microseconds of crd_terrain_update (five launches) beside crd_occupancy_update (three launches) on the same
cloud in the same process, which is the yardstick, and their ratio.

    python tools/time_terrain.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_terrain.py --eager --shape 8x256x416 --cell 0.2
                                                                 # the per-launch split (k_ter_*, k_occ_*) of one shape and cell size
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import bev, cloud, occupancy, terrain  # noqa: E402
from time_bev import CELLS, K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene  # noqa: E402

N_POSES, N_BINS, CAMERA_HEIGHT = 20, 720, 1.5


def timed(call, poses, pose, warmup, runs, eager):
    """call() reads the pose buffer `pose`; -> median, min, max microseconds of one call (a graph replay unless eager)."""
    pose.copy_(poses[0])
    call()                                                   # loads the code objects before the capture
    torch.cuda.synchronize()
    run = call
    if not eager:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        run = g.replay
    for i in range(warmup):
        pose.copy_(poses[i % N_POSES])
        run()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for i, (a, b) in enumerate(ev):
        pose.copy_(poses[i % N_POSES])
        a.record()
        run()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--eager", action="store_true", help="plain calls in place of graph replays, for a kernel trace")
    ap.add_argument("--shape", choices=list(SHAPES), help="this shape alone")
    ap.add_argument("--cell", type=float, choices=list(CELLS), help="this cell size alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_terrain: no GPU (a time measured anywhere else says nothing)")
    K = torch.tensor(K_FULL, dtype=torch.float64, device="cuda")
    poses = []
    for i in range(N_POSES):                         # the camera 1.5 m over the road of the map frame, one metre on per pose
        T = bev.CAM_TO_BEV.clone()
        T[0, 3], T[2, 3] = float(i), CAMERA_HEIGHT
        poses.append(T.cuda())
    pose = poses[0].clone()
    for name, (B, size, s, cut) in SHAPES.items():
        if a.shape not in (None, name):
            continue
        h, w = cloud.map_shape(size, s, cut)
        g = torch.Generator(device="cuda").manual_seed(5)
        K_shape = K * torch.tensor([[size[1] / 1600.0], [size[0] / 900.0], [1.0]], dtype=torch.float64, device="cuda")
        pts = cloud.point_cloud(road_scene(B, h, w, s, cut, size, g), K_shape, image_size=size, downsample_scale=s, y_cutoff=cut)
        n = int(pts["frame_offsets"][-1])
        for cell in CELLS:
            if a.cell not in (None, cell):
                continue
            nx, ny = bev.grid_shape(X_RANGE, Y_RANGE, cell)
            tmap = terrain.TerrainMap(B, nx, ny, cell)
            tws = terrain.TerrainWorkspace(tmap, B)
            omap = occupancy.OccupancyMap(B, nx, ny, cell, n_bins=N_BINS, max_range=80.0, z_floor=-0.3, z_lo=0.3, z_hi=3.0)
            ows = occupancy.OccupancyWorkspace(omap, B)
            line = {"shape": name, "cell_m": cell, "map": [B, nx, ny], "points": n, "replays": not a.eager}
            med, lo, hi = timed(lambda: terrain.update(tmap, pts, map_from_points=pose, workspace=tws, out=tws.out), poses, pose, a.warmup,
                                a.runs, a.eager)
            ter_us = med
            line.update(crd_terrain_update_us_median=round(med, 2), crd_terrain_update_us_min_max=[round(lo, 2), round(hi, 2)],
                        status=tmap.status()[:1], states_unknown_free_occupied=torch.bincount(tws.out["state"].view(-1).long(), minlength=3).tolist(),
                        cells_observed=int(tws.out["evidence"].sum()), max_rows_in_a_cell=int(tws.cells[2 * ((4 * B * nx * ny + 15) & ~15):][
                            :4 * B * nx * ny].view(torch.int32).max()))
            med, lo, hi = timed(lambda: occupancy.update(omap, pts, map_from_points=pose, workspace=ows, out=ows.out), poses, pose, a.warmup,
                                a.runs, a.eager)
            line.update(crd_occupancy_update_us_median=round(med, 2), crd_occupancy_update_us_min_max=[round(lo, 2), round(hi, 2)],
                        ratio=round(ter_us / med, 2))
            print(json.dumps(dict(line, runs=a.runs)), flush=True)


if __name__ == "__main__":
    main()
