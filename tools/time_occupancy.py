#!/usr/bin/env python3
"""Time the occupancy map (camradepth_amd.occupancy) on the road scene of tools/time_bev.py -- a ground plane 1.5 m under the camera up
to walls at 10 .. 80 m -- driven straight ahead through 20 poses one metre apart: the compact cloud of 1 x 416 x 800 (a full frame) and
of 8 x 256 x 416 (a batch, one map per frame) into a window of 80 m x 80 m of 0.5 m and of 0.2 m cells, 720 bearing bins.  HIP events,
20 warm-up and 100 timed calls that go round the poses; per shape and cell size the median microseconds of crd_occupancy_update
(workspace= and out=, three launches) beside crd_bev_grid on the same cloud in the same process, which is the yardstick.

    python tools/time_occupancy.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_occupancy.py      # the per-launch split (k_occ_*, k_bev_*)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import bev, cloud, occupancy  # noqa: E402
from time_bev import CELLS, K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene, timed  # noqa: E402

N_POSES, N_BINS, CAMERA_HEIGHT = 20, 720, 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_occupancy: no GPU (a time measured anywhere else says nothing)")
    K = torch.tensor(K_FULL, dtype=torch.float64, device="cuda")
    poses = []
    for i in range(N_POSES):                         # the camera 1.5 m over the road of the map frame, one metre on per pose
        T = bev.CAM_TO_BEV.clone()
        T[0, 3], T[2, 3] = float(i), CAMERA_HEIGHT
        poses.append(T.cuda())
    for name, (B, size, s, cut) in SHAPES.items():
        h, w = cloud.map_shape(size, s, cut)
        g = torch.Generator(device="cuda").manual_seed(5)
        K_shape = K * torch.tensor([[size[1] / 1600.0], [size[0] / 900.0], [1.0]], dtype=torch.float64, device="cuda")
        pts = cloud.point_cloud(road_scene(B, h, w, s, cut, size, g), K_shape, image_size=size, downsample_scale=s, y_cutoff=cut)
        n = int(pts["frame_offsets"][-1])
        for cell in CELLS:
            nx, ny = bev.grid_shape(X_RANGE, Y_RANGE, cell)
            omap = occupancy.OccupancyMap(B, nx, ny, cell, n_bins=N_BINS, max_range=80.0, z_floor=-0.3, z_lo=0.3, z_hi=3.0)
            ws = occupancy.OccupancyWorkspace(omap, B)
            turn = [0]

            def update():
                turn[0] += 1
                return occupancy.update(omap, pts, map_from_points=poses[turn[0] % N_POSES], workspace=ws, out=ws.out)

            res = update()
            line = {"shape": name, "cell_m": cell, "map": [B, nx, ny], "bins": N_BINS, "points": n,
                    "evidence_unknown_free_occupied": torch.bincount(res["evidence"].view(-1).long(), minlength=3).tolist()}
            med, lo, hi = timed(update, a.warmup, a.runs)
            line.update(crd_occupancy_update_us_median=round(med, 2), crd_occupancy_update_us_min_max=[round(lo, 2), round(hi, 2)],
                        status=omap.status()[:1], states_unknown_free_occupied=torch.bincount(ws.out["state"].view(-1).long(), minlength=3).tolist())
            bws = bev.BevWorkspace(B, nx, ny)
            kw = dict(x_range=X_RANGE, y_range=Y_RANGE, cell=cell, grid_from_points=poses[0], workspace=bws, out=bws.out)
            med, lo, hi = timed(lambda: bev.bev_grid(pts, **kw), a.warmup, a.runs)
            line.update(crd_bev_grid_us_median=round(med, 2), crd_bev_grid_us_min_max=[round(lo, 2), round(hi, 2)])
            print(json.dumps(dict(line, runs=a.runs)), flush=True)


if __name__ == "__main__":
    main()
