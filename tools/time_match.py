#!/usr/bin/env python3
"""Time the scan matcher (camradepth_amd.match) on the drive of tools/time_occupancy.py -- the road scene of tools/time_bev.py fused
through 20 poses one metre apart -- for 1 map of a full frame and 8 maps of a batch, windows of 80 m x 80 m of 0.5 m (160 x 160) and
0.2 m cells (400 x 400) and search windows (n_xy, n_theta) = (4, 4), (8, 10) and (16, 32), turns of 0.25 degrees.  The map is built
with the true poses; the prior of the timed match is the last pose moved back by one cell along x, which the pick has to undo.  Every
call is captured in a graph with its workspace and replayed: HIP events round a replay, 20 warm-up and 100 timed replays, the median
microseconds of crd_match_scan (four launches) beside crd_occupancy_update on the same cloud and window (three launches, on a map of
its own), and beside the NumPy restatement tests/match_ref.py on the host with its copies down (wall clock, one run).

    python tools/time_match.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_match.py --no-host      # the per-launch split (k_match_*, k_occ_*)
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import bev, cloud, match, occupancy  # noqa: E402
from time_bev import CELLS, K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene  # noqa: E402
from time_objects import replayed  # noqa: E402
from time_occupancy import CAMERA_HEIGHT, N_BINS, N_POSES  # noqa: E402

WINDOWS = ((4, 4), (8, 10), (16, 32))
D_THETA = math.radians(0.25)
MAP = dict(n_bins=N_BINS, max_range=80.0, z_floor=-0.3, z_lo=0.3, z_hi=3.0)


def host_match_us(omap, spec, pts, prior):
    """Wall-clock microseconds of tests/match_ref.match_scan on the host: the cloud, the prior and the map copied down, the restatement."""
    from tests import match_ref
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    params = dict(M=omap.M, nx=omap.nx, ny=omap.ny, cell=omap.cell, max_range=omap.max_range, z_lo=omap.z_lo, z_hi=omap.z_hi, min_points=omap.min_points)
    state = {"map": omap.log_odds.cpu().numpy(), "cur_origin": omap.cur_origin.cpu().numpy(), "initialised": omap.initialised.cpu().numpy()}
    numbers = dict(n_xy=spec.n_xy, n_theta=spec.n_theta, d_theta=spec.d_theta, min_points=spec.min_points, min_cells=spec.min_cells, min_score=spec.min_score)
    out = match_ref.match_scan(params, state, numbers, pts["xyz"].cpu().numpy(), omap.M if omap.M > 1 else 1,
                               frame_offsets=pts["frame_offsets"].cpu().numpy(), T=prior.cpu().numpy())
    return (time.perf_counter() - t0) * 1e6, out["pick"].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="leave the NumPy restatement on the host out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_match: no GPU (a time measured anywhere else says nothing)")
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
            omap, other = (occupancy.OccupancyMap(B, nx, ny, cell, **MAP) for _ in range(2))
            ows = occupancy.OccupancyWorkspace(omap, B)
            for T in poses:
                occupancy.update(omap, pts, map_from_points=T, workspace=ows, out=ows.out)
                occupancy.update(other, pts, map_from_points=T, workspace=ows, out=ows.out)
            prior = poses[-1].clone()
            prior[0, 3] -= cell
            med, lo, hi = replayed(lambda: occupancy.update(other, pts, map_from_points=poses[-1], workspace=ows, out=ows.out), a.warmup, a.runs)
            update_us = [round(med, 2), round(lo, 2), round(hi, 2)]
            for n_xy, n_theta in WINDOWS:
                spec = match.MatchSpec(n_xy=n_xy, n_theta=n_theta, d_theta=D_THETA)
                ws = match.MatchWorkspace(omap, spec, B)
                med, lo, hi = replayed(lambda: match.match_scan(omap, spec, pts, map_from_points=prior, workspace=ws), a.warmup, a.runs)
                line = {"shape": name, "cell_m": cell, "map": [B, nx, ny], "points": n, "n_xy": n_xy, "n_theta": n_theta,
                        "candidates": (2 * n_theta + 1) * (2 * n_xy + 1) ** 2, "workspace_MiB": round(ws.buf.numel() / 2 ** 20, 1),
                        "crd_match_scan_us_median": round(med, 2), "crd_match_scan_us_min_max": [round(lo, 2), round(hi, 2)],
                        "crd_occupancy_update_us_median_min_max": update_us, "pick": ws.out["pick"][:2].tolist(),
                        "status": ws.out["status"][:2].tolist(), "n_cells": ws.out["n_cells"][:2].tolist(),
                        "score_prior_score": [ws.out["score"][:2].tolist(), ws.out["prior_score"][:2].tolist()]}
                if not a.no_host:
                    us, pick = host_match_us(omap, spec, pts, prior)
                    line.update(host_numpy_us=round(us, 0), host_pick_equal=pick[:2] == line["pick"])
                print(json.dumps(dict(line, runs=a.runs)), flush=True)
                del ws


if __name__ == "__main__":
    main()
