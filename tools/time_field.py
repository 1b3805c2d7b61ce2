#!/usr/bin/env python3
"""Time the distance field (camradepth_amd.field) on the scene, the windows and the drive of tools/time_occupancy.py: the road scene
fused into an occupancy map of 80 m x 80 m of 0.5 m and of 0.2 m cells, B = 1 and B = 8 maps, then the field of its `state`.  HIP
events, 20 warm-up and 100 timed calls; per shape and cell size the median microseconds of crd_distance_field (workspace= and out=,
two launches) at max_cells 16, 64 and 255 and of crd_field_paths (64 paths of 128 poses) beside crd_occupancy_update on the same
window in the same process, which is the yardstick.  For context, where scipy imports, scipy.ndimage.distance_transform_edt of the
same state on the host, the copy down and the result's copy up included (wall clock, 5 runs).

    python tools/time_field.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_field.py      # the per-launch split (k_field_*, k_occ_*)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import bev, cloud, field, occupancy  # noqa: E402
from time_bev import CELLS, K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene, timed  # noqa: E402
from time_occupancy import CAMERA_HEIGHT, N_BINS, N_POSES  # noqa: E402

RADII = (16, 64, 255)
N_PATHS, N_PATH_POSES = 64, 128


def host_edt_us(state, runs=5):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        src = (state == occupancy.OCCUPIED).cpu().numpy()
        d = [ndimage.distance_transform_edt(~m) for m in src]
        torch.from_numpy(d[0]).cuda()
        for m in d[1:]:
            torch.from_numpy(m).cuda()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_field: no GPU (a time measured anywhere else says nothing)")
    K = torch.tensor(K_FULL, dtype=torch.float64, device="cuda")
    poses = []
    for i in range(N_POSES):
        T = bev.CAM_TO_BEV.clone()
        T[0, 3], T[2, 3] = float(i), CAMERA_HEIGHT
        poses.append(T.cuda())
    for name, (B, size, s, cut) in SHAPES.items():
        h, w = cloud.map_shape(size, s, cut)
        g = torch.Generator(device="cuda").manual_seed(5)
        K_shape = K * torch.tensor([[size[1] / 1600.0], [size[0] / 900.0], [1.0]], dtype=torch.float64, device="cuda")
        pts = cloud.point_cloud(road_scene(B, h, w, s, cut, size, g), K_shape, image_size=size, downsample_scale=s, y_cutoff=cut)
        for cell in CELLS:
            nx, ny = bev.grid_shape(X_RANGE, Y_RANGE, cell)
            omap = occupancy.OccupancyMap(B, nx, ny, cell, n_bins=N_BINS, max_range=80.0, z_floor=-0.3, z_lo=0.3, z_hi=3.0)
            ows = occupancy.OccupancyWorkspace(omap, B)
            turn = [0]

            def update():
                turn[0] += 1
                return occupancy.update(omap, pts, map_from_points=poses[turn[0] % N_POSES], workspace=ows, out=ows.out)

            med, lo, hi = timed(update, a.warmup, a.runs)
            res = update()
            line = {"shape": name, "cell_m": cell, "map": [B, nx, ny],
                    "states_unknown_free_occupied": torch.bincount(res["state"].view(-1).long(), minlength=3).tolist(),
                    "crd_occupancy_update_us_median": round(med, 2), "crd_occupancy_update_us_min_max": [round(lo, 2), round(hi, 2)]}
            for R in RADII:
                spec = field.FieldSpec(cell, max_cells=R)
                ws = field.FieldWorkspace(spec, B, nx, ny)
                f = field.distance_field(spec, res, workspace=ws, out=ws.out)
                line[f"far_share_R{R}"] = round(float((f["dist2"] == spec.far).float().mean()), 3)
                med, lo, hi = timed(lambda: field.distance_field(spec, res, workspace=ws, out=ws.out), a.warmup, a.runs)
                line[f"crd_distance_field_R{R}_us_median"] = round(med, 2)
                line[f"crd_distance_field_R{R}_us_min_max"] = [round(lo, 2), round(hi, 2)]
            gen = torch.Generator(device="cuda").manual_seed(9)                   # trajectories over the window and a little beyond it
            span = torch.tensor([nx * cell * 1.1, ny * cell * 1.1], dtype=torch.float64, device="cuda")
            low = res["origin"][0].double() * cell - 0.05 * span
            xy = low + torch.rand(N_PATHS, N_PATH_POSES, 2, dtype=torch.float64, device="cuda", generator=gen) * span
            path_map = (torch.arange(N_PATHS, device="cuda") % B).int()
            pout = field.path_outputs(N_PATHS, N_PATH_POSES)
            check = lambda: field.check_paths(spec, f, res, xy, path_map=path_map, out=pout)      # noqa: E731
            got = check()
            line["paths_blocked_outside"] = [int((got["first_blocked"] >= 0).sum()), int(got["n_outside"].sum())]
            med, lo, hi = timed(check, a.warmup, a.runs)
            line.update(crd_field_paths_us_median=round(med, 2), crd_field_paths_us_min_max=[round(lo, 2), round(hi, 2)])
            edt = host_edt_us(res["state"])
            if edt is not None:
                line["scipy_edt_host_us_median"] = round(edt, 1)
            print(json.dumps(dict(line, runs=a.runs)), flush=True)


if __name__ == "__main__":
    main()
