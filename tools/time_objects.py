#!/usr/bin/env python3
"""Time the map objects (camradepth_amd.objects) on the scene, the windows and the drive of tools/time_occupancy.py -- the road scene
fused into an occupancy map of 80 m x 80 m of 0.5 m and of 0.2 m cells (160 x 160 and 400 x 400), 1 and 8 maps -- and on maps of the
same sizes with sources drawn on 1 % and on 41 % of the cells (41 %: the 8-connected percolation threshold, the largest and most
winding objects a density gives).  Every call is captured in a graph with its workspace and replayed: HIP events round a replay, 20
warm-up and 100 timed replays, the median microseconds of crd_map_objects (eight launches) with what it found, beside
crd_distance_field at max_cells 16 on the same state, captured and replayed the same way.  For context, where scipy imports,
scipy.ndimage.label + find_objects on the host over the same states: the copy down, the labelling, the boxes and the label map's
copy up (wall clock, 3 runs).

    python tools/time_objects.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_objects.py      # the per-launch split (k_obj_*)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import bev, cloud, field, objects, occupancy  # noqa: E402
from time_bev import CELLS, K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene, timed  # noqa: E402
from time_occupancy import CAMERA_HEIGHT, N_BINS, N_POSES  # noqa: E402

FIELD_R = 16
MAP_UPDATES = 121                                            # time_field.py's 20 warm-up and 100 timed updates and the one it keeps
MAX_OBJECTS = 4096


def replayed(fn, warmup, runs):
    """fn captured once on a side stream -> (median, min, max) microseconds of a replay."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return timed(g.replay, warmup, runs)


def host_label_us(state, runs=3):
    """Median microseconds of scipy.ndimage.label + find_objects over the states on the host, its copies included; None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    eight = ndimage.generate_binary_structure(2, 2)
    whole = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = state.cpu().numpy()
        labels = np.empty(s.shape, np.int32)
        for m in range(s.shape[0]):
            ndimage.label(s[m] == occupancy.OCCUPIED, structure=eight, output=labels[m])
            ndimage.find_objects(labels[m])
        torch.from_numpy(labels).cuda()
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e6)
    return sorted(whole)[runs // 2]


def measure(line, res, cell, a):
    """The objects of the maps res['state'] with the origins res['origin'] -> line, with its times."""
    M, nx, ny = res["state"].shape
    spec = objects.ObjectSpec(cell, max_objects=MAX_OBJECTS)
    ws = objects.ObjectWorkspace(spec, M, nx, ny)
    got = objects.map_objects(spec, res, res, workspace=ws)
    info = got["info"].tolist()
    line.update(map=[M, nx, ny], states_unknown_free_occupied=torch.bincount(res["state"].view(-1).long(), minlength=3).tolist(),
                objects=[r[0] for r in info], overflow=[r[1] for r in info], guard=[r[3] for r in info],
                largest_object_cells=int(got["objects"][:, :, 1].max()))
    med, lo, hi = replayed(lambda: objects.map_objects(spec, res, res, workspace=ws), a.warmup, a.runs)
    line.update(crd_map_objects_us_median=round(med, 2), crd_map_objects_us_min_max=[round(lo, 2), round(hi, 2)])
    no_centre = dict(ws.out, centre=None)
    med, lo, hi = replayed(lambda: objects.map_objects(spec, res, res, workspace=ws, out=no_centre), a.warmup, a.runs)
    line.update(crd_map_objects_without_centre_us_median=round(med, 2))
    fspec = field.FieldSpec(cell, max_cells=FIELD_R, inscribed=cell, scale=1.0)
    fws = field.FieldWorkspace(fspec, M, nx, ny)
    med, lo, hi = replayed(lambda: field.distance_field(fspec, res, workspace=fws, out=fws.out), a.warmup, a.runs)
    line.update(crd_distance_field_R16_us_median=round(med, 2))
    host = host_label_us(res["state"])
    if host is not None:
        line.update(scipy_label_find_objects_host_us_median=round(host, 1))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_objects: no GPU (a time measured anywhere else says nothing)")
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
            for turn in range(1, MAP_UPDATES + 1):                           # the map tools/time_field.py measures on
                res = occupancy.update(omap, pts, map_from_points=poses[turn % N_POSES], workspace=ows, out=ows.out)
            print(json.dumps(dict(measure({"shape": name, "cell_m": cell}, res, cell, a), runs=a.runs)), flush=True)
    for share in (0.01, 0.41):
        for M in (1, 8):
            for nx, ny in ((160, 160), (400, 400)):
                gen = torch.Generator(device="cuda").manual_seed(nx + M)
                state = torch.where(torch.rand(M, nx, ny, device="cuda", generator=gen) < share, occupancy.OCCUPIED, occupancy.FREE).to(torch.uint8)
                res = {"state": state, "origin": torch.zeros(M, 2, dtype=torch.int64, device="cuda")}
                line = {"shape": f"sources on {round(share * 100)} % of the cells", "cell_m": 0.5}
                print(json.dumps(dict(measure(line, res, 0.5, a), runs=a.runs)), flush=True)


if __name__ == "__main__":
    main()
