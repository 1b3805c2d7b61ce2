#!/usr/bin/env python3
"""Time the navigation field (camradepth_amd.nav) on the scene, the windows and the drive of tools/time_occupancy.py: the road scene fused
into an occupancy map of 80 m x 80 m of 0.5 m and of 0.2 m cells (160 x 160 and 400 x 400), B = 1 and B = 8 maps, the distance field's
costmap of its `state` (max_cells 16, inscribed one cell, scale 1), then the cost-to-go towards one goal per map, three quarters of
the window ahead, and 64 planned paths of at most 512 cells; and the same on one cluttered map of each size, obstacles drawn on 1 % of
its cells, whose paths turn more often, so that the sweep needs more rounds.  HIP events, 20 warm-up and 100 timed calls; per shape and cell size the median microseconds of
crd_nav_field (workspace=: three launches) with the rounds every map needed, of crd_nav_field without the direction map, and of
crd_nav_paths, beside crd_distance_field on the same window in the same process.  For context, where scipy imports,
scipy.sparse.csgraph.dijkstra on the host over the same costmaps: the copy down, the graph, the search and the result's copy up (wall
clock, 3 runs), and the search alone.

    python tools/time_nav.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_nav.py        # the per-launch split (k_nav_*)
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
from camradepth_amd import bev, cloud, field, nav, occupancy  # noqa: E402
from time_bev import CELLS, K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene, timed  # noqa: E402
from time_occupancy import CAMERA_HEIGHT, N_BINS, N_POSES  # noqa: E402

FIELD_R = 16
MAP_UPDATES = 121                                            # time_field.py's 20 warm-up and 100 timed updates and the one it keeps
N_PATHS, MAX_PATH_CELLS = 64, 512
GOAL_AHEAD = 0.75                                            # the goal: the passable cell nearest to this share of the window's rows, mid column


def host_dijkstra_us(cost, goal_cells, spec, runs=3):
    """(whole, search alone) median microseconds of scipy's Dijkstra over the costmaps on the host, or None without scipy."""
    try:
        from scipy import sparse
        from scipy.sparse import csgraph
    except ImportError:
        return None
    M, nx, ny = cost.shape
    idx = np.arange(nx * ny).reshape(nx, ny)
    whole, search = [], []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = cost.cpu().numpy()
        spent = 0.0
        for m in range(M):
            ok = c[m] < spec.blocked_at
            w = (spec.neutral + c[m].astype(np.int64)).astype(np.float64)
            rows, cols, vals = [], [], []
            for (di, dj) in nav.NEIGHBOURS:                  # the edge b -> a for every move a -> b = a + (di, dj)
                a = (slice(max(0, -di), nx - max(0, di)), slice(max(0, -dj), ny - max(0, dj)))
                b = (slice(max(0, di), nx - max(0, -di)), slice(max(0, dj), ny - max(0, -dj)))
                both = ok[a] & ok[b]
                rows.append(idx[b][both]), cols.append(idx[a][both]), vals.append((7.0 if di and dj else 5.0) * w[a][both])
            graph = sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny, nx * ny))
            t1 = time.perf_counter()
            dist = csgraph.dijkstra(graph, directed=True, indices=[goal_cells[m]], min_only=True)
            spent += time.perf_counter() - t1
            torch.from_numpy(np.where(np.isfinite(dist), dist, nav.UNREACHED).astype(np.int32)).cuda()
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e6)
        search.append(spent * 1e6)
    return sorted(whole)[runs // 2], sorted(search)[runs // 2]


def measure(line, f, res, B, nx, ny, cell, a):
    """The navigation field of the costmap f['cost'] of B maps with the origins res['origin'] -> line, with its times."""
    spec = nav.NavSpec(cell)
    cost_host, origin_host = f["cost"].cpu().numpy(), res["origin"].cpu().numpy()
    goal_cells, goals = [], []
    for m in range(B):                               # set-up on the host, not timed
        ii, jj = np.nonzero(cost_host[m] < spec.blocked_at)
        k = int(np.argmin((ii - int(GOAL_AHEAD * nx)) ** 2 + (jj - ny // 2) ** 2))
        goal_cells.append(int(ii[k]) * ny + int(jj[k]))
        goals.append([((origin_host[m, 0] + ii[k] + 0.5) * cell, (origin_host[m, 1] + jj[k] + 0.5) * cell)])
    goals = torch.tensor(goals, dtype=torch.float64, device="cuda")
    ws = nav.NavWorkspace(spec, B, nx, ny)
    got = nav.nav_field(spec, f, res, goals, workspace=ws)
    info = got["info"].tolist()
    line.update(passable_share=round(float((f["cost"] < spec.blocked_at).float().mean()), 4),
                reached_share=round(float((got["togo"] != nav.UNREACHED).float().mean()), 4),
                converged=[r[0] for r in info], rounds=[r[1] for r in info], goals_used=[r[2] for r in info])
    med, lo, hi = timed(lambda: nav.nav_field(spec, f, res, goals, workspace=ws), a.warmup, a.runs)
    line.update(crd_nav_field_us_median=round(med, 2), crd_nav_field_us_min_max=[round(lo, 2), round(hi, 2)])
    togo_only = dict(ws.out, next=None)
    med, lo, hi = timed(lambda: nav.nav_field(spec, f, res, goals, out=togo_only), a.warmup, a.runs)
    line.update(crd_nav_field_without_next_us_median=round(med, 2))
    gen = torch.Generator(device="cuda").manual_seed(9)                   # starts all over the window
    span = torch.tensor([nx * cell, ny * cell], dtype=torch.float64, device="cuda")
    starts = res["origin"][0].double() * cell + torch.rand(N_PATHS, 2, dtype=torch.float64, device="cuda", generator=gen) * span
    path_map = (torch.arange(N_PATHS, device="cuda") % B).int()
    pout = nav.path_outputs(N_PATHS, MAX_PATH_CELLS)
    plan = lambda: nav.plan_paths(spec, got, res, starts, MAX_PATH_CELLS, path_map, out=pout)     # noqa: E731
    paths = plan()
    line["path_status_counts_0_1_2_3"] = torch.bincount(paths["status"].long(), minlength=4).tolist()
    line["path_cells_max_mean"] = [int(paths["n_cells"].max()), round(float(paths["n_cells"].float().mean()), 1)]
    med, lo, hi = timed(plan, a.warmup, a.runs)
    line.update(crd_nav_paths_us_median=round(med, 2), crd_nav_paths_us_min_max=[round(lo, 2), round(hi, 2)])
    host = host_dijkstra_us(f["cost"], goal_cells, spec)
    if host is not None:
        line.update(scipy_dijkstra_host_us_median=round(host[0], 1), scipy_dijkstra_search_alone_us_median=round(host[1], 1))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nav: no GPU (a time measured anywhere else says nothing)")
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
            fspec = field.FieldSpec(cell, max_cells=FIELD_R, inscribed=cell, scale=1.0)
            fws = field.FieldWorkspace(fspec, B, nx, ny)
            f = field.distance_field(fspec, res, workspace=fws, out=fws.out)
            med, lo, hi = timed(lambda: field.distance_field(fspec, res, workspace=fws, out=fws.out), a.warmup, a.runs)
            line = {"shape": name, "cell_m": cell, "map": [B, nx, ny],
                    "states_unknown_free_occupied": torch.bincount(res["state"].view(-1).long(), minlength=3).tolist(),
                    "crd_distance_field_R16_us_median": round(med, 2)}
            measure(line, f, res, B, nx, ny, cell, a)
            print(json.dumps(dict(line, runs=a.runs)), flush=True)
    # the road scene's map is nearly empty, so its paths hardly turn; a cluttered one: obstacles on 1 % of the cells, inflated
    for nx, ny in ((160, 160), (400, 400)):
        cell, gen = 0.5, torch.Generator(device="cuda").manual_seed(nx)
        state = torch.where(torch.rand(1, nx, ny, device="cuda", generator=gen) < 0.01, occupancy.OCCUPIED, occupancy.FREE).to(torch.uint8)
        res = {"state": state, "origin": torch.zeros(1, 2, dtype=torch.int64, device="cuda")}
        fspec = field.FieldSpec(cell, max_cells=FIELD_R, inscribed=cell, scale=1.0)
        f = field.distance_field(fspec, res)
        line = {"shape": "obstacles on 1 % of the cells", "cell_m": cell, "map": [1, nx, ny],
                "states_unknown_free_occupied": torch.bincount(state.view(-1).long(), minlength=3).tolist()}
        print(json.dumps(dict(measure(line, f, res, 1, nx, ny, cell, a), runs=a.runs)), flush=True)


if __name__ == "__main__":
    main()
