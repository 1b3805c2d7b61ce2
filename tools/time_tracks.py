#!/usr/bin/env python3
"""Time the object tracks (camradepth_amd.tracks) on the object tables of the states tools/time_objects.py measures on -- the road scene
fused into an occupancy map of 80 m x 80 m of 0.5 m and of 0.2 m cells, 1 and 8 maps, and maps of 160 x 160 and 400 x 400 cells with
sources drawn on 1 % and on 41 % of the cells -- with max_objects = max_tracks = 256 and 1024.  Every call is captured in a graph with
its workspace and replayed: HIP events round a replay, 20 warm-up and 100 timed replays, the median microseconds of
  crd_track_objects in the steady state: the same table every replay, so every track finds its object again (one launch);
  crd_track_objects with the first half of the table only, on tracks of every row that never drop: half the tracks find nothing and
  are still open in the second round;
  ObjectTracks.reset() and crd_track_objects behind it: every row is born (the fills of reset() alone are timed beside it);
  crd_map_objects on the same state (eight launches), which makes the table.
For context the same assignment on the host: the table and the tracks copied down, the distance matrix in NumPy, the pairs within the
gate sorted, the greedy loop, the matched tracks moved, the results copied up (wall clock, 3 runs; births and drops left out).

    python tools/time_tracks.py
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
from camradepth_amd import bev, cloud, objects, occupancy, tracks  # noqa: E402
from time_bev import CELLS, K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene  # noqa: E402
from time_objects import MAP_UPDATES, replayed  # noqa: E402
from time_occupancy import CAMERA_HEIGHT, N_BINS, N_POSES  # noqa: E402

CAPS = (256, 1024)                                           # max_objects = max_tracks


def host_tracks_us(spec, held, table, origin, runs=3):
    """Median microseconds of the assignment on the host over the live tracks and the table's rows, its copies included."""
    whole = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        centre, info = table["centre"].cpu().numpy(), table["info"].cpu().numpy()
        table["objects"].cpu(), origin.cpu()
        status, pos, vel = held.tracks[..., 0].cpu().numpy(), held.pos.cpu().numpy(), held.vel.cpu().numpy()
        held.ids.cpu()
        M, N = centre.shape[:2]
        track_of = np.full((M, N), -1, np.int32)
        for m in range(M):
            pred = pos[m] + vel[m]
            live = status[m] != 0
            rows = (np.arange(N) < info[m, 0]) & np.isfinite(centre[m]).all(axis=1)
            d = centre[m][None, :, :] - pred[:, None, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
            with np.errstate(invalid="ignore"):
                t, k = np.nonzero((d2 <= spec.gate * spec.gate) & live[:, None] & rows[None, :])
            order = np.lexsort((k, t, d2[t, k]))
            taken_t, taken_k = np.zeros(len(live), bool), np.zeros(N, bool)
            for e in order:
                if not taken_t[t[e]] and not taken_k[k[e]]:
                    taken_t[t[e]] = taken_k[k[e]] = True
                    track_of[m, k[e]] = t[e]
            kk = np.flatnonzero(track_of[m] >= 0)
            r = centre[m, kk] - pred[track_of[m, kk]]
            pos[m, track_of[m, kk]] = pred[track_of[m, kk]] + spec.alpha * r
            vel[m, track_of[m, kk]] += spec.beta * r
        torch.from_numpy(track_of).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda()
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e6)
    return sorted(whole)[runs // 2]


def measure(line, res, cell, cap, a):
    """The tracks of the objects of the maps res['state'] with the origins res['origin'] -> line, with its times."""
    M, nx, ny = res["state"].shape
    ospec = objects.ObjectSpec(cell, max_objects=cap)
    ows = objects.ObjectWorkspace(ospec, M, nx, ny)
    table = objects.map_objects(ospec, res, res, workspace=ows)
    spec = tracks.TrackSpec(max_tracks=cap)
    held = tracks.ObjectTracks(spec, M, nx, ny, cell)
    ws = tracks.TrackWorkspace(spec, held, cap)

    def call():
        return tracks.track_objects(spec, held, table, res, workspace=ws)

    born = call()["info"].tolist()
    steady = call()["info"].tolist()
    line.update(map=[M, nx, ny], max_objects=cap, max_tracks=cap, objects=table["info"][:, 0].tolist(),
                first_call_born=[r[tracks.N_BORN] for r in born], steady_matched=[r[tracks.N_MATCHED] for r in steady],
                steady_rounds=[r[tracks.ROUNDS] for r in steady])
    med, lo, hi = replayed(call, a.warmup, a.runs)
    line.update(crd_track_objects_steady_us_median=round(med, 2), crd_track_objects_steady_us_min_max=[round(lo, 2), round(hi, 2)])
    # the first half of the table only, on tracks of every row that never drop: half the tracks stay open over the rounds
    coast = tracks.TrackSpec(max_tracks=cap, max_misses=2 ** 31 - 1)
    coasting = tracks.ObjectTracks(coast, M, nx, ny, cell)
    tracks.track_objects(coast, coasting, table, res, workspace=ws)
    half = dict(table, info=table["info"].clone())
    half["info"][:, 0] //= 2
    med, lo, hi = replayed(lambda: tracks.track_objects(coast, coasting, half, res, workspace=ws), a.warmup, a.runs)
    line.update(crd_track_objects_half_the_tracks_unmatched_us_median=round(med, 2), half_matched=ws.out["info"][:, tracks.N_MATCHED].tolist(),
                half_rounds=ws.out["info"][:, tracks.ROUNDS].tolist())
    med, lo, hi = replayed(lambda: (held.reset(), call()), a.warmup, a.runs)
    line.update(reset_and_crd_track_objects_all_born_us_median=round(med, 2))
    med, lo, hi = replayed(held.reset, a.warmup, a.runs)
    line.update(reset_alone_us_median=round(med, 2))
    med, lo, hi = replayed(lambda: objects.map_objects(ospec, res, res, workspace=ows), a.warmup, a.runs)
    line.update(crd_map_objects_us_median=round(med, 2))
    call()
    last = call()["info"]
    line.update(guard=last[:, tracks.GUARD].tolist(), host_assignment_us_median=round(host_tracks_us(spec, held, table, res["origin"]), 1))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tracks: no GPU (a time measured anywhere else says nothing)")
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
            for turn in range(1, MAP_UPDATES + 1):                           # the map tools/time_objects.py measures on
                res = occupancy.update(omap, pts, map_from_points=poses[turn % N_POSES], workspace=ows, out=ows.out)
            for cap in CAPS:
                print(json.dumps(dict(measure({"shape": name, "cell_m": cell}, res, cell, cap, a), runs=a.runs)), flush=True)
    for share in (0.01, 0.41):
        for M in (1, 8):
            for nx, ny in ((160, 160), (400, 400)):
                gen = torch.Generator(device="cuda").manual_seed(nx + M)
                state = torch.where(torch.rand(M, nx, ny, device="cuda", generator=gen) < share, occupancy.OCCUPIED, occupancy.FREE).to(torch.uint8)
                res = {"state": state, "origin": torch.zeros(M, 2, dtype=torch.int64, device="cuda")}
                for cap in CAPS:
                    line = {"shape": f"sources on {round(share * 100)} % of the cells", "cell_m": 0.5}
                    print(json.dumps(dict(measure(line, res, 0.5, cap, a), runs=a.runs)), flush=True)


if __name__ == "__main__":
    main()
