#!/usr/bin/env python3
"""Time the local planner (camradepth_amd.rollout) on the map of tools/time_occupancy.py's drive -- the road scene of tools/time_bev.py
fused through 20 poses one metre apart -- for 1 map of a full frame and 8 maps of a batch, a window of 80 m x 80 m of 0.5 m cells
(160 x 160) with its distance field (max_cells 16) and a cost-to-go towards a goal 30 m ahead.  The vehicle stands at the last pose.
(K, P, T) = (255, 64, 0), (1023, 128, 256) and (1023, 128, 1024): n_v x n_w = 15 x 17 and 33 x 31, the nearest to 256 and 1,024 that an
odd n_w allows; the T tracks are drawn over the window, all of them counting.  Every call is captured in a graph with its workspace and
replayed: HIP events round a replay, 20 warm-up and 100 timed replays, the median microseconds of crd_plan_rollouts (two launches)
beside crd_field_paths on the same 'xy' (the static half it generalises), and beside the NumPy restatement tests/rollout_ref.py on the
host with its copies down (wall clock, one run).

    python tools/time_rollout.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_rollout.py --no-host      # the per-launch split (k_rollouts, k_rollout_pick)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import bev, cloud, field, nav, occupancy, rollout, tracks  # noqa: E402
from time_bev import K_FULL, SHAPES, X_RANGE, Y_RANGE, road_scene  # noqa: E402
from time_objects import replayed  # noqa: E402
from time_occupancy import CAMERA_HEIGHT, N_BINS, N_POSES  # noqa: E402

CELL = 0.5
PLANS = ((15, 17, 64, 0), (33, 31, 128, 256), (33, 31, 128, 1024))               # n_v, n_w, P, T
MAP = dict(n_bins=N_BINS, max_range=80.0, z_floor=-0.3, z_lo=0.3, z_hi=3.0)


def drawn_tracks(M, nx, ny, T, origin):
    """An ObjectTracks of T confirmed slots per map, spread over the window, moving up to 0.2 m per update."""
    t = tracks.ObjectTracks(tracks.TrackSpec(max_tracks=T), M, nx, ny, CELL)
    g = torch.Generator(device="cuda").manual_seed(7)
    low = origin.double() * CELL
    span = torch.tensor([nx * CELL, ny * CELL], dtype=torch.float64, device="cuda")
    t.pos.copy_(low[:, None, :] + torch.rand(M, T, 2, dtype=torch.float64, device="cuda", generator=g) * span)
    t.vel.copy_((torch.rand(M, T, 2, dtype=torch.float64, device="cuda", generator=g) - 0.5) * 0.4)
    t.tracks[..., tracks.STATUS] = tracks.CONFIRMED
    t.tracks[..., tracks.N_CELLS] = 10
    return t


def host_rollout_us(numbers, pose, res, dist, togo, trk):
    """Wall-clock microseconds of tests/rollout_ref.plan_rollouts on the host: the inputs copied down, the restatement, the command up."""
    from tests import rollout_ref
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kw = {} if trk is None else dict(tracks=trk.tracks.cpu().numpy(), pos=trk.pos.cpu().numpy(), vel=trk.vel.cpu().numpy())
    out = rollout_ref.plan_rollouts(rollout_ref.spec(**numbers), pose.cpu().numpy(), res["origin"].cpu().numpy(), CELL, dist["cost"].cpu().numpy(),
                                    togo=togo["togo"].cpu().numpy(), chunk=16, **kw)
    torch.from_numpy(out["command"]).cuda()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out["best"].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="leave the NumPy restatement on the host out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rollout: no GPU (a time measured anywhere else says nothing)")
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
        nx, ny = bev.grid_shape(X_RANGE, Y_RANGE, CELL)
        omap = occupancy.OccupancyMap(B, nx, ny, CELL, **MAP)
        ows = occupancy.OccupancyWorkspace(omap, B)
        for T in poses:
            res = occupancy.update(omap, pts, map_from_points=T, workspace=ows, out=ows.out)
        fspec = field.FieldSpec(CELL, max_cells=16, inscribed=CELL)
        dist = field.distance_field(fspec, res)
        vehicle = torch.eye(3, 4, dtype=torch.float64).repeat(B, 1, 1)
        vehicle[:, 0, 3] = float(N_POSES - 1)
        vehicle = vehicle.cuda()
        goals = torch.tensor([[[N_POSES - 1 + 30.0, 0.0]]], dtype=torch.float64).repeat(B, 1, 1).cuda()
        togo = nav.nav_field(nav.NavSpec(CELL), dist, res, goals)
        for n_v, n_w, P, T in PLANS:
            numbers = dict(v=(0.5, 4.0, n_v), w=(0.8, n_w), dt=0.1, n_poses=P, keep_out=0.5, cell=CELL)
            spec = rollout.RolloutSpec(**numbers)
            trk = drawn_tracks(B, nx, ny, T, res["origin"]) if T else None
            ws = rollout.RolloutWorkspace(spec, B, tables=True, xy=True)
            plan = lambda: rollout.plan_rollouts(spec, vehicle, dist, res, nav_result=togo, tracks=trk, workspace=ws, tables=True, xy=True)      # noqa: E731
            med, lo, hi = replayed(plan, a.warmup, a.runs)
            out = ws.out
            xy = out["xy"].view(B * spec.K, P, 2)
            path_map = torch.arange(B, device="cuda").repeat_interleave(spec.K).int()
            pout = field.path_outputs(B * spec.K, P)
            pmed, plo, phi = replayed(lambda: field.check_paths(fspec, dist, res, xy, path_map=path_map, out=pout), a.warmup, a.runs)
            line = {"shape": name, "map": [B, nx, ny], "K": spec.K, "P": P, "T": T, "tests": B * spec.K * P * T,
                    "crd_plan_rollouts_us_median": round(med, 2), "crd_plan_rollouts_us_min_max": [round(lo, 2), round(hi, 2)],
                    "crd_field_paths_us_median": round(pmed, 2), "crd_field_paths_us_min_max": [round(plo, 2), round(phi, 2)],
                    "best": out["best"][:2].tolist(), "command": out["command"][:2].tolist(), "info": out["info"][:2, :5].tolist(),
                    "track_hits": int((out["first_track"] >= 0).sum())}
            if not a.no_host:
                us, best = host_rollout_us(numbers, vehicle, res, dist, togo, trk)
                line.update(host_numpy_us=round(us, 0), host_best_equal=best == out["best"].tolist())
            print(json.dumps(dict(line, runs=a.runs)), flush=True)
            del ws


if __name__ == "__main__":
    main()
