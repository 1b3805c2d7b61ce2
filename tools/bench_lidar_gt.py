#!/usr/bin/env python3
"""Time camradepth_amd.lidar.lidar_gt for one key frame at the reference's size: 27 sweeps x 34,720 synthetic points, 40 boxes,
900 x 1600 -> 416 x 800, both occlusion filters on.  Warm runs, device events, the median; one JSON line.

    python tools/bench_lidar_gt.py --runs 30
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_lidar_gt.py --runs 20        # the per-launch split (k_lidar_*, k_zbuf_*)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import lidar  # noqa: E402

AXES = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 1.2], [1.0, 0.0, 0.0, -0.5], [0.0, 0.0, 0.0, 1.0]])


def pose(centre, yaw):
    M = np.eye(4)
    M[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
    M[:3, 3] = centre
    return M


def make_frame(S=27, per_sweep=34720, n_boxes=40, seed=0):
    """A spinning lidar's rings on a ground plane and on the boxes' tops, seen by a front camera; every box in every sweep."""
    rs = np.random.RandomState(seed)
    n = S * per_sweep
    az, ring = rs.uniform(-np.pi, np.pi, n), rs.randint(0, 32, n)
    elev = np.radians(-30.0 + ring * (40.0 / 31.0))
    r = np.where(elev < -0.02, np.minimum(1.84 / np.maximum(-np.sin(elev), 1e-3), 90.0), rs.uniform(5, 90, n))
    pts = np.stack([r * np.cos(elev) * np.cos(az), r * np.cos(elev) * np.sin(az), r * np.sin(elev)], axis=1)
    sweep = np.repeat(np.arange(S, dtype=np.int32), per_sweep)
    shift = lambda dx: np.array([[1.0, 0, 0, dx], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])      # noqa: E731
    cam1 = np.stack([(AXES @ shift(0.4 * (s - 9)))[:3] for s in range(S)])
    cam2 = np.stack([(AXES @ shift(0.4 * (s - 9) - 0.8))[:3] for s in range(S)])
    car_z = np.tile(np.array([[0.0, 0.0, 1.0, 1.84]]), (S, 1))
    centres = np.stack([rs.uniform(6, 60, n_boxes), rs.uniform(-12, 12, n_boxes), np.full(n_boxes, -1.0)], axis=1)
    sizes = np.stack([rs.uniform(1.6, 2.4, n_boxes), rs.uniform(3.5, 8.0, n_boxes), rs.uniform(1.4, 3.0, n_boxes)], axis=1)       # w, l, h
    yaws = rs.uniform(-0.5, 0.5, n_boxes)
    entries, box_id = [], []
    for s in range(S):
        for k in range(n_boxes):
            P = pose(centres[k] + [0.1 * (s - 9), 0, 0], yaws[k])
            entries.append(np.concatenate([np.linalg.inv(P)[:3].reshape(12), 0.5 * sizes[k, [1, 0, 2]]]))
            box_id.append(k)
    cam1_box = np.stack([(AXES @ pose(centres[k], yaws[k]))[:3] for k in range(n_boxes)])
    cam2_box = np.stack([(AXES @ shift(-0.8) @ pose(centres[k] + [0.3, 0, 0], yaws[k]))[:3] for k in range(n_boxes)])
    K = np.array([[1266.4, 0.0, 816.3], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]])
    rr, cc = np.mgrid[0:416, 0:800]
    dev = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a if t is None else np.asarray(a).astype(t))).cuda()      # noqa: E731
    args = dict(points=dev(pts), sweep_index=dev(sweep), frame_offsets=dev(np.array([0, n], dtype=np.int32)), cam1_from_sensor=dev(cam1),
                cam2_from_sensor=dev(cam2), car_z_from_sensor=dev(car_z), K=dev(K),
                sweep_boxes=dev(np.arange(S + 1, dtype=np.int32) * n_boxes), box_entries=dev(np.array(entries)),
                box_id=dev(np.array(box_id, dtype=np.int32)), cam1_from_box=dev(cam1_box), cam2_from_box=dev(cam2_box),
                vehicle=dev((np.arange(n_boxes) % 4 != 0).astype(np.uint8)))
    off = dev(np.array([0, n_boxes], dtype=np.int32))
    args["corners"] = lidar.project_corners(dev(cam2_box), dev(sizes), off, args["K"])
    args["corner_offsets"] = off
    args["seg"] = dev(((rr // 16 + cc // 16) % 3 != 0).astype(np.uint8)[None])
    args["flow_im"] = dev(rs.normal(0, 2.0, size=(1, 416, 800, 2)).astype(np.float32))
    return args, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lidar_gt: no GPU (a time measured anywhere else says nothing)")
    args, n = make_frame()
    ws = lidar.LidarWorkspace(1, max_points=n, max_boxes=40)
    out = {"gt": torch.empty(1, 416, 800, 3, device="cuda"), "depth": torch.empty(1, 416, 800, device="cuda"),
           "msk_lh": torch.empty(1, 416, 800, dtype=torch.uint8, device="cuda")}
    for _ in range(a.warmup):
        lidar.lidar_gt(**args, workspace=ws, out=out)
    torch.cuda.synchronize()
    times = {"lidar_gt": [], "project_lidar": [], "lidar_ground_truth": []}
    proj_args = {k: v for k, v in args.items() if k not in ("corners", "corner_offsets", "seg", "flow_im")}
    for _ in range(a.runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        lidar.lidar_gt(**args, workspace=ws, out=out)
        ev[1].record()
        proj = lidar.project_lidar(**proj_args, out=ws.proj_out(n))
        ev[2].record()
        lidar.lidar_ground_truth(proj, args["frame_offsets"], args["K"], seg=args["seg"], corners=args["corners"],
                                 corner_offsets=args["corner_offsets"], flow_im=args["flow_im"], workspace=ws, out=out)
        ev[3].record()
        torch.cuda.synchronize()
        for k, i in (("lidar_gt", 0), ("project_lidar", 1), ("lidar_ground_truth", 2)):
            times[k].append(ev[i].elapsed_time(ev[i + 1]))
    valid = int(ws.proj_out(n)["valid"].sum())
    res = {"points": n, "valid_points": valid, "pixels_left": int((out["depth"] != 0).sum()), "runs": a.runs}
    res.update({k + "_ms_median": round(float(np.median(v)), 4) for k, v in times.items()})
    res.update({k + "_ms_min_max": [round(float(min(v)), 4), round(float(max(v)), 4)] for k, v in times.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
