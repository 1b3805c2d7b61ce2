#!/usr/bin/env python3
"""Time the camera front end and the live pipeline at the shape a live caller runs: one 900 x 1600 frame -> 416 x 800, the full
7-channel model, 3000 radar points of 6 sweeps, the compact cloud with colours and the pictures.  ONE process measures, in this order
and with (b) and (c) alternating round by round so that the machine's drift enters both alike:

  (a) crd_camera_frontend alone (image only, and image + normalised planes): a graph of 50 launches replayed under HIP events,
      microseconds per launch beside its algorithmic bytes (the source rows it reads + what it writes) and the GB/s they make;
  (b) one LivePipeline.run: the copies into the static buffers and one replay of the one graph;
  (c) the same stages one by one as they could be called before LivePipeline existed: camera_inputs, radar_inputs (workspace and
      out= given), assemble_batch, InferenceGraph.run(clone=False), point_cloud and Visualizer.render (workspace and out= given),
      every stage a host call.  (c) minus (a) is what the stages cost without the camera kernel.

(b) and (c) are host wall-clock times from the call to the end of a device synchronise (`latency`: what a caller waits for one frame)
and of `--runs` calls back to back with one synchronise at the end (`pipelined`: the rate the device sustains).  The outputs of (b)
and (c) are compared first: equal bits or the tool stops.

    python tools/time_live.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import camera, cloud, radar, viz  # noqa: E402
from camradepth_amd.batch import assemble_batch  # noqa: E402
from camradepth_amd.inference import InferenceGraph  # noqa: E402
from camradepth_amd.live import LivePipeline  # noqa: E402
from camradepth_amd.model import CamRaDepth  # noqa: E402

B, SIZE, S, CUT = 1, (900, 1600), 2, 34
N_POINTS, N_SWEEPS = 3000, 6


def sensors(seed):
    rs = np.random.RandomState(seed)
    axes = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 1.2], [1.0, 0.0, 0.0, -0.5]])       # sensor x forward -> camera z forward
    pts = np.stack([rs.uniform(3, 100, N_POINTS), rs.uniform(-40, 40, N_POINTS), rs.uniform(-2, 3, N_POINTS), rs.normal(0, 3, N_POINTS),
                    rs.normal(0, 3, N_POINTS)], axis=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    return dict(frames=t(rs.randint(0, 256, size=(B,) + SIZE + (3,)).astype(np.uint8)), points=t(pts),
                sweep_index=t(rs.randint(0, N_SWEEPS, N_POINTS).astype(np.int32)), frame_offsets=t(np.array([0, N_POINTS], dtype=np.int32)),
                cam1_from_sensor=t(np.stack([axes] * N_SWEEPS)), cam2_from_sensor=t(np.stack([axes] * N_SWEEPS)),
                lags=t(rs.uniform(-0.3, 0.3, size=(N_SWEEPS, 2))),
                K=t(np.array([[1266.4, 0.0, 816.3], [0.0, 1270.9, 491.5], [0.0, 0.0, 1.0]])))


def events_per_launch(fn, launches, warmup, runs):
    """Median microseconds of one launch of fn: a graph of `launches` calls, replayed `runs` times under HIP events."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for a, b in ev:
        a.record()
        g.replay()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 / launches for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def latency(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def pipelined(fn, runs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / runs


def stats(v):
    v = sorted(v)
    return {"us_median": round(v[len(v) // 2], 1), "us_min_max": [round(v[0], 1), round(v[-1], 1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_live: no GPU (a time measured anywhere else says nothing)")
    h, w = camera.map_shape(SIZE, S, CUT)
    c = sensors(3)
    # (a) the camera kernel alone
    image = torch.empty(B, h, w, 3, dtype=torch.uint8, device="cuda")
    x3 = torch.empty(B, 3, h, w, device="cuda")
    read = B * h * S * SIZE[1] * 3
    for what, out, nbytes in (("image", {"image": image}, read + image.numel()), ("image + x", {"image": image, "x": x3}, read + image.numel() + 4 * x3.numel())):
        med, lo, hi = events_per_launch(lambda: camera.camera_inputs(c["frames"], S, CUT, out=out), 50, a.warmup, a.runs)
        print(json.dumps({"measure": "a", "entry": "crd_camera_frontend", "outputs": what, "us_median": round(med, 2), "us_min_max": [round(lo, 2), round(hi, 2)],
                          "algorithmic_bytes": nbytes, "GB_per_s": round(nbytes / med * 1e-3, 1)}), flush=True)
        if what == "image":
            camera_us = med
    # (b) and (c)
    model = CamRaDepth(input_channels=7).cuda().eval()
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=N_POINTS, max_sweeps=N_SWEEPS, cloud=dict(rgb=True, min_range=1.0), viz={})
    ig = InferenceGraph(model, B, h, w)
    rws, cws, vz = radar.RadarWorkspace(B, SIZE, S, max_points=N_POINTS), cloud.CloudWorkspace(B, SIZE, S, CUT), viz.Visualizer(B, h, w)
    maps = {"radar": torch.empty(B, h, w, 3, device="cuda"), "rad_vel": torch.empty(B, h, w, device="cuda")}
    gt = torch.zeros(B, h, w, device="cuda")
    cout = cws.outputs(rgb=True)

    def one_graph():
        return live.run(**c)

    def one_by_one():
        cam = camera.camera_inputs(c["frames"], S, CUT, out={"image": image})
        m = radar.radar_inputs(c["points"], c["sweep_index"], c["frame_offsets"], c["cam1_from_sensor"], c["cam2_from_sensor"], c["lags"], c["K"],
                               SIZE, 1.0, 2.0, S, CUT, workspace=rws, out=maps)
        x = assemble_batch(cam["image"], m["radar"], m["rad_vel"], gt)["image"]
        pred = ig.run(x, clone=False)
        pts = cloud.point_cloud(pred["depth"]["final_depth"], c["K"], SIZE, S, CUT, min_range=1.0, image=cam["image"], workspace=cws, out=cout)
        return {"pred": pred, "cloud": pts, "pictures": vz.render(cam["image"], x, pred)}

    got = one_graph()
    keep = {"depth": got["pred"]["depth"]["final_depth"].clone(), "collage": got["pictures"]["collage"].clone(),
            "offsets": got["cloud"]["frame_offsets"].clone()}
    n = int(keep["offsets"][-1])
    keep["xyz"] = got["cloud"]["xyz"][:n].clone()
    want = one_by_one()
    torch.cuda.synchronize()
    same = (torch.equal(keep["depth"], want["pred"]["depth"]["final_depth"]) and torch.equal(keep["collage"], want["pictures"]["collage"]) and
            torch.equal(keep["offsets"], want["cloud"]["frame_offsets"]) and torch.equal(keep["xyz"], want["cloud"]["xyz"][:n]))
    if not same:
        raise SystemExit("time_live: the one graph and the stages one by one disagree; nothing is timed")
    for fn in (one_graph, one_by_one):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    lat, pipe = {"b": [], "c": []}, {"b": [], "c": []}
    for _ in range(a.rounds):
        for key, fn in (("b", one_graph), ("c", one_by_one)):
            lat[key] += [latency(fn) for _ in range(a.runs)]
            pipe[key].append(pipelined(fn, a.runs))
    for key, what in (("b", "LivePipeline.run"), ("c", "stages one by one")):
        print(json.dumps({"measure": key, "what": what, "points_in_cloud": n, "latency": stats(lat[key]), "pipelined": stats(pipe[key]),
                          "runs": a.runs, "rounds": a.rounds}), flush=True)
    b_lat, c_lat = stats(lat["b"])["us_median"], stats(lat["c"])["us_median"]
    b_pipe, c_pipe = stats(pipe["b"])["us_median"], stats(pipe["c"])["us_median"]
    print(json.dumps({"measure": "c - a", "camera_us": round(camera_us, 2), "latency_us": round(c_lat - camera_us, 1), "pipelined_us": round(c_pipe - camera_us, 1),
                      "b_over_c_latency": round(b_lat / c_lat, 3), "b_over_c_pipelined": round(b_pipe / c_pipe, 3)}), flush=True)


if __name__ == "__main__":
    main()
