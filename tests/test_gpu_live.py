"""GPU: camradepth_amd.live.LivePipeline -- raw camera frames and radar sweeps to depth, point cloud and pictures in one captured graph
-- against the same stages called one by one: camera_inputs -> radar_inputs -> assemble_batch -> InferenceGraph.run -> point_cloud ->
Visualizer.render.  Each stage has its own test file against its restatement; here every tensor the pipeline returns must have the
bits of the composition (torch.equal, floats as their bit patterns where no NaN can hide a difference)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_radar import offsets_of, sensor_points, sweeps

pytestmark = pytest.mark.gpu

B, SIZE, S, CUT = 2, (132, 192), 2, 2            # maps of 64 x 96
H, W = 64, 96
N_SWEEPS = 6
K1 = np.array([[150.0, 0, 96.3], [0, 153.0, 66.1], [0, 0, 1.0]])
CLOUD = dict(stride=1, min_range=1.0, rgb=True, pixel=True)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def small_model(input_channels=7, **kw):
    from camradepth_amd.model import CamRaDepth
    return CamRaDepth(input_channels=input_channels, depths=(1, 1, 1, 1), **kw).cuda().eval()


def sensor_set(seed, counts, pose=False):
    """Raw frames and radar sweeps of one batch on the device, with the dtypes LivePipeline.run copies without a conversion."""
    rs = np.random.RandomState(seed)
    cam1, cam2, lags = sweeps(rs, N_SWEEPS)
    pts, sw = sensor_points(rs, sum(counts), 0, N_SWEEPS)
    c = dict(frames=cuda(rs.randint(0, 256, size=(B,) + SIZE + (3,)).astype(np.uint8)), points=cuda(pts), sweep_index=cuda(sw),
             frame_offsets=cuda(offsets_of(counts)), cam1_from_sensor=cuda(cam1), cam2_from_sensor=cuda(cam2), lags=cuda(lags), K=cuda(K1))
    if pose:
        T = np.concatenate([np.linalg.qr(rs.normal(size=(3, 3)))[0], rs.uniform(-2, 2, size=(3, 1))], axis=1)
        c["out_from_cam"] = cuda(T)
    return c


SETS = ((11, (350, 250), False), (12, (200, 320), True))        # the second set has fewer points, and a pose for the cloud


def flat(result):
    """{name: tensor} of everything a run returns; the cloud's rows beyond its count are left out (they are not written)."""
    out = {k: result[k] for k in ("image", "x", "radar", "rad_vel") if k in result}
    d, s = result["pred"]["depth"], result["pred"]["seg"]
    out.update({"final_depth": d["final_depth"], "half": d["intermediate_depths"][3], "quarter": d["intermediate_depths"][2]})
    out.update({k: s[k] for k in ("final_seg", "unsup_map") if s[k] is not None})
    if "cloud" in result:
        n = int(result["cloud"]["frame_offsets"][-1])
        out.update({f"cloud.{k}": (v if k == "frame_offsets" else v[:n]) for k, v in result["cloud"].items()})
    out.update({f"pictures.{k}": v for k, v in result.get("pictures", {}).items()})
    return out


def assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in sorted(got):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == torch.float32 and not torch.isnan(a).any():
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} values"


def stagewise(model, ig, vz, c, Cin=7):
    """The same stages one by one, every result a fresh tensor."""
    from camradepth_amd import camera, cloud, radar
    from camradepth_amd.batch import assemble_batch
    out = {}
    if Cin == 3:
        cam = camera.camera_inputs(c["frames"], S, CUT, "rgb", "bgr", normalised=True)
        x = cam["x"]
    else:
        cam = camera.camera_inputs(c["frames"], S, CUT, "rgb", "bgr")
        maps = radar.radar_inputs(c["points"], c["sweep_index"], c["frame_offsets"], c["cam1_from_sensor"], c["cam2_from_sensor"], c["lags"],
                                  c["K"], SIZE, 1.0, 2.0, S, CUT)
        zeros = torch.zeros(B, H, W, device="cuda")
        x = assemble_batch(cam["image"], maps["radar"], maps["rad_vel"] if Cin == 7 else None, zeros)["image"]
        out.update(radar=maps["radar"], rad_vel=maps["rad_vel"])
    out.update(image=cam["image"], x=x, pred=ig.run(x))
    out["cloud"] = cloud.point_cloud(out["pred"]["depth"]["final_depth"], c["K"], SIZE, S, CUT, out_from_cam=c.get("out_from_cam"),
                                     min_range=1.0, image=cam["image"], with_pixel=True)
    out["pictures"] = {k: v.clone() for k, v in vz.render(cam["image"], x if Cin > 3 else None, out["pred"]).items()}
    return out


@pytest.mark.parametrize("heads", [False, True], ids=["base", "both seg heads"])
def test_one_graph_equals_the_stages_one_by_one(heads):
    from camradepth_amd import viz
    from camradepth_amd.inference import InferenceGraph
    from camradepth_amd.live import LivePipeline
    model = small_model(supervised_seg=True, unsupervised_seg=True) if heads else small_model()
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={})
    ig, vz = InferenceGraph(model, B, H, W), viz.Visualizer(B, H, W)
    seen, views = [], []
    for seed, counts, pose in SETS:
        c = sensor_set(seed, counts, pose)
        res = live.run(**c)
        names = {"image", "x", "radar", "rad_vel", "pred", "cloud", "pictures"}
        assert set(res) == names and res["x"].shape == (B, 7, H, W) and res["pred"]["depth"]["final_depth"].shape == (B, 1, H, W)
        assert set(res["cloud"]) == {"xyz", "frame_offsets", "rgb", "pixel"}
        assert set(res["pictures"]) == {"depth_pred", "depth_on_rgb", "radar", "collage"} | ({"pred_seg", "unsup"} if heads else set())
        views.append({k: v.data_ptr() for k, v in flat(res).items()})
        got = {k: v.clone() for k, v in flat(res).items()}       # the plan's buffers are the InferenceGraph's too: keep the bits first
        torch.cuda.synchronize()
        assert int(res["cloud"]["frame_offsets"][-1]) > 0 and (res["radar"][..., 0] != 0).sum() >= 5
        assert_same(got, flat(stagewise(model, ig, vz, c)), f"heads {heads}, set {seed}")
        seen.append(got)
    assert views[0] == views[1]                                  # views of the same static buffers, run after run
    for k in ("image", "radar", "final_depth", "pictures.collage"):
        assert not torch.equal(seen[0][k], seen[1][k]), k        # the second set's results, not the first's again
    assert seen[0]["cloud.xyz"].shape != seen[1]["cloud.xyz"].shape or not torch.equal(seen[0]["cloud.xyz"], seen[1]["cloud.xyz"])


def test_run_allocates_nothing_and_clone_returns_copies():
    from camradepth_amd.live import LivePipeline
    live = LivePipeline(small_model(), B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={})
    sets = [sensor_set(seed, counts, pose) for seed, counts, pose in SETS]
    first = live.run(**sets[0])
    torch.cuda.synchronize()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    for c in (sets[1], sets[0]):
        again = live.run(**c)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count
    assert {k: v.data_ptr() for k, v in flat(again).items()} == {k: v.data_ptr() for k, v in flat(first).items()}
    copies = flat(live.run(clone=True, **sets[0]))
    kept = {k: v.clone() for k, v in copies.items()}
    assert all(copies[k].data_ptr() != v.data_ptr() for k, v in flat(first).items())
    live.run(**sets[1])                                          # overwrites the views, not the copies
    torch.cuda.synchronize()
    assert_same(copies, kept, "copies after another run")
    assert not torch.equal(flat(first)["final_depth"], kept["final_depth"])


def test_changed_weights_show_after_mark_params_changed():
    from camradepth_amd.inference import InferenceGraph
    from camradepth_amd.live import LivePipeline
    model = small_model()
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS)
    c = sensor_set(*SETS[0])
    res = live.run(clone=True, **c)
    assert set(res) == {"image", "x", "radar", "rad_vel", "pred"}                  # cloud=None, viz=None: those keys are left out
    before = res["pred"]["depth"]["final_depth"]
    with torch.no_grad():
        model.flat.mul_(0.9)
    model.mark_params_changed()
    after = live.run(clone=True, **c)["pred"]["depth"]["final_depth"]
    assert not torch.equal(before, after)
    want = InferenceGraph(model, B, H, W).run(res["x"])["depth"]["final_depth"]
    assert torch.equal(after, want)


@pytest.mark.parametrize("Cin", [6, 3], ids=["without rad_vel", "RGB only"])
def test_other_input_layouts(Cin):
    from camradepth_amd import lib as L
    from camradepth_amd import viz
    from camradepth_amd.inference import InferenceGraph
    from camradepth_amd.live import LivePipeline
    model = small_model(Cin)
    tables = dict(max_points=600, max_sweeps=N_SWEEPS) if Cin > 3 else {}
    live = LivePipeline(model, B, SIZE, S, CUT, cloud=CLOUD, viz={}, **tables)
    c = sensor_set(*SETS[1])
    args = c if Cin > 3 else {k: c[k] for k in ("frames", "K", "out_from_cam")}
    res = live.run(**args)
    got = {k: v.clone() for k, v in flat(res).items()}
    assert res["x"].shape == (B, Cin, H, W) and ("radar" in res) == (Cin > 3) and ("radar" in res["pictures"]) == (Cin > 3)
    want = flat(stagewise(model, InferenceGraph(model, B, H, W), viz.Visualizer(B, H, W), c, Cin))
    assert_same(got, want, f"{Cin} input channels")
    with pytest.raises(L.CrdError):
        live.run(**(c if Cin == 3 else {k: c[k] for k in ("frames", "K")}))       # radar arguments where none belong, none where they do


def test_wrong_models_shapes_and_arguments_are_refused():
    from camradepth_amd import lib as L
    from camradepth_amd.live import LivePipeline
    model = small_model()
    with pytest.raises(L.CrdError, match="32"):
        LivePipeline(model, B, (100, 192), S, CUT, max_points=10, max_sweeps=2)       # maps of 48 x 96
    with pytest.raises(L.CrdError, match="max_points"):
        LivePipeline(model, B, SIZE, S, CUT)
    with pytest.raises(L.CrdError, match="cloud"):
        LivePipeline(model, B, SIZE, S, CUT, max_points=10, max_sweeps=2, cloud=dict(colour=True))
    with pytest.raises(L.CrdError, match="order"):
        LivePipeline(model, B, SIZE, S, CUT, max_points=10, max_sweeps=2, order_in="yuv")
    with pytest.raises(L.CrdError, match="input channels"):
        LivePipeline(small_model(5), B, SIZE, S, CUT, max_points=10, max_sweeps=2)
    live = LivePipeline(model, B, SIZE, S, CUT, max_points=100, max_sweeps=N_SWEEPS)
    c = sensor_set(13, (350, 250))
    with pytest.raises(L.CrdError, match="capacity"):
        live.run(**c)                                            # 600 points into tables of 100
    few = sensor_set(14, (40, 50))
    for bad in (dict(frames=few["frames"][:, :100]), dict(frames=few["frames"].float()), dict(K=few["K"].float()),
                dict(points=few["points"][:, :4]), dict(sweep_index=few["sweep_index"][:50])):
        with pytest.raises(L.CrdError):
            live.run(**dict(few, **bad))
    live.run(**few)
