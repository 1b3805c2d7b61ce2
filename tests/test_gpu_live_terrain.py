"""GPU: LivePipeline(terrain=) -- the terrain map as one more stage of the captured graph, directly behind occupancy.update, at the
model and image size of tests/test_gpu_live.py.  run()['terrain'] has the bits of terrain.update on the clouds of the stages called
one by one, fused from an empty map; with feeds_field=True the distance field is that of the terrain's state; with terrain=None the
pipeline is the one built without the argument."""
import numpy as np
import pytest
import torch

from tests import occupancy_cases

pytestmark = pytest.mark.gpu

# the occupancy map needs four frames of evidence for an OCCUPIED cell and sees three; the terrain map calls every cell with a step
# of more than a quantum OCCUPIED: the two states differ wherever the terrain has one, so a field shows which of them it read
# The small model's depth is untrained: its cloud is a shell 87 to 141 m ahead, so the window is centred 110 m ahead.
OCC = dict(nx=64, ny=48, cell=2.0, n_bins=64, max_range=200.0, z_floor=-50.0, z_lo=0.0, z_hi=50.0, min_points=2, l_occ=3, l_free=1, l_max=10,
           occupied_at=10, free_at=2, centre=(110.0, 0.0, 0.0))
TER = dict(z_quantum=1.0 / 64, z_range=(-60.0, 60.0), max_range=200.0, headroom=2.0, min_points=1, w_max=2, step_max=0.0, slope_max=0.0)
FIELD = dict(max_cells=8, unknown_cost=60)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in sorted(got):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == torch.float32:                                            # NaN where the ground is unknown
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} values"


def test_live_pipeline_with_a_terrain_map():
    from camradepth_amd import bev, field, occupancy, terrain, viz
    from camradepth_amd import lib as L
    from camradepth_amd.inference import InferenceGraph
    from camradepth_amd.live import LivePipeline
    from tests.test_gpu_live import B, CLOUD, CUT, H, N_SWEEPS, S, SIZE, W, assert_same, flat, sensor_set, small_model, stagewise
    model = small_model()
    common = dict(max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, viz={}, occupancy=OCC, field=FIELD)
    with pytest.raises(L.CrdError, match="terrain= needs occupancy="):
        LivePipeline(model, B, SIZE, S, CUT, max_points=600, max_sweeps=N_SWEEPS, cloud=CLOUD, terrain=TER)
    live = LivePipeline(model, B, SIZE, S, CUT, terrain=dict(TER, picture=True, picture_z_range=(-10.0, 10.0), feeds_field=True), **common)
    beside = LivePipeline(model, B, SIZE, S, CUT, terrain=dict(TER), **common)          # the field keeps reading the occupancy map
    off = LivePipeline(model, B, SIZE, S, CUT, terrain=None, **common)
    plain = LivePipeline(model, B, SIZE, S, CUT, **common)
    assert off.terrain_map is None and plain.terrain_map is None and live.terrain_map.M == B and live.terrain_map.status() == [0, 0]
    assert (live.terrain_map.nx, live.terrain_map.ny, live.terrain_map.cell) == (64, 48, 2.0)
    ig, vz = InferenceGraph(model, B, H, W), viz.Visualizer(B, H, W)
    fresh = terrain.TerrainMap(B, 64, 48, 2.0, device="cuda", **TER)
    fresh_occ = occupancy.OccupancyMap(B, device="cuda", **{k: v for k, v in OCC.items() if k != "centre"})
    spec = field.FieldSpec(2.0, **FIELD)
    out_from_cam = bev.CAM_TO_BEV.clone()
    out_from_cam[:, 3] = torch.tensor([1.5, 0.0, 1.6], dtype=torch.float64)                             # x forward, y left, z up
    out_from_cam = out_from_cam.cuda()
    centre, views, weights = cuda(np.array(OCC["centre"])), [], []
    for i, (seed, n_points) in enumerate(((11, (350, 250)), (12, (200, 320)), (13, (300, 300)))):
        c = dict(sensor_set(seed, n_points), out_from_cam=out_from_cam)
        pose = None if i == 0 else cuda(occupancy_cases.pose(3.0 * i, -2.5 * i, 0.2 * i, 0.25 * i))
        res = live.run(map_from_out=pose, **c)
        assert set(res) == {"image", "x", "radar", "rad_vel", "pred", "cloud", "occupancy", "terrain", "field", "pictures"}
        assert set(res["terrain"]) == set(terrain.OUTPUTS) | {"picture"}
        views.append({k: v.data_ptr() for k, v in res["terrain"].items()})
        got = {k: {n: v.clone() for n, v in res[k].items()} for k in ("terrain", "occupancy", "field")}
        got_flat = {k: v.clone() for k, v in flat(res).items()}
        torch.cuda.synchronize()
        stages = stagewise(model, ig, vz, c)
        kw = dict(map_from_points=pose, sensor=out_from_cam[:, 3].contiguous(), centre=centre)
        want = terrain.update(fresh, stages["cloud"], **kw)
        want_occ = occupancy.update(fresh_occ, stages["cloud"], **kw)
        assert torch.equal(want["origin"], want_occ["origin"])                                           # equal by construction
        want_field = field.distance_field(spec, want)
        same(got["terrain"], dict(want, picture=terrain.picture(want, (-10.0, 10.0))), f"frame {i}: terrain")
        same(got["occupancy"], want_occ, f"frame {i}: occupancy")
        same(got["field"], want_field, f"frame {i}: the field of the terrain's state")
        occupied = (int((want["state"] == terrain.OCCUPIED).sum()), int((want_occ["state"] == occupancy.OCCUPIED).sum()))
        print(f"frame {i}: OCCUPIED cells of the terrain map and of the occupancy map: {occupied}")
        assert occupied[0] > 0 and occupied[1] == 0 and not torch.equal(want_field["cost"], field.distance_field(spec, want_occ)["cost"])
        weights.append(want["weight"].clone())
        # feeds_field=False: the terrain beside a field that reads the occupancy map; terrain=None: the pipeline without the argument
        r = beside.run(map_from_out=pose, **c)
        same({k: v.clone() for k, v in r["terrain"].items()}, want, f"frame {i}: terrain beside the field")
        same({k: v.clone() for k, v in r["field"].items()}, field.distance_field(spec, want_occ), f"frame {i}: the field of the occupancy map")
        a, b = off.run(map_from_out=pose, **c), plain.run(map_from_out=pose, **c)
        assert set(a) == set(b) == set(res) - {"terrain"}
        assert_same({k: v.clone() for k, v in flat(a).items()}, {k: v.clone() for k, v in flat(b).items()}, f"frame {i}: terrain=None")
        assert_same(got_flat, {k: v.clone() for k, v in flat(b).items()}, f"frame {i}: with and without terrain=")
        for k in ("occupancy", "field"):
            same(dict(a[k]), dict(b[k]), f"frame {i}: {k} with terrain=None")
    assert views[0] == views[1] == views[2] and live.terrain_map.status() == [0, 0]
    assert int(weights[0].max()) == 1 and int(weights[2].max()) == 2 and int((weights[0] > 0).sum()) > 0     # fused over the runs, from an empty map
    live.terrain_map.reset()
    again = live.run(map_from_out=pose, **c)["terrain"]
    assert int(again["weight"].max()) == 1
