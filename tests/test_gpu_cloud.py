"""GPU: the point-cloud back end (camradepth_amd.cloud: unproject_depth, point_cloud, CloudWorkspace) against the NumPy restatement in
tests/cloud_ref.py.

Both sides are fp64 additions, multiplications and divisions in a stated order, never contracted, and one rounding to fp32 per
coordinate -- all correctly rounded -- and the order of the compact cloud is specified, so everything is compared bit for bit.  The
default map is image (40, 64), downsample_scale 2, y_cutoff 3: 17 x 32."""
import itertools

import numpy as np
import pytest
import torch

from tests import cloud_ref as ref

pytestmark = pytest.mark.gpu

SIZE, S, CUT = (40, 64), 2, 3
H, W = 17, 32
MAX_DEPTH = 100.0
ENCODING_BOUND = 4 * 2.0 ** -24 * MAX_DEPTH          # test_cloud_ref_cpu.py: three fp32 roundings of the encoder, one of the point
K1 = np.array([[50.7, 0.0, 32.6], [0.0, 50.9, 19.7], [0.0, 0.0, 1.0]])
SENTINEL = 7


@pytest.fixture(scope="module")
def cloud():
    from camradepth_amd import cloud as module
    return module


def cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def assert_equal(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == torch.float32:                                           # bits: -0.0 is not 0.0 and a NaN equals itself
        got, want = got.view(torch.int32), want.view(torch.int32)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} values differ; first at {i}: {got[i].item()!r} against {want[i].item()!r}")


def intrinsics(B, per_frame):
    if not per_frame:
        return K1
    return np.stack([K1 * np.array([[1 + 0.01 * b, 1, 1 - 0.02 * b], [1, 1 - 0.015 * b, 1 + 0.01 * b], [1, 1, 1]]) for b in range(B)])


def pose(rs):
    """A rigid transform [3, 4]: camera axes to x forward / z up, a yaw and a translation."""
    a = rs.uniform(-0.5, 0.5)
    yaw = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    axes = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    return np.concatenate([yaw @ axes, rs.uniform(-30, 30, size=(3, 1))], axis=1)


def random_map(rs, B, h, w, encoding):
    """Every kind of value: inside and outside the valid interval, NaN, +-inf, 0, 1, negative, above 1."""
    d = (rs.uniform(-0.2, 1.2, size=(B, h, w)) if encoding == "inverse" else rs.uniform(-5.0, 120.0, size=(B, h, w))).astype(np.float32)
    kind = rs.randint(0, 24, size=d.shape)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0)):
        d[kind == k] = v
    return d


def run_both(cloud, depth, K, what, strides=(1,), image=None, out_tail=True, **kw):
    """unproject_depth and point_cloud at every stride against the restatement, bit for bit; rows behind the last point keep the
    sentinel they were given."""
    B, h, w = depth.shape
    size, s, cut = kw.pop("size", SIZE), kw.pop("s", S), kw.pop("cut", CUT)
    dev = {k: (cuda(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    ref_kw = {("T" if k == "out_from_cam" else k): v for k, v in kw.items()}
    want_points, want_valid = ref.unproject(depth, K, s, cut, **ref_kw)
    got = cloud.unproject_depth(cuda(depth), cuda(K), size, s, cut, **dev)
    assert_equal(got["points"], want_points, f"{what}: points")
    assert_equal(got["valid"], want_valid, f"{what}: valid")
    for stride in strides:
        want = ref.point_cloud(depth, K, s, cut, stride=stride, image=image, **ref_kw)
        cap = B * cloud.candidates(h, w, stride)
        out = {"xyz": torch.full((cap, 3), float(SENTINEL), device="cuda"), "frame_offsets": torch.full((B + 1,), SENTINEL, dtype=torch.int32, device="cuda"),
               "pixel": torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda")}
        if image is not None:
            out["rgb"] = torch.full((cap, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        if "labels" in kw:
            out["label"] = torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda")
        got = cloud.point_cloud(cuda(depth), cuda(K), size, s, cut, stride=stride, image=None if image is None else cuda(image), with_pixel=True,
                                out=out, **dev)
        torch.cuda.synchronize()
        assert set(got) == set(out) and all(got[k].data_ptr() == out[k].data_ptr() for k in out)
        assert_equal(got["frame_offsets"], want["frame_offsets"], f"{what}, stride {stride}: frame_offsets")
        n = int(want["frame_offsets"][-1])
        for k in out:
            if k != "frame_offsets":
                assert_equal(got[k][:n], want[k], f"{what}, stride {stride}: {k}")
                assert (got[k][n:] == SENTINEL).all(), f"{what}, stride {stride}: {k} is written behind its last point"
    return want_valid


@pytest.mark.parametrize("encoding", ["inverse", "metres"])
def test_bit_equality_with_the_restatement(cloud, encoding):
    rs = np.random.RandomState(31)
    B = 3
    depth = random_map(rs, B, H, W, encoding)
    image = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    mask = (rs.uniform(size=(B, H, W)) < 0.7).astype(np.uint8) * rs.randint(1, 256, size=(B, H, W)).astype(np.uint8)
    labels = rs.randint(0, 256, size=(B, H, W)).astype(np.uint8)
    keep = set(rs.permutation(256)[:150].tolist())
    lo, hi = (20.0, 75.0)
    options = {"plain": {}, "mask": dict(mask=mask), "labels": dict(labels=labels, keep=keep), "skip_empty": dict(skip_empty=True),
               "range": dict(min_range=lo, max_range=hi), "min_range": dict(min_range=lo),
               "all": dict(mask=mask, labels=labels, keep=keep, skip_empty=True, min_range=lo, max_range=hi)}
    poses = {"no T": None, "one T": pose(rs), "T per frame": np.stack([pose(rs) for _ in range(B)])}
    seen = set()
    for (tname, T), per_frame, (oname, opt) in itertools.product(poses.items(), (False, True), options.items()):
        kw = dict(opt, encoding=encoding, max_depth=MAX_DEPTH if per_frame else 80.0)
        if T is not None:
            kw["out_from_cam"] = T
        valid = run_both(cloud, depth, intrinsics(B, per_frame), f"{encoding}, {tname}, K per frame {per_frame}, {oname}", strides=(1, 2, 3),
                         image=image, **kw)
        seen.add(int(valid.sum()))
        assert 0 < valid.sum() < valid.size
    assert len(seen) >= 5                                                    # the options do select different pixels
    # the depth values by name, one per pixel of a 1 x 8 map
    named = np.array([[[np.nan, np.inf, -np.inf, 0.0, 1.0, -0.25, 1.5, 0.5]]], dtype=np.float32)
    valid = run_both(cloud, named, K1, f"{encoding}, named values", strides=(1, 2), size=(2, 16), cut=0, encoding=encoding, max_depth=MAX_DEPTH)
    assert valid.flatten().tolist() == ([0, 0, 0, 1, 0, 1, 0, 1] if encoding == "inverse" else [0, 0, 0, 0, 1, 0, 1, 1])
    # a keep table on the device in place of a collection
    table = np.zeros(256, dtype=np.uint8)
    table[sorted(keep)] = 200
    run_both(cloud, depth, K1, f"{encoding}, keep table", labels=labels, keep=table, encoding=encoding)


def frames_of(rs, kinds, h, w):
    """Metres maps: 'none' has no valid pixel, 'all' only valid ones, 'some' about half."""
    out = []
    for kind in kinds:
        d = rs.uniform(1.0, 50.0, size=(h, w)).astype(np.float32)
        if kind == "none":
            d[:] = rs.choice([0.0, -3.0, np.nan], size=(h, w))
        elif kind == "some":
            d[rs.uniform(size=(h, w)) < 0.5] = 0.0
        out.append(d)
    return np.stack(out)


def edge_shapes():
    from camradepth_amd.cloud import TILE
    return [((10, 14), 0), ((2, 2 * (TILE - 1)), 0), ((2, 2 * TILE), 0), ((2, 2 * (TILE + 1)), 0), ((66, 134), 0)]


@pytest.mark.parametrize("case", range(5))
def test_compaction_edges(cloud, case):
    """Candidates per frame below one wave's share, TILE - 1, TILE, TILE + 1 and 2211 (no multiple of 64, three tiles), three frames with
    an empty, a full and a half-full one in every order, and a batch with no valid pixel at all."""
    size, cut = edge_shapes()[case]
    h, w = size[0] // 2 - cut, size[1] // 2
    assert cloud.candidates(h, w) == (35, cloud.TILE - 1, cloud.TILE, cloud.TILE + 1, 2211)[case]
    rs = np.random.RandomState(40 + case)
    for kinds in itertools.permutations(("none", "all", "some")):
        depth = frames_of(rs, kinds, h, w)
        valid = run_both(cloud, depth, K1, f"{h} x {w}, {kinds}", strides=(1, 2) if case in (0, 4) else (1,), size=size, s=2, cut=cut,
                         encoding="metres")
        counts = valid.reshape(3, -1).sum(axis=1)
        assert counts[kinds.index("none")] == 0 and counts[kinds.index("all")] == h * w and 0 < counts[kinds.index("some")] < h * w
    depth = frames_of(rs, ("none", "none", "none"), h, w)
    valid = run_both(cloud, depth, K1, f"{h} x {w}, no valid pixel", size=size, s=2, cut=cut, encoding="metres")      # offsets 0, nothing written
    assert not valid.any()


def test_more_tiles_than_one_pass_of_the_scan(cloud):
    """2,500 frames of 1 x 3 pixels: one tile each, so the single workgroup that sums the tile counts takes three passes."""
    rs = np.random.RandomState(50)
    depth = frames_of(rs, ["some"] * 2500, 1, 3)
    valid = run_both(cloud, depth, K1, "2500 frames", size=(2, 6), s=2, cut=0, encoding="metres")
    assert 3000 < valid.sum() < 4500


def sparse_metres(rs, B, h, w, fill=0.3):
    d = rs.uniform(2.5, 100.0, size=(B, h, w)).astype(np.float32)
    d[rs.uniform(size=d.shape) > fill] = 0.0
    return d


def test_round_trip_through_the_lidar_front_end(cloud):
    """point_cloud -> project_lidar -> lidar_ground_truth gives the metres map back bit for bit; the frame_offsets the cloud wrote are
    the ones the projection reads.  s = 2: at s = 1 the first row and column sit at coordinate 0, which the projection refuses."""
    from camradepth_amd import lidar
    rs = np.random.RandomState(60)
    B = 3
    depth = sparse_metres(rs, B, H, W)
    depth[1] = 0.0                                                           # an empty frame repeats an offset
    K = cuda(K1)
    c = cloud.point_cloud(cuda(depth), K, SIZE, S, CUT, encoding="metres", out={"xyz": torch.zeros(B * H * W, 3, device="cuda"),
                                                                                 "frame_offsets": torch.zeros(B + 1, dtype=torch.int32, device="cuda")})
    n = int(c["frame_offsets"][-1])
    assert n == (depth > 0).sum() >= 100 and c["frame_offsets"].tolist()[1] == c["frame_offsets"].tolist()[2]
    eye = torch.eye(4, dtype=torch.float64, device="cuda")[None, :3].contiguous()
    N = c["xyz"].shape[0]
    proj = lidar.project_lidar(c["xyz"].double(), torch.zeros(N, dtype=torch.int32, device="cuda"), c["frame_offsets"], eye, eye,
                               torch.zeros(1, 4, dtype=torch.float64, device="cuda"), K, image_size=SIZE, min_distance=0.0, min_z=0.0)
    assert int(proj["valid"].sum()) == n and bool(proj["valid"][:n].all())   # the rows behind the last point belong to no frame
    back = lidar.lidar_ground_truth(proj, c["frame_offsets"], K, SIZE, S, CUT)
    assert_equal(back["depth"], depth, "depth after the round trip")


def test_hand_off_from_the_batch_assembler(cloud):
    from camradepth_amd.batch import assemble_batch
    rs = np.random.RandomState(70)
    B = 2
    gt = sparse_metres(rs, B, H, W)
    gt[0, 0, :3] = (99.5, 2.5, 50.0)
    img = cuda(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8))
    radar, vel = cuda(rs.uniform(0, 60, size=(B, H, W, 3)).astype(np.float32)), cuda(rs.uniform(size=(B, H, W)).astype(np.float32))
    full = assemble_batch(img, radar, vel, cuda(gt), max_depth=MAX_DEPTH)["gt_full"]
    assert full.shape == (B, 1, H, W)
    c = cloud.point_cloud(full, cuda(K1), SIZE, S, CUT, max_depth=MAX_DEPTH, encoding="inverse", skip_empty=True, with_pixel=True)
    off = c["frame_offsets"].tolist()
    assert off[0] == 0 and off[-1] == (gt > 0).sum()
    b, r, col = np.nonzero(gt > 0)                                           # points only where there is ground truth, in (b, r, c) order
    assert off == [0] + np.cumsum(np.bincount(b, minlength=B)).tolist()
    assert_equal(c["pixel"][:off[-1]], (r * W + col).astype(np.int32), "pixel")
    err = np.abs(c["xyz"][:off[-1], 2].cpu().numpy().astype(np.float64) - gt[b, r, col].astype(np.float64))
    print(f"z against gt_depth: max |error| {err.max():.3e}, bound {ENCODING_BOUND:.3e}")
    assert err.max() <= ENCODING_BOUND


def test_two_runs_capture_and_no_allocation(cloud):
    """Two runs give the same bits.  With a CloudWorkspace and out= the call is kernel launches only: nothing is allocated, and a graph
    captured on a side stream replays with fewer, then more, valid pixels in the depth buffer; counts and contents follow."""
    rs = np.random.RandomState(80)
    B = 3
    maps = {"first": random_map(rs, B, H, W, "inverse"), "fewer": random_map(rs, B, H, W, "inverse"), "more": random_map(rs, B, H, W, "inverse")}
    maps["fewer"][rs.uniform(size=(B, H, W)) < 0.6] = np.nan
    maps["more"][np.isnan(maps["more"]) | np.isinf(maps["more"])] = 0.5
    image = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    T = np.stack([pose(rs) for _ in range(B)])
    want = {k: ref.point_cloud(v, K1, S, CUT, stride=1, image=image, T=T, max_depth=MAX_DEPTH) for k, v in maps.items()}
    counts = {k: int(v["frame_offsets"][-1]) for k, v in want.items()}
    assert counts["fewer"] < counts["first"] < counts["more"]
    depth, K, Td, img = cuda(maps["first"]).unsqueeze(1), cuda(K1), cuda(T), cuda(image)          # [B,1,h,w], as final_depth
    a = cloud.point_cloud(depth, K, SIZE, S, CUT, out_from_cam=Td, image=img, with_pixel=True)
    b = cloud.point_cloud(depth, K, SIZE, S, CUT, out_from_cam=Td, image=img, with_pixel=True)
    torch.cuda.synchronize()
    n = counts["first"]
    assert a["xyz"].data_ptr() != b["xyz"].data_ptr()
    for k in a:
        rows = slice(None) if k == "frame_offsets" else slice(0, n)
        assert_equal(a[k][rows], b[k][rows], f"{k}, second run")
    ws = cloud.CloudWorkspace(B, SIZE, S)                                    # sized for y_cutoff 0: the cutoff of the call fits
    out = ws.outputs(rgb=True, pixel=True)
    assert set(ws.out) == {"xyz", "frame_offsets"} and ws.xyz.shape[0] == B * 20 * 32

    def call():
        return cloud.point_cloud(depth, K, SIZE, S, CUT, out_from_cam=Td, image=img, with_pixel=True, workspace=ws, out=out)

    def check(which):
        torch.cuda.synchronize()
        assert_equal(out["frame_offsets"], want[which]["frame_offsets"], f"{which}: frame_offsets")
        for k in ("xyz", "rgb", "pixel"):
            assert_equal(out[k][:counts[which]], want[which][k], f"{which}: {k}")

    res = call()                                                             # eager once: the code objects are loaded before the capture
    assert all(res[k].data_ptr() == out[k].data_ptr() for k in out)
    check("first")
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                # captures on a side stream
        call()
    for which in ("fewer", "more", "first"):
        depth.copy_(cuda(maps[which]).unsqueeze(1))
        for k in out:
            out[k].fill_(SENTINEL)
        g.replay()
        check(which)
        assert (out["xyz"][counts[which]:] == SENTINEL).all()


def test_cloud_graph_behind_the_inference_graph(cloud):
    """INTEGRATION.md's worked example: InferenceGraph.run(x, clone=False) returns views of static buffers, the cloud's graph is captured
    once on them and replayed behind every frame."""
    from camradepth_amd import synth
    from camradepth_amd.inference import InferenceGraph
    from camradepth_amd.model import CamRaDepth
    B, h, w = 2, 64, 96
    size = (2 * h, 2 * w)
    model = CamRaDepth(input_channels=7, depths=(1, 1, 1, 1)).cuda().eval()
    ig = InferenceGraph(model, B, h, w)
    frames = [synth.make_batch(B, h, w, seed=s)["image"].cuda() for s in (5, 6)]
    final = ig.run(frames[0], clone=False)["depth"]["final_depth"]
    assert final.shape == (B, 1, h, w)
    K = cuda(K1)
    ws = cloud.CloudWorkspace(B, size, 2)
    cloud.point_cloud(final, K, size, 2, 0, min_range=1.0, workspace=ws, out=ws.out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cloud.point_cloud(final, K, size, 2, 0, min_range=1.0, workspace=ws, out=ws.out)
    seen = []
    for x in frames:
        again = ig.run(x, clone=False)["depth"]["final_depth"]
        g.replay()
        torch.cuda.synchronize()
        assert again.data_ptr() == final.data_ptr()
        want = ref.point_cloud(final[:, 0].cpu().numpy(), K1, 2, 0, min_range=1.0)
        n = int(want["frame_offsets"][-1])
        assert n > 0
        assert_equal(ws.frame_offsets, want["frame_offsets"], "frame_offsets")
        assert_equal(ws.xyz[:n], want["xyz"], "xyz")
        seen.append(ws.xyz[:n].clone())
    assert seen[0].shape != seen[1].shape or not torch.equal(seen[0], seen[1])       # the second frame's points, not the first's again


def test_wrong_inputs_are_refused(cloud):
    from camradepth_amd import lib as L
    B = 2
    depth, K = torch.rand(B, H, W, device="cuda"), cuda(K1)
    mask = torch.ones(B, H, W, dtype=torch.uint8, device="cuda")
    image = torch.zeros(B, H, W, 3, dtype=torch.uint8, device="cuda")
    T = torch.zeros(3, 4, dtype=torch.float64, device="cuda")
    ws = cloud.CloudWorkspace(B, SIZE, S, CUT)
    marker = torch.full((B + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    ws.frame_offsets.copy_(marker)

    def refused(d=depth, k=K, fns=(cloud.unproject_depth, cloud.point_cloud), size=SIZE, s=S, cut=CUT, **kw):
        for fn in fns:
            with pytest.raises(L.CrdError):
                fn(d, k, size, s, cut, **kw)

    only_cloud = (cloud.point_cloud,)
    refused(d=depth.cpu()), refused(k=K.cpu()), refused(mask=mask.cpu()), refused(out_from_cam=T.cpu())          # not on the GPU
    refused(d=depth.double()), refused(d=depth.half()), refused(k=K.float()), refused(mask=mask.bool()), refused(mask=mask.int())
    refused(labels=mask.int(), keep={1}), refused(out_from_cam=T.float()), refused(image=image.float(), fns=only_cloud)       # wrong dtypes
    refused(d=depth[:, :-1].contiguous()), refused(d=depth[:, :, :-1].contiguous()), refused(d=depth.view(1, B, H, W))     # wrong shapes
    refused(d=depth.view(B, H, W, 1)), refused(cut=4), refused(s=1), refused(size=(40, 66)), refused(cut=20), refused(s=0)
    refused(k=K.expand(3, 3, 3).contiguous()), refused(out_from_cam=T.expand(3, 3, 4).contiguous()), refused(out_from_cam=T[:, :3].contiguous())
    refused(mask=mask[:1]), refused(labels=mask[:, :-1].contiguous(), keep={1}), refused(image=image[..., :2].contiguous(), fns=only_cloud)
    refused(d=depth.transpose(1, 2).contiguous().transpose(1, 2) if H != W else None)                              # not contiguous
    refused(d=torch.rand(B, 2 * H, W, device="cuda")[:, ::2]), refused(mask=torch.ones(B, H, 2 * W, dtype=torch.uint8, device="cuda")[:, :, ::2])
    refused(labels=mask), refused(keep={1}), refused(labels=mask, keep={256}), refused(labels=mask, keep=torch.ones(255, dtype=torch.uint8, device="cuda"))
    refused(labels=mask, keep=torch.ones(256, dtype=torch.uint8))                                                 # a host table
    refused(encoding="disparity"), refused(encoding=0), refused(max_depth=0.0), refused(max_depth=float("inf")), refused(min_range=float("nan"))
    for stride in (0, -1, 1.5):
        refused(stride=stride, fns=only_cloud)
    refused(fns=only_cloud, workspace=ws, out=ws.outputs(rgb=True))                                               # rgb without image
    refused(fns=only_cloud, workspace=ws, out=ws.outputs(label=True)), refused(fns=only_cloud, workspace=ws, out=ws.outputs(pixel=True))
    refused(fns=only_cloud, image=image, out=ws.out), refused(fns=only_cloud, labels=mask, keep={1}, out=ws.out)
    refused(fns=only_cloud, with_pixel=True, out=ws.out)
    refused(fns=only_cloud, out={"xyz": ws.xyz[:-1], "frame_offsets": ws.frame_offsets})                           # a row short
    refused(fns=only_cloud, out={"xyz": ws.xyz, "frame_offsets": ws.frame_offsets[:-1]})
    refused(fns=only_cloud, out={"xyz": ws.xyz.double(), "frame_offsets": ws.frame_offsets})
    refused(fns=only_cloud, out={"xyz": ws.xyz}), refused(fns=only_cloud, out={"xyz": ws.xyz, "frame_offsets": ws.frame_offsets.cpu()})
    refused(fns=(cloud.unproject_depth,), out={"points": torch.empty(B, H, W, 3, device="cuda"), "valid": torch.empty(B, H, W, device="cuda")})
    refused(fns=(cloud.unproject_depth,), out={"points": torch.empty(B, H, W, device="cuda"), "valid": mask})
    refused(fns=only_cloud, workspace=cloud.CloudWorkspace(1, SIZE, S))                                           # a workspace for fewer frames
    small = cloud.CloudWorkspace(B, SIZE, S, CUT, stride=2)
    refused(fns=only_cloud, workspace=small, out=small.out)                                                       # sized for stride 2, called with 1
    tight = cloud.CloudWorkspace(B, (2, 2 * cloud.TILE + 2), 2)
    tight.tiles = tight.tiles[:4 * B]                                                                             # one tile per frame; two are needed
    refused(d=torch.rand(B, 1, cloud.TILE + 1, device="cuda"), size=(2, 2 * cloud.TILE + 2), cut=0, fns=only_cloud, workspace=tight)
    for bad in (dict(B=0), dict(B=2, stride=0), dict(B=2, y_cutoff=20), dict(B=2, downsample_scale=0)):
        with pytest.raises(L.CrdError):
            cloud.CloudWorkspace(**dict(dict(image_size=SIZE, downsample_scale=S), **bad))
    torch.cuda.synchronize()
    assert_equal(ws.frame_offsets, marker, "frame_offsets after the refused calls")                                # nothing was launched
