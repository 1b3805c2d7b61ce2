"""GPU: the visualisation back end (camradepth_amd.viz) against the NumPy restatement in tests/viz_ref.py, run on the host copy of the
same inputs.  Every comparison is torch.equal: the arithmetic is specified operation by operation (include/camradepth_hip.h) and
tests/test_viz_ref_cpu.py holds the restatement to matplotlib, so a picture either has the restatement's bytes or is wrong."""
import numpy as np
import pytest
import torch

from tests import viz_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 77


@pytest.fixture(scope="module")
def viz():
    from camradepth_amd import viz as module
    return module


def tables():
    from camradepth_amd._viz_tables import TABLES
    return {k: np.frombuffer(v, dtype=np.uint8).reshape(256, 3) for k, v in TABLES.items()}


def shapes():
    """(B, h, w): one pixel; odd; w no multiple of 4 with several rows and frames; exactly two workgroups' share of the range pass per
    frame; one share and a bit with w no multiple of 4; a frame of a multiple of 4 pixels whose rows are not."""
    from camradepth_amd.viz import TILE
    return [(1, 1, 1), (2, 5, 7), (3, 33, 130), (2, 2, TILE), (1, 3, TILE // 3 + 2), (2, 4, 9)]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_same(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} values differ; first at {i}: {got[i].item()!r} against {want[i].item()!r}")


def float_maps(rs, B, h, w):
    n = B * h * w
    maps = {"random": rs.standard_normal(size=n), "sparse": rs.standard_normal(size=n) * (rs.uniform(size=n) >= 0.7),
            "scaled": rs.standard_normal(size=n) * 100, "constant": np.full(n, 3.25), "zeros": np.zeros(n)}
    lo, span = F(0.1), F(0.6)
    maps["bin boundaries"] = lo + (np.arange(n) % 257).astype(F) / F(256) * span                    # per frame: the same rows of the table
    maps["bin boundaries 0..1"] = (rs.permutation(n) % 257).astype(F) / F(256)
    special = rs.standard_normal(size=n).astype(F)
    kind = rs.randint(0, 12, size=n)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -3e-39, 1e-38)):
        special[kind == k] = v
    maps["non-finite, -0.0 and subnormals"] = special
    maps["subnormals only"] = (rs.randint(-40, 40, size=n) * 1e-45).astype(F)
    maps["-0.0 and 0.0"] = np.where(rs.uniform(size=n) < 0.5, F(-0.0), F(0.0))
    out = {k: np.ascontiguousarray(v, dtype=F).reshape(B, h, w) for k, v in maps.items()}
    if B > 1:
        per_frame = out["random"].copy()
        per_frame[0] = np.nan                                                                    # an all-NaN frame next to normal ones
        per_frame[-1] *= F(7)
        out["ranges are per frame"] = per_frame
    return out


def check_float_maps(viz, B, h, w, seed, names=None):
    jet = tables()["jet"]
    rs = np.random.RandomState(seed)
    for name, m in float_maps(rs, B, h, w).items():
        if names is not None and name not in names:
            continue
        x = cuda(m)
        assert_same(viz.colorize(x, bad_colour=(9, 200, 30)), ref.colorize(m, jet, bad_colour=(9, 200, 30)), f"{(B, h, w)} {name}")
        rng = viz.frame_range(x)
        assert_same(rng, ref.frame_range(m), f"{(B, h, w)} {name}: frame_range")
        finite = m[np.isfinite(m)]
        if finite.size:                                                                          # fixed range: as floats and as a device tensor
            lo, hi = F(np.quantile(finite, 0.2)), F(np.quantile(finite, 0.9))                    # values below, at and above the ends
            want = ref.colorize(m, jet, lo, hi)
            assert_same(viz.colorize(x, vmin=float(lo), vmax=float(hi)), want, f"{(B, h, w)} {name}: fixed range")
            fixed = torch.tensor([[lo, hi]] * B, dtype=torch.float32, device="cuda")
            assert_same(viz.colorize(x, vmin=fixed), want, f"{(B, h, w)} {name}: fixed range on the device")
            assert_same(viz.colorize(x.unsqueeze(1), "rainbow", vmin=rng), ref.colorize(m, tables()["rainbow"]), f"{(B, h, w)} {name}: own range passed back")


@pytest.mark.parametrize("case", range(6))
def test_float_maps(viz, case):
    check_float_maps(viz, *shapes()[case], seed=100 + case)


def test_float_map_at_full_resolution(viz):
    check_float_maps(viz, 1, 416, 800, seed=110, names=("sparse", "non-finite, -0.0 and subnormals", "bin boundaries"))


def test_x_equal_vmax_and_the_ends_of_a_fixed_range(viz):
    jet = tables()["jet"]
    m = np.array([[[-2.0, -1.0, -0.999, 0.0, 0.5, 2.999, 3.0, 3.001, 7.0, np.nan]]], dtype=F)
    for lo, hi in ((-1.0, 3.0), (0.0, 0.5), (-5.0, 10.0), (0.25, 0.25), (7.0, 7.0)):
        assert_same(viz.colorize(cuda(m), vmin=lo, vmax=hi), ref.colorize(m, jet, lo, hi), f"fixed range {lo} .. {hi}")
    got = viz.colorize(cuda(m)).cpu().numpy()[0, 0]
    assert got[8].tolist() == jet[255].tolist() and got[0].tolist() == jet[0].tolist() and got[9].tolist() == [0, 0, 0]
    custom = np.random.RandomState(3).randint(0, 256, size=(256, 3)).astype(np.uint8)              # the caller's own table
    assert_same(viz.colorize(cuda(m), cmap=cuda(custom)), ref.colorize(m, custom), "custom table")


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_labels(viz, case):
    B, h, w = shapes()[case]
    rainbow = tables()["rainbow"]
    rs = np.random.RandomState(120 + case)
    n = B * h * w
    with_ignore = rs.randint(0, 21, size=n)
    with_ignore[rs.uniform(size=n) < 0.05] = 255
    cases = {"0..20": rs.randint(0, 21, size=n), "0..20 and 255": with_ignore, "one value": np.full(n, 7), "all 256": np.arange(n) % 256,
             "zeros": np.zeros(n)}
    for name, lab in cases.items():
        lab = lab.astype(np.uint8).reshape(B, h, w)
        x = cuda(lab)
        assert_same(viz.colorize_labels(x), ref.colorize(lab, rainbow), f"{(B, h, w)} {name}")
        assert_same(viz.frame_range(x), ref.frame_range(lab), f"{(B, h, w)} {name}: frame_range")
        assert_same(viz.colorize_labels(x, "jet", vmin=0, vmax=20), ref.colorize(lab, tables()["jet"], 0, 20), f"{(B, h, w)} {name}: fixed range")
        assert_same(viz.colorize_labels(x, vmin=0.5, vmax=19.25), ref.colorize(lab, rainbow, 0.5, 19.25), f"{(B, h, w)} {name}: fractional range")


@pytest.mark.parametrize("C", [1, 2, 21, 256])
def test_seg_labels(viz, C):
    rs = np.random.RandomState(130 + C)
    for B, h, w in ((2, 5, 7), (1, 33, 130), (2, 4, 9), (1, 2, viz.TILE + 4)):
        x = rs.standard_normal(size=(B, C, h, w)).astype(F)
        x = np.round(x * 2) / 2                                                                  # ties: the first maximum wins
        if C > 1:
            x[0, :, 0, 0] = 1.0
            x[0, 1, 1, 1] = np.nan                                                               # a NaN beats everything
            x[B - 1, C - 1, h - 1, w - 1] = np.nan
            x[B - 1, 0, h - 1, w - 1] = np.inf
            x[0, :, 1, 3] = np.nan                                                               # the first NaN wins
            x[0, :, 1, 2] = -np.inf
            x[0, C // 2, :, w // 2] = np.nan                                                     # a NaN channel down one column
        want = ref.seg_labels(x)
        assert np.array_equal(want, np.argmax(x, axis=1).astype(np.uint8))
        assert_same(viz.seg_labels(cuda(x)), want, f"C {C}, {(B, h, w)}")
    out = torch.full((2, 5, 7), SENTINEL, dtype=torch.uint8, device="cuda")
    x = rs.standard_normal(size=(2, C, 5, 7)).astype(F)
    assert viz.seg_labels(cuda(x), out=out).data_ptr() == out.data_ptr()
    assert_same(out, ref.seg_labels(x), "out=")


def radar_maps(rs, B, h, w):
    r = np.zeros((B, h, w), dtype=F)
    k = max(1, h * w // 40)
    for b in range(B - 1 if B > 1 else B):                                                       # the last of several frames stays empty
        r[b, rs.randint(0, h, size=k), rs.randint(0, w, size=k)] = rs.uniform(0.02, 1.0, size=k).astype(F)
    r[0, 0, 0], r[0, h - 1, w - 1], r[0, 0, w - 1], r[0, h - 1, 0] = 0.5, 0.25, 0.75, 0.125         # corners
    r[0, h // 2, 0], r[0, 0, w // 2] = 0.3, 0.6                                                  # borders
    if w > 4:
        r[0, h // 2, w // 2], r[0, h // 2, w // 2 + 1], r[0, h // 2, w // 2 - 2] = 0.2, 0.9, 1.0   # adjacent returns; r == 1 vanishes
        r[0, h - 1, w // 2] = 1.5                                                                 # r > 1: negative, never pasted
        r[0, 0, 2], r[0, 0, 3] = np.nan, np.inf                                                   # no return
    return r


@pytest.mark.parametrize("case", range(6))
def test_radar_panel(viz, case):
    B, h, w = shapes()[case]
    jet = tables()["jet"]
    rs = np.random.RandomState(140 + case)
    r = radar_maps(rs, B, h, w)
    image = rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)
    for k in (1, 5, 9):
        for order in ("bgr", "rgb"):
            assert_same(viz.radar_overlay(cuda(image), cuda(r), dilate=k, image_order=order), ref.radar_overlay(image, r, jet, k, order),
                        f"{(B, h, w)} dilate {k} {order}")
    ws = viz.VizWorkspace(B, h, w)
    viz.radar_overlay(cuda(image), cuda(r), dilate=3, workspace=ws)
    assert_same(ws.dilated, ref.dilate(ref.radar_transform(r), 3), "the dilated map")
    assert_same(ws.range, ref.frame_range(ref.dilate(ref.radar_transform(r), 3)), "the dilated map's range")
    if B > 1:
        empty = ref.radar_overlay(image, r, jet, 5)[-1]
        assert np.array_equal(empty, ref.grey(ref.to_rgb(image[-1])))                             # an empty frame is the grey image


@pytest.mark.parametrize("case", [1, 2, 4])
def test_paste_and_blend(viz, case):
    B, h, w = shapes()[case]
    jet = tables()["jet"]
    rs = np.random.RandomState(150 + case)
    gt = rs.uniform(0.01, 0.99, size=(B, h, w)).astype(F) * (rs.uniform(size=(B, h, w)) < 0.2)
    gt[0, 0, 0], gt[0, -1, -1] = -0.5, np.nan
    depth = rs.uniform(size=(B, h, w)).astype(F)
    labels = rs.randint(0, 4, size=(B, h, w)).astype(np.uint8)
    image = rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)
    image[0, 0, :min(w, 4)] = np.array([[0, 0, 0], [255, 255, 255], [2, 2, 2], [1, 3, 5]], dtype=np.uint8)[:min(w, 4)]
    for order in ("bgr", "rgb"):
        assert_same(viz.overlay(cuda(image), cuda(gt), "paste", image_order=order), ref.overlay(image, gt, jet, "paste", image_order=order),
                    f"paste {order}")
        assert_same(viz.overlay(cuda(image), cuda(labels), "paste", cmap="rainbow", image_order=order),
                    ref.overlay(image, labels, tables()["rainbow"], "paste", image_order=order), f"paste of labels {order}")
        # 0.5 / 0.25 and 1.5 / 0.5 land on exact halves, 0.8 / 0.75 and 1.5 / 1.0 go beyond 255, negative weights below 0
        for alpha, beta in ((0.8, 0.75), (0.5, 0.25), (1.5, 0.5), (1.5, 1.0), (-1.0, 0.5), (0.0, 1.0), (1.0, 0.0)):
            want = ref.overlay(image, depth, jet, "blend", alpha, beta, image_order=order)
            assert_same(viz.overlay(cuda(image), cuda(depth), "blend", alpha, beta, image_order=order), want, f"blend {alpha} {beta} {order}")
        assert_same(viz.image_rgb(cuda(image), order), ref.to_rgb(image, order), f"image {order}")
        assert_same(viz.image_rgb(cuda(image), order, grey=True), ref.grey(ref.to_rgb(image, order)), f"grey image {order}")
    halves = ref.to_rgb(image).astype(F) * F(0.5) + ref.colorize(depth, jet).astype(F) * F(0.25)
    assert (halves % 1 == 0.5).any() and (ref.to_rgb(image).astype(F) * F(0.8) + ref.colorize(depth, jet).astype(F) * F(0.75) > 255.5).any()
    assert_same(viz.overlay(cuda(image), cuda(gt), "blend", vmin=0.0, vmax=1.0, bad_colour=(255, 0, 255)),
                ref.overlay(image, gt, jet, "blend", vmin=0.0, vmax=1.0, bad_colour=(255, 0, 255)), "blend, fixed range, bad colour")


@pytest.mark.parametrize("case", [1, 2, 3, 5])
def test_strided_out_writes_its_panel_and_nothing_else(viz, case):
    """The panels of a 2 x 3 canvas equal the stand-alone calls; the canvas outside them keeps its bytes."""
    B, h, w = shapes()[case]
    rs = np.random.RandomState(160 + case)
    depth = rs.uniform(size=(B, h, w)).astype(F)
    labels = rs.randint(0, 21, size=(B, h, w)).astype(np.uint8)
    radar = radar_maps(rs, B, h, w)
    image = cuda(rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8))
    # a margin row and four margin columns: where w is a multiple of 4 the pitches stay multiples of 4 and the dword stores are taken
    canvas = torch.full((B, 2 * h + 1, 3 * w + 4, 3), SENTINEL, dtype=torch.uint8, device="cuda")

    def panel(i, j):
        return canvas[:, i * h:(i + 1) * h, j * w:(j + 1) * w]

    alone = {(0, 0): viz.image_rgb(image), (0, 1): viz.colorize_labels(cuda(labels)), (1, 0): viz.colorize(cuda(depth)),
             (1, 1): viz.overlay(image, cuda(depth), "blend"), (1, 2): viz.radar_overlay(image, cuda(radar))}
    viz.image_rgb(image, out=panel(0, 0))
    viz.colorize_labels(cuda(labels), out=panel(0, 1))
    viz.colorize(cuda(depth), out=panel(1, 0))
    viz.overlay(image, cuda(depth), "blend", out=panel(1, 1))
    viz.radar_overlay(image, cuda(radar), out=panel(1, 2))
    want = torch.full_like(canvas, SENTINEL).cpu()
    for (i, j), p in alone.items():
        want[:, i * h:(i + 1) * h, j * w:(j + 1) * w] = p.cpu()
    assert torch.equal(canvas.cpu(), want)
    assert (canvas[:, :h, 2 * w:3 * w] == SENTINEL).all() and (canvas[:, 2 * h:] == SENTINEL).all() and (canvas[:, :, 3 * w:] == SENTINEL).all()
    from camradepth_amd import lib as L
    for bad in (canvas[:, :h, :w, :2], canvas[:, :h, :2 * w:2], canvas[:, :h, :w].float(), canvas[:, :h - 1, :w] if h > 1 else canvas[:1, :, :w],
                canvas[:, :h, :w].cpu()):
        with pytest.raises(L.CrdError):
            viz.colorize(cuda(depth), out=bad)


def test_two_runs_give_the_same_bits(viz):
    rs = np.random.RandomState(170)
    B, h, w = 3, 33, 130
    m = float_maps(rs, B, h, w)["non-finite, -0.0 and subnormals"]
    image, radar = cuda(rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)), cuda(radar_maps(rs, B, h, w))
    logits = cuda(np.round(rs.standard_normal(size=(B, 21, h, w)) * 2).astype(F))

    def run():
        return (viz.colorize(cuda(m)), viz.frame_range(cuda(m)).view(torch.int32), viz.overlay(image, cuda(m), "blend"), viz.radar_overlay(image, radar),
                viz.seg_labels(logits), viz.colorize_labels(viz.seg_labels(logits)))

    first, second = run(), run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_workspace_no_allocation_and_capture(viz):
    """With workspace= and out= a call is kernel launches only: nothing is allocated, and a graph captured on a side stream replays
    with a changed map in the same buffer and draws the changed picture, its range read on the device."""
    jet = tables()["jet"]
    rs = np.random.RandomState(180)
    B, h, w = 2, 33, 130
    maps = {"first": rs.uniform(size=(B, h, w)).astype(F), "wider": (rs.standard_normal(size=(B, h, w)) * 50).astype(F),
            "with NaN": float_maps(rs, B, h, w)["non-finite, -0.0 and subnormals"]}
    image_np = rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)
    radar_np = radar_maps(rs, B, h, w)
    x, image, radar = cuda(maps["first"]).unsqueeze(1), cuda(image_np), cuda(radar_np)               # [B,1,h,w], as final_depth
    ws = viz.VizWorkspace(B, h, w)
    outs = [torch.empty(B, h, w, 3, dtype=torch.uint8, device="cuda") for _ in range(3)]

    def call():
        viz.colorize(x, out=outs[0], workspace=ws)
        viz.overlay(image, x, "blend", vmin=ws.range, out=outs[1], workspace=ws)
        viz.radar_overlay(image, radar, out=outs[2], workspace=ws)

    def check(which):
        torch.cuda.synchronize()
        assert_same(outs[0], ref.colorize(maps[which], jet), f"{which}: colorize")
        assert_same(outs[1], ref.overlay(image_np, maps[which], jet, "blend"), f"{which}: blend")
        assert_same(outs[2], ref.radar_overlay(image_np, radar_np, jet), f"{which}: radar")

    call()                                                                                       # eager once: the code objects are loaded before the capture
    check("first")
    before, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    call()
    assert torch.cuda.memory_allocated() == before and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                                    # captures on a side stream
        call()
    for which in ("wider", "with NaN", "first"):
        x.copy_(cuda(maps[which]).unsqueeze(1))
        for o in outs:
            o.fill_(SENTINEL)
        g.replay()
        check(which)
    from camradepth_amd import lib as L
    with pytest.raises(L.CrdError):                                                              # a workspace for fewer pixels
        viz.colorize(x, workspace=viz.VizWorkspace(B, h, w - 100))
    with pytest.raises(L.CrdError):
        viz.radar_overlay(image, radar, workspace=viz.VizWorkspace(1, h, w))


def small_model(**kw):
    from camradepth_amd.model import CamRaDepth
    return CamRaDepth(input_channels=7, depths=(1, 1, 1, 1), **kw).cuda().eval()


def hand_made(batch, image, pred, heads):
    """Visualizer.render's pictures composed from the restatement."""
    t = tables()
    depth = pred["depth"]["final_depth"][:, 0].cpu().numpy()
    seg = batch["seg"].numpy().astype(np.uint8)
    want = {"depth_pred": ref.colorize(depth, t["jet"]), "depth_on_rgb": ref.overlay(image, depth, t["jet"], "blend"),
            "lidar_gt": ref.overlay(image, batch["gt_full"][:, 0].numpy(), t["jet"], "paste"), "seg": ref.colorize(seg, t["rainbow"]),
            "radar": ref.radar_overlay(image, batch["image"][:, 3].numpy(), t["jet"], 5)}
    if heads:
        want["pred_seg"] = ref.colorize(ref.seg_labels(pred["seg"]["final_seg"].cpu().numpy()), t["rainbow"])
        want["unsup"] = ref.colorize(pred["seg"]["unsup_map"][:, 0].cpu().numpy(), t["jet"])
    B, h, w = depth.shape
    panels = {(0, 0): ref.to_rgb(image), (0, 1): want["seg"], (1, 0): want["depth_pred"], (1, 1): want["lidar_gt"],
              (1, 2): want["unsup"] if heads else want["depth_on_rgb"]}
    if heads:
        panels[(0, 2)] = want["pred_seg"]
    want["collage"] = ref.collage(panels, B, h, w)
    return want


@pytest.mark.parametrize("heads", [False, True])
def test_visualizer_render_behind_the_inference_graph(viz, heads):
    """INTEGRATION.md's worked example: InferenceGraph.run(x, clone=False) returns views of static buffers; render() is captured once on
    them and replayed behind every frame.  Every picture equals the restatement composed by hand; the base model has no 'pred_seg' and
    no 'unsup', the model with both segmentation heads has them."""
    from camradepth_amd import synth
    from camradepth_amd.inference import InferenceGraph
    B, h, w = 2, 64, 96
    model = small_model(supervised_seg=True, unsupervised_seg=True) if heads else small_model()
    ig = InferenceGraph(model, B, h, w)
    batches = [synth.make_batch(B, h, w, seed=s) for s in (5, 6)]
    rs = np.random.RandomState(190)
    image_np = rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)
    x, image = batches[0]["image"].cuda(), cuda(image_np)
    gt, seg = batches[0]["gt_full"].cuda(), batches[0]["seg"].to(torch.uint8).cuda()
    pred = ig.run(x, clone=False)
    vz = viz.Visualizer(B, h, w)
    got = vz.render(image, x, pred, gt_full=gt, seg=seg)                                         # eager once
    names = {"depth_pred", "depth_on_rgb", "lidar_gt", "seg", "radar", "collage"} | ({"pred_seg", "unsup"} if heads else set())
    assert set(got) == names and set(got) <= set(viz.PANELS)
    assert got["collage"].shape == (B, 2 * h, 3 * w, 3) and got["depth_pred"].data_ptr() == vz.panel(1, 0).data_ptr()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    vz.render(image, x, pred, gt_full=gt, seg=seg)
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vz.render(image, x, pred, gt_full=gt, seg=seg)
    seen = []
    for batch in batches:
        x.copy_(batch["image"].cuda()), gt.copy_(batch["gt_full"].cuda()), seg.copy_(batch["seg"].to(torch.uint8).cuda())
        again = ig.run(x, clone=False)
        g.replay()
        torch.cuda.synchronize()
        assert again["depth"]["final_depth"].data_ptr() == pred["depth"]["final_depth"].data_ptr()
        want = hand_made(batch, image_np, again, heads)
        assert set(want) == names
        for k in sorted(names):
            assert_same(got[k], want[k], f"heads {heads}: {k}")
        seen.append(got["collage"].clone())
    assert not torch.equal(seen[0], seen[1])                                                     # the second frame's pictures, not the first's again
    # without the optional inputs their pictures are left out and their panels stay black
    plain = viz.Visualizer(B, h, w, image_order="rgb").render(image, None, pred)
    assert set(plain) == {"depth_pred", "depth_on_rgb", "collage"} | ({"pred_seg", "unsup"} if heads else set())
    assert not plain["collage"][:, :h, w:2 * w].any() and not plain["collage"][:, h:, w:2 * w].any()
    assert_same(plain["collage"][:, :h, :w], image_np, "the image panel, rgb order")
