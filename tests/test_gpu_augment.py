"""GPU: batch augmentation (camradepth_amd.batch.Augment / assemble_batch(augment=) / augment_batch, runner.Trainer(augment=)) against
the numpy restatement in tests/augment_ref.py.

The draw's integer words are exact; its float words are lo + u * (hi - lo) in fp32 without contraction, compared to 1 ulp.  The image
table is compared with a float64 evaluation (test_table_against_float64).  Given the device's own table, everything the fused assembly
and the gather write is a copy, a clamp, an IEEE division or a sign flip: compared bit for bit."""
import dataclasses

import numpy as np
import pytest
import torch

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.params import param_specs
from tests import augment_ref as ref

pytestmark = pytest.mark.gpu

PHOTO = dict(gamma=(0.9, 1.1), brightness=(0.75, 1.25), colour=(0.9, 1.1))
LEVELS = ("gt_half", "gt_quarter", "gt_eighth")
# test_table_against_float64: 4 x the largest deviation measured there (5.96e-7), and in any case below 1e-5
TABLE_BOUND = 2.4e-6


def raw_frames(B, H, W, seed, rad_vel=True, seg=True):
    """Raw buffers as the loader hands them over (numpy): random uint8 image, about 5 % non-zero radar / LiDAR points (depths past
    max_depth and below zero among them), labels 0..20 and 255."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    hit = rs.uniform(size=(B, H, W)) < 0.05
    radar = np.zeros((B, H, W, 3), dtype=np.float32)
    radar[..., 0][hit] = rs.uniform(-5.0, 120.0, size=int(hit.sum())).astype(np.float32)
    radar[..., 1][hit] = rs.normal(0, 0.4, size=int(hit.sum())).astype(np.float32)
    radar[..., 2][hit] = rs.normal(0, 0.2, size=int(hit.sum())).astype(np.float32)
    rv = (hit & (rs.uniform(size=(B, H, W)) < 0.5)).astype(np.float32) if rad_vel else None
    depth = np.where(rs.uniform(size=(B, H, W)) < 0.05, rs.uniform(-2.0, 110.0, size=(B, H, W)), 0.0).astype(np.float32)
    lab = rs.randint(0, 21, size=(B, H, W)).astype(np.uint8)
    lab[rs.uniform(size=(B, H, W)) < 0.05] = 255
    return {"img": img, "radar": radar, "rv": rv, "depth": depth, "seg": lab if seg else None}


def on_gpu(raw):
    return {k: (torch.from_numpy(v).cuda() if v is not None else None) for k, v in raw.items()}


def assemble(dev, **kw):
    from camradepth_amd.batch import assemble_batch
    return assemble_batch(dev["img"], dev["radar"], dev["rv"], dev["depth"], **kw)


def assert_same(got, want, what):
    """Bit equality of two tensors / arrays of one dtype (floats through their integer view: -0.0 != 0.0, NaN == NaN)."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = (got.view(np.int32), want.view(np.int32)) if got.dtype == np.float32 else (got, want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at {i}: {got[i]!r} against {want[i]!r}")


def table(rows, floats=None):
    """An injected table: rows of (y0, x0, flip), photometric words from `floats` [B, 5] (1.0 when None)."""
    p = np.empty((len(rows), 8), dtype=np.int32)
    p[:, :3] = rows
    p[:, 3:] = (np.ones((len(rows), 5), dtype=np.float32) if floats is None else floats.astype(np.float32)).view(np.int32)
    return p


def ulp_distance(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ----------------------------------------------------------------------------------------------------------- 1, 2: draw and table
def test_draw_against_the_restatement():
    from camradepth_amd.batch import Augment
    B, H, W, h, w = 3, 70, 101, 32, 64
    aug = Augment(crop=(h, w), hflip=0.5, seed=1234, rank=3, **PHOTO)
    for counter in (0, 5, (1 << 40) + 9):
        got = aug.draw(B, H, W, counter=counter).cpu().numpy()
        want = ref.draw(B, H, W, h, w, p=0.5, seed=1234, rank=3, counter=counter, **PHOTO)
        assert np.array_equal(got[:, :3], want[:, :3]), (counter, got[:, :3], want[:, :3])
        d = ulp_distance(ref.floats(got), ref.floats(want))
        print(f"counter {counter}: float words differ by at most {d.max()} ulp")
        assert d.max() <= 1
        assert np.array_equal(aug.draw(B, H, W, counter=counter).cpu().numpy(), got)            # the same draw twice: equal bits
        assert not np.array_equal(aug.draw(B, H, W, counter=counter + 1).cpu().numpy(), got)
    assert aug.counter == 0                                                                         # replays do not advance it
    # fixed slots on the device: one transform off, the others' words stay; no crop / flip leaves zeros
    base = aug.draw(B, H, W, counter=5).cpu().numpy()
    for off, own in (("gamma", [3]), ("brightness", [4]), ("colour", [5, 6, 7])):
        a2 = Augment(crop=(h, w), hflip=0.5, seed=1234, rank=3, **{k: v for k, v in PHOTO.items() if k != off})
        got = a2.draw(B, H, W, counter=5).cpu().numpy()
        others = [c for c in range(8) if c not in own]
        assert np.array_equal(got[:, others], base[:, others]) and (ref.floats(got)[:, [c - 3 for c in own]] == 1.0).all()
    ident = Augment(seed=1234).draw(B, H, W, counter=5).cpu().numpy()
    assert np.array_equal(ident, ref.draw(B, H, W, H, W, seed=1234, counter=5))
    # another rank, another stream
    assert not np.array_equal(Augment(crop=(h, w), hflip=0.5, seed=1234, rank=4, **PHOTO).draw(B, H, W, counter=5).cpu().numpy(), base)


def test_table_against_float64():
    """The device's fp32 chain v / 255 -> powf -> x brightness -> x colour -> clamp -> (t - mean) / std against the float64 restatement
    rounded once, over the draws of test_draw_against_the_restatement and the corners of the ranges.
    Largest absolute deviation measured on an MI355X: 5.96e-7 (2.5 ulp of the largest table values, 2.64); TABLE_BOUND = 2.4e-6 is
    4 x that, to leave room for another ROCm's powf.  One 8-bit step of the image is 1 / 255 / 0.229 = 1.7e-2."""
    from camradepth_amd.batch import Augment
    B, H, W, h, w = 3, 70, 101, 32, 64
    aug = Augment(crop=(h, w), hflip=0.5, seed=1234, rank=3, **PHOTO)
    tables = [aug.draw(B, H, W, counter=c) for c in (0, 5, (1 << 40) + 9)]
    corners = np.array([[g, b, c0, c1, c0] for g in (0.9, 1.1) for b in (0.75, 1.25) for (c0, c1) in ((0.9, 1.1), (1.1, 0.9))],
                       dtype=np.float32)
    tables.append(torch.from_numpy(table([(0, 0, 0)] * len(corners), corners)).cuda())
    worst = 0.0
    for p in tables:
        got = aug.lut(p).cpu().numpy()
        want = ref.lut(p.cpu().numpy())
        assert got.shape == want.shape == (p.shape[0], 3, 256) and np.isfinite(got).all()
        worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
    print(f"image table: largest |device - float64 restatement| = {worst:.3e} (bound {TABLE_BOUND:.3e})")
    assert worst <= TABLE_BOUND < 1e-5
    # a partly enabled chain skips the disabled steps: gamma off -> the table does not depend on word 3
    a2 = Augment(crop=(h, w), brightness=PHOTO["brightness"])
    p = tables[-1]
    assert_same(a2.lut(p)[0], a2.lut(p)[4], "table with gamma off, rows that differ in gamma only")
    got = a2.lut(p).cpu().numpy()
    want = ref.lut(p.cpu().numpy(), gamma=False, colour=False)
    assert np.abs(got.astype(np.float64) - want).max() <= TABLE_BOUND


# ----------------------------------------------------------------------------------------------------------- 3: identity
@pytest.mark.parametrize("rad_vel", [True, False])
def test_identity_configuration_keeps_the_bits(rad_vel):
    from camradepth_amd.batch import Augment, augment_batch
    B, H, W = 2, 64, 96
    dev = on_gpu(raw_frames(B, H, W, seed=3, rad_vel=rad_vel, seg=False))
    plain = assemble(dev)
    for aug in (Augment(), Augment(crop=(H, W))):
        got = assemble(dev, augment=aug)
        assert set(got) == set(plain)
        for k in plain:
            assert_same(got[k], plain[k], f"{k} (rad_vel {rad_vel})")
    assert plain["image"].shape[1] == (7 if rad_vel else 6)
    # ... and through augment_batch
    got = augment_batch(plain, Augment())
    for k in plain:
        assert_same(got[k], plain[k], f"augment_batch {k}")


# ----------------------------------------------------------------------------------------------------------- 4: fused assembly
@pytest.mark.parametrize("full", [True, False], ids=["rad_vel+labels", "plain"])
def test_fused_assembly_with_injected_tables(full):
    from camradepth_amd.batch import Augment, seg_targets
    B, H, W, h, w = 4, 70, 101, 32, 64
    raw = raw_frames(B, H, W, seed=21, rad_vel=full, seg=full)
    dev = on_gpu(raw)
    aug = Augment(crop=(h, w), hflip=0.5, seed=2, **PHOTO)
    floats = ref.floats(ref.draw(B, H, W, h, w, seed=2, counter=1, **PHOTO))
    # (0, 0); the far corner (H - h, W - w) = (38, 37), an odd column; two interior offsets with odd y0; flips 0, 1, 1, 0
    p_host = table([(0, 0, 0), (38, 37, 1), (7, 12, 1), (21, 30, 0)], floats)
    params = torch.from_numpy(p_host).cuda()
    got = assemble(dev, augment=aug, params=params, seg=dev["seg"])
    assert aug.counter == 0                                        # an injected table draws nothing
    lut = aug.lut(params).cpu().numpy()
    want = ref.assemble(raw["img"], raw["radar"], raw["rv"], raw["depth"], raw["seg"], p_host, lut, h, w)
    image = got["image"].cpu().numpy()
    assert image.shape == (B, 7 if full else 6, h, w)
    for c in range(image.shape[1]):
        assert_same(image[:, c], want["image"][:, c], f"channel {c}")
    # the mirrored u: sign changed on flipped rows only, and no negative zero anywhere
    src_u = ref.gather(np.ascontiguousarray(raw["radar"][..., 1]), p_host, h, w)
    for b, flip in enumerate((0, 1, 1, 0)):
        assert (src_u[b] != 0).sum() > 20
        assert np.array_equal(image[b, 4], -src_u[b] + 0.0 if flip else src_u[b])
    u = got["image"][:, 4]
    assert not bool(torch.signbit(u[u == 0]).any())
    assert_same(got["gt_full"], want["gt_full"], "gt_full")
    assert float(got["gt_full"].max()) < 1.0 and float(got["gt_full"].min()) == 0.0
    # the pyramid: the host min-pool of the AUGMENTED full map (and not the cropped / flipped levels of the source frame)
    cur = got["gt_full"].cpu()
    for name, lvl in zip(LEVELS, ref.pyramid(want["gt_full"], 3)):
        cur = synth.min_pool_ignore_zero(cur)
        assert_same(got[name], lvl, name)
        assert_same(got[name], cur, name + " (torch min-pool)")
    if full:
        assert_same(got["final_seg"], want["final_seg"], "final_seg")
        assert_same(got["intermediate_seg"], want["intermediate_seg"], "intermediate_seg")
        assert got["seg"] is got["final_seg"] and got["final_seg"].dtype == torch.int64
        # the rule of seg_targets on the augmented final map
        st = seg_targets(got["final_seg"].to(torch.uint8), rows=h, sizes=((h, w), (h // 2, w // 2)))
        assert_same(got["intermediate_seg"], st["intermediate_seg"], "intermediate_seg against seg_targets")
        assert int((got["final_seg"] == 255).sum()) > 0
    else:
        assert "final_seg" not in got and "seg" not in got
    # out-of-range offsets in a table are clamped into the frame, never followed
    wild = torch.from_numpy(table([(-5, -9, 0), (1000, 1000, 1), (38, 37, 1), (0, 0, 0)], floats)).cuda()
    tame = torch.from_numpy(table([(0, 0, 0), (38, 37, 1), (38, 37, 1), (0, 0, 0)], floats)).cuda()
    a, b = assemble(dev, augment=aug, params=wild), assemble(dev, augment=aug, params=tame)
    assert_same(a["image"], b["image"], "clamped offsets")


# ----------------------------------------------------------------------------------------------------------- 5: live = injected
def test_live_draw_equals_injected_table():
    from camradepth_amd.batch import Augment
    B, H, W, h, w = 4, 70, 101, 32, 64
    dev = on_gpu(raw_frames(B, H, W, seed=33))
    aug = Augment(crop=(h, w), hflip=0.5, seed=77, rank=1, **PHOTO)
    aug.counter = 6
    live = assemble(dev, augment=aug, seg=dev["seg"])
    assert aug.counter == 7
    params = aug.draw(B, H, W, counter=6)
    assert aug.counter == 7
    want = ref.draw(B, H, W, h, w, p=0.5, seed=77, rank=1, counter=6, **PHOTO)
    assert np.array_equal(params.cpu().numpy()[:, :3], want[:, :3])
    injected = assemble(dev, augment=aug, params=params, seg=dev["seg"])
    assert set(live) == set(injected)
    for k in live:
        assert_same(live[k], injected[k], k)
    nxt = assemble(dev, augment=aug, seg=dev["seg"])                   # counter 7: another draw
    assert aug.counter == 8 and not torch.equal(nxt["image"], live["image"])
    # state_dict carries the counter: a restored object replays draw 7
    other = Augment(crop=(h, w), hflip=0.5, seed=77, rank=1, **PHOTO)
    other.load_state_dict({"counter": 7})
    assert_same(assemble(dev, augment=other, seg=dev["seg"])["image"], nxt["image"], "resumed draw")


# ----------------------------------------------------------------------------------------------------------- 6: the two paths commute
def test_gather_of_assembled_equals_fused_assembly():
    from camradepth_amd.batch import Augment, augment_batch
    B, H, W, h, w = 2, 64, 96, 32, 64
    dev = on_gpu(raw_frames(B, H, W, seed=44))
    aug = Augment(crop=(h, w), hflip=0.5, seed=9)
    params = torch.from_numpy(table([(13, 32, 1), (32, 5, 0)])).cuda()
    fused = assemble(dev, augment=aug, params=params, seg=dev["seg"])
    whole = assemble(dev, seg=dev["seg"])                               # no augmentation, labels through the same entry
    assert whole["image"].shape == (B, 7, H, W) and whole["intermediate_seg"].shape == (B, H // 2, W // 2)
    two_step = augment_batch(whole, aug, params=params)
    assert set(two_step) == set(fused) and aug.counter == 0
    for k in fused:
        assert_same(two_step[k], fused[k], k)
    # live draw through augment_batch: the restatement's gather on the host
    aug.counter = 3
    live = augment_batch(whole, aug)
    p = ref.draw(B, H, W, h, w, p=0.5, seed=9, counter=3)
    assert aug.counter == 4
    assert_same(live["image"], ref.mirror_u(ref.gather(whole["image"].cpu().numpy(), p, h, w), p), "augment_batch live")
    # a 3-channel (RGB-only) batch has no uv channels: nothing is negated; unknown keys pass through
    rgb = {"image": whole["image"][:, :3], "gt_full": whole["gt_full"], "gt_half": whole["gt_half"], "name": ["a", "b"]}
    got = augment_batch(rgb, aug, params=params)
    p_host = params.cpu().numpy()
    assert_same(got["image"], ref.gather(whole["image"][:, :3].cpu().numpy(), p_host, h, w), "RGB-only image")
    assert got["name"] == ["a", "b"] and set(got) == set(rgb)
    assert_same(got["gt_half"], fused["gt_half"], "gt_half of the RGB-only batch")
    # a 5-channel image likewise (C < 6): channel 4 is not u
    five = augment_batch({"image": whole["image"][:, :5], "gt_full": whole["gt_full"]}, aug, params=params)
    assert_same(five["image"], ref.gather(whole["image"][:, :5].cpu().numpy(), p_host, h, w), "5-channel image")
    # host tensors are moved to the device (what the Trainer hands over)
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in whole.items()}
    moved = augment_batch(cpu, aug, params=params)
    assert moved["image"].is_cuda
    assert_same(moved["image"], fused["image"], "host batch")


# ----------------------------------------------------------------------------------------------------------- 7: Trainer
def test_trainer_augments_training_batches_only():
    from camradepth_amd.batch import Augment
    from camradepth_amd.model import CamRaDepth
    from camradepth_amd.runner import Trainer
    cfg = dataclasses.replace(ModelConfig.variant("supervised_seg"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    train = [synth.make_batch(B, 64, 96, seed=10 + i) for i, B in enumerate((2, 2, 1))]          # a ragged last batch
    val = [synth.make_batch(2, 64, 96, seed=30)]

    def run(augment):
        m = CamRaDepth(input_channels=7, depths=cfg.depths, supervised_seg=True)
        m.load_state_dict(sd)
        tr = Trainer(m.cuda().train(), train, val, None, learning_rate=1e-3, num_epochs=1, update_interval=2, augment=augment)
        r = tr.train_one_epoch(0)
        torch.cuda.synchronize()
        return tr, r

    tr, r = run(Augment(crop=(32, 64), hflip=0.5, seed=7))
    assert set(tr._steps) == {(2, 32, 64), (1, 32, 64)}
    assert all((ts.H, ts.W) == (32, 64) and ts.state is tr._train_state for ts in tr._steps.values())
    assert tr.augment.counter == 3 and tr._train_state.iter_count == 3
    assert all(np.isfinite(v) for v in r.values()), r
    val_loss, rmse = tr.eval(0)
    assert set(tr._infer) == {(2, 64, 96)} and np.isfinite(val_loss) and rmse > 0            # eval() never augments
    assert tr.augment.counter == 3
    tr2, r2 = run(Augment(crop=(32, 64), hflip=0.5, seed=7))
    assert r2 == r, (r, r2)
    assert torch.equal(tr2.model.flat, tr.model.flat)
    tr3, r3 = run(None)
    assert set(tr3._steps) == {(2, 64, 96), (1, 64, 96)} and tr3.augment is None and all(np.isfinite(v) for v in r3.values())
