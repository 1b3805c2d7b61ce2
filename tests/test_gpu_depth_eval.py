"""GPU: crd_depth_eval / camradepth_amd.metrics.DepthEval -- the standard depth-evaluation sums, binned by true distance --
against the float64 numpy restatement of their definition (tests/depth_eval_ref.py), against DepthMetrics where the two
overlap, and through Trainer.test(extended=True) and a one-rank process group."""
import dataclasses
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from camradepth_amd import synth
from tests import depth_eval_ref as ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
RTOL = 2e-5                      # the bound test_gpu_ops.py uses for crd_test_metrics against its oracle
# SILog and the mean of r = log dp - log dg (column 5 / count) are differences of nearly equal quantities: a relative bound says
# nothing about them.  Their ABSOLUTE gap to the float64 restatement was measured over seeds 0-4, both frames, caps 30 / 50 / 80 /
# 100 m of parity_inputs() (the test prints them: pytest -s); the bounds are 4x the largest gap seen:
#   largest |mean r - ref|: 1.53e-08 (seeds 0-4: 1.36e-08, 1.28e-08, 1.42e-08, 1.35e-08, 1.53e-08)
#   largest |SILog  - ref|: 1.26e-06 (seeds 0-4: 1.05e-06, 1.18e-06, 1.23e-06, 9.58e-07, 1.26e-06; SILog itself is about 17)
MEAN_R_GAP_MEASURED, SILOG_GAP_MEASURED = 1.53e-8, 1.26e-6
MEAN_R_ATOL, SILOG_ATOL = 4 * MEAN_R_GAP_MEASURED, 4 * SILOG_GAP_MEASURED
PARITY_CAPS = (30.0, 50.0, 80.0, 100.0)


def run_eval(pred, gt, **kw):
    from camradepth_amd.metrics import DepthEval
    ev = DepthEval(**kw)
    ev.update(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda())
    return ev


def parity_inputs(seed):
    """synth.make_batch(2, 256, 416, seed)'s ground truth; pred = the same distances times (1 + 0.3 u), u uniform in (-1, 1),
    re-normalised; both fp32.  Hits closer than 1e-3 * bin_width (1 cm) to a bin edge are moved 5 cm into their bin first.
    About 75 hits per batch are moved: 0.035 % of the 212992 pixels (0.17 % of the hits; two 1 cm margins per 10 m bin).
    -> pred, gt, number of hits moved."""
    gt = synth.make_batch(2, 256, 416, seed, with_seg=False)["gt_full"].numpy().copy()
    md, bw = F(100.0), F(10.0)

    def near_edge(g):
        dg = md * (F(1.0) - g)
        frac = np.mod(dg, bw)
        return dg, frac, (g > 0) & ((frac < F(1e-2)) | (frac > bw - F(1e-2)))

    dg, frac, near = near_edge(gt)
    target = np.where(frac < 5, np.floor(dg / bw) * bw + F(0.05), np.ceil(dg / bw) * bw - F(0.05))
    gt[near] = (F(1.0) - target[near] / md).astype(F)
    assert not near_edge(gt)[2].any()
    rs = np.random.RandomState(1000 + seed)
    d = 100.0 * (1.0 - gt.astype(np.float64))
    pred = (1.0 - d * (1.0 + 0.3 * rs.uniform(-1.0, 1.0, size=gt.shape)) / 100.0).astype(F)
    return pred, gt, int(near.sum())


def parity_gaps(seed, check=True):
    """Compares DepthEval with the float64 restatement on parity_inputs(seed); -> (largest |mean r| gap, largest SILog gap)."""
    pred, gt, moved = parity_inputs(seed)
    print(f"seed {seed}: {moved} of {gt.size} pixels ({int((gt > 0).sum())} hits) moved off a bin edge")
    assert moved <= 1e-3 * gt.size
    exp = ref.batch_sums(pred, gt)
    ev = run_eval(pred, gt)
    got = ev.sums()
    assert got.shape == exp.shape == (2, 10, 12)
    gap_r = gap_s = 0.0
    for f in range(2):
        frames = ev.per_frame()
        assert frames[f] is not None
        for cap in PARITY_CAPS:
            se, sg = ref.cap_sums(exp[f], cap), ref.cap_sums(got[f], cap)
            assert se[0] >= 100, (f, cap, se[0])                 # enough pixels for the bounds to mean something
            me, mg = ref.metrics(se), ev.per_frame(cap)[f]
            gr, gs = abs(sg[5] / sg[0] - se[5] / se[0]), abs(mg["SILog"] - me["SILog"])
            print(f"  frame {f} cap {cap:5.0f}: n {int(se[0]):6d}  |mean r gap| {gr:.2e}  |SILog gap| {gs:.2e}  "
                  f"rel gaps cols 1-4,7,8: {[float('%.1e' % abs(sg[c] / se[c] - 1)) for c in (1, 2, 3, 4, 7, 8)]}  "
                  f"RMSElog {abs(mg['RMSElog'] / me['RMSElog'] - 1):.1e}")
            gap_r, gap_s = max(gap_r, gr), max(gap_s, gs)
            if not check:
                continue
            for c in (0, 9, 10, 11):
                assert sg[c] == se[c], (f, cap, c)
            for c in (1, 2, 3, 4, 7, 8):
                np.testing.assert_allclose(sg[c], se[c], rtol=RTOL, err_msg=f"column {c} frame {f} cap {cap}")
            np.testing.assert_allclose(mg["RMSElog"], me["RMSElog"], rtol=RTOL)
            for k in ("MAE", "RMSE", "AbsRel", "SqRel", "iMAE", "iRMSE"):
                np.testing.assert_allclose(mg[k], me[k], rtol=RTOL, err_msg=k)
            for k in ("delta1", "delta2", "delta3"):
                assert mg[k] == me[k]
            assert gr <= MEAN_R_ATOL, (f, cap, gr)
            assert gs <= SILOG_ATOL, (f, cap, gs)
        # per-bin counts and delta columns: exact
        assert np.array_equal(got[f][:, [0, 9, 10, 11]], exp[f][:, [0, 9, 10, 11]])
    return gap_r, gap_s


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_parity_with_float64_restatement(seed):
    parity_gaps(seed)


def test_bin_edges_exact():
    """max_depth 128, bin_width 16, distances that are exact in fp32 (gt = 1 - d / 128)."""
    from camradepth_amd import lib as L
    kw = dict(max_depth=128.0, bin_width=16.0)
    min_depth = 1e-3

    def one(d, pred_d=None, pred_raw=None, **extra):
        gt = np.zeros((1, 1, 4, 8), dtype=F)
        pred = np.full_like(gt, 0.5)
        gt[0, 0, 1, 3] = F(1.0) - F(d) / F(128.0)
        assert F(128.0) * (F(1.0) - gt[0, 0, 1, 3]) == F(d)                         # dg is exact
        pred[0, 0, 1, 3] = pred_raw if pred_raw is not None else F(1.0) - F(d if pred_d is None else pred_d) / F(128.0)
        return run_eval(pred, gt, **dict(kw, **extra))

    counts = lambda ev: ev.sums()[0, :, 0].tolist()
    assert counts(one(16.0)) == [0, 1, 0, 0, 0, 0, 0, 0]                            # an edge belongs to the bin above it
    assert counts(one(15.5)) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert counts(one(127.5)) == [0, 0, 0, 0, 0, 0, 0, 1]
    assert counts(one(112.0)) == [0, 0, 0, 0, 0, 0, 0, 1]
    ev = one(32.0, pred_d=48.0)
    s = ev.sums()[0, 2]
    assert s.tolist()[:5] == [1.0, 16.0, 256.0, 0.5, 8.0] and s[9:].tolist() == [0.0, 1.0, 1.0]      # m = 1.5
    assert ev.per_frame(cap=32.0) == [None] and ev.per_frame(cap=48.0)[0]["MAE"] == 16.0
    # a hit closer than min_depth is dropped: d = 2^-11 m (exact) < 1e-3 m; at min_depth = 2^-12 it counts
    d_small = 2.0 ** -11
    assert one(d_small).per_frame() == [None]
    assert counts(one(d_small, min_depth=2.0 ** -12))[0] == 1
    # pred = 1 (distance 0) is clamped to min_depth: e = min_depth - dg
    ev = one(16.0, pred_raw=1.0)
    np.testing.assert_allclose(ev.sums()[0, 1, 1], 16.0 - float(F(min_depth)), rtol=1e-7)
    np.testing.assert_allclose(ev.sums()[0, 1, 5], math.log(float(F(min_depth))) - math.log(16.0), rtol=1e-6)
    # pred < 0 (beyond max_depth) is clamped to max_depth
    assert one(16.0, pred_raw=-0.5).sums()[0, 1, 1] == 112.0
    # pred = NaN: the partials add nothing, the sticky flag is raised, the frame reads NaN
    L.nonfinite()
    ev = one(16.0, pred_raw=float("nan"))
    assert np.isnan(ev.sums()).all() and all(math.isnan(v) for v in ev.per_frame()[0].values())
    assert L.nonfinite() is True                                                    # still reported by the status query (and cleared)
    assert L.nonfinite() is False
    # the flag belongs to the update() that raised it: a clean call afterwards reads finite numbers, also in the same DepthEval
    gt = np.zeros((2, 1, 4, 8), dtype=F)
    gt[:, 0, 2, 2] = 0.5
    clean, bad = np.full_like(gt, 0.4), np.full_like(gt, np.nan)
    from camradepth_amd.metrics import DepthEval
    ev = DepthEval(**kw)
    for p in (clean, bad, clean):
        ev.update(torch.from_numpy(p).cuda(), torch.from_numpy(gt).cuda())
    nan_frames = [math.isnan(m["MAE"]) for m in ev.per_frame()]
    assert nan_frames == [False, False, True, True, False, False]
    assert L.nonfinite() is True


def test_consistent_with_depth_metrics():
    """cap = max_depth: MAE and RMSE are what DepthMetrics reports (the inversion 100 m - d keeps differences)."""
    from camradepth_amd.metrics import DepthMetrics
    gt = synth.make_batch(2, 256, 416, 7, with_seg=False)["gt_full"].numpy()
    rs = np.random.RandomState(77)
    d = 100.0 * (1.0 - gt.astype(np.float64))
    pred = (1.0 - np.clip(d * (1.0 + 0.3 * rs.uniform(-1, 1, size=gt.shape)), 0.5, 99.5) / 100.0).astype(F)
    # the condition under which the two agree: no ground truth below min_depth, no prediction that needs a clamp
    dg, dp, valid = ref.distances(pred, gt)
    assert (valid == (gt > 0)).all() and valid.sum() > 1000
    assert (pred > 0).all() and (pred < 1).all() and (F(100.0) * (F(1.0) - pred) >= F(1e-3)).all()
    ev = run_eval(pred, gt)
    dm = DepthMetrics(100.0, 100.0)
    dm.update(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())
    for a, b in zip(ev.per_frame(cap=100.0), dm.per_frame()):
        np.testing.assert_allclose(a["MAE"], b["MAE"], rtol=RTOL)
        np.testing.assert_allclose(a["RMSE"], b["RMSE"], rtol=RTOL)
    ra, rb = ev.result(cap=100.0), dm.result()
    np.testing.assert_allclose([ra["MAE"], ra["RMSE"]], [rb["MAE"], rb["RMSE"]], rtol=RTOL)


def test_reproducible_and_independent_of_batch_order():
    from camradepth_amd.metrics import DepthEval
    pred, gt, _ = parity_inputs(11)
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    ev = DepthEval()
    ev.update(p, g)
    ev.update(p, g)
    ev.update(p.flip(0).contiguous(), g.flip(0).contiguous())
    torch.cuda.synchronize()
    a0, a1, a2 = (part[0] for part in ev._parts)
    assert a0.abs().sum() > 0 and torch.equal(a0, a1)
    assert torch.equal(a2, a0.flip(0))
    s = ev.sums()
    assert np.array_equal(s[0], s[2]) and np.array_equal(s[0], s[5]) and np.array_equal(s[1], s[4])


def test_caps_from_one_pass():
    """result(cap=50) of the binned pass = a second pass over ground truth whose hits at >= 50 m were removed beforehand."""
    pred, gt, _ = parity_inputs(12)
    dg = F(100.0) * (F(1.0) - gt)
    gt50 = np.where(dg >= F(50.0), F(0.0), gt).astype(F)
    ev, ev50 = run_eval(pred, gt), run_eval(pred, gt50)
    assert (gt50 > 0).sum() < (gt > 0).sum()
    full, cut = ev.sums(), ev50.sums()
    assert np.array_equal(full[:, :5], cut[:, :5]) and not cut[:, 5:].any() and full[:, 5:, 0].sum() > 0      # bit-equal sums
    assert cut[:, :, 0].sum() == (gt50 > 0).sum()                                                             # exact counts
    assert ev.per_frame(cap=50.0) == ev50.per_frame()
    assert ev.result(cap=50.0) == ev50.result() and ev.result(cap=50.0, pooled=True) == ev50.result(pooled=True)
    assert ev.result(cap=50.0) != ev.result()


def _check_against_ref(pred, gt, **kw):
    exp = ref.batch_sums(pred.reshape(pred.shape[0], -1), gt.reshape(gt.shape[0], -1), **{k: v for k, v in kw.items()})
    ev = run_eval(pred, gt, **kw)
    got = ev.sums()
    assert np.array_equal(got[:, :, [0, 9, 10, 11]], exp[:, :, [0, 9, 10, 11]])
    tot_g, tot_e = got.sum(axis=1), exp.sum(axis=1)
    for c in (1, 2, 3, 4, 7, 8):
        ok = tot_e[:, 0] > 0
        np.testing.assert_allclose(tot_g[ok, c], tot_e[ok, c], rtol=RTOL, err_msg=f"column {c}")
    return ev, exp


def test_shapes():
    rs = np.random.RandomState(5)

    def dense(shape):
        d = rs.uniform(1.0, 99.0, size=shape)
        gt = (1.0 - d / 100.0).astype(F)
        pred = (1.0 - d * (1.0 + 0.3 * rs.uniform(-1, 1, size=shape)) / 100.0).astype(F)
        return pred, gt

    # one full-resolution frame, every pixel valid
    pred, gt = dense((1, 1, 928, 1600))
    ev, exp = _check_against_ref(pred, gt)
    assert exp[0, :, 0].sum() == 928 * 1600 and ev.result()["delta3"] > 0.9
    # three small frames, [B,H,W] layout; the middle one has no hit at all
    pred, gt = dense((3, 24, 40))
    gt[1] = 0.0
    ev, exp = _check_against_ref(pred, gt)
    frames = ev.per_frame()
    assert frames[1] is None and frames[0] is not None and frames[2] is not None
    res = ev.result()
    for k in ("MAE", "SILog", "delta1"):
        np.testing.assert_allclose(res[k], (frames[0][k] + frames[2][k]) / 2, rtol=1e-12)
    assert run_eval(np.zeros((2, 1, 8, 8), dtype=F), np.zeros((2, 1, 8, 8), dtype=F)).result() is None
    # n neither a multiple of the workgroup's 2048 pixels nor of 4 (frames then start off a 16-byte boundary), and n just past a tile
    for shape in ((2, 1, 37, 53), (3, 1, 1, 2049), (2, 1, 1, 4100), (1, 1, 1, 1)):
        pred, gt = dense(shape)
        gt[rs.uniform(size=shape) < 0.7] = 0.0
        _check_against_ref(pred, gt)
    # other settings: 80 m in four bins of 20 m, hits closer than half a metre dropped
    pred, gt = dense((2, 1, 40, 50))
    _check_against_ref(pred * F(0.8), gt * F(0.8), max_depth=80.0, bin_width=20.0, min_depth=0.5)


def test_trainer_extended():
    from camradepth_amd.config import ModelConfig
    from camradepth_amd.metrics import DepthEval
    from camradepth_amd.model import CamRaDepth
    from camradepth_amd.params import param_specs
    from camradepth_amd.runner import Trainer
    cfg = dataclasses.replace(ModelConfig.variant("base"), depths=(1, 1, 1, 1))
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    m = CamRaDepth(input_channels=7, depths=cfg.depths)
    m.load_state_dict(sd)
    m = m.cuda().train()
    test = [synth.make_batch(2, 64, 96, seed=40 + i, with_seg=False) for i in range(3)]
    tr = Trainer(m, None, None, test)
    plain = tr.test()
    ext = tr.test(extended=True)
    assert set(plain) == {"time", "max_depth_100", "max_depth_50"}
    assert set(ext) == set(plain) | {"extended", "by_range"}
    for k in ("max_depth_100", "max_depth_50"):
        assert ext[k] == plain[k]
    assert set(ext["extended"]) == {100.0, 50.0}
    # a DepthEval driven by hand over the same predictions
    ev = DepthEval(100.0)
    m.eval()
    with torch.no_grad():
        for b in test:
            out = tr._forward_eval(b["image"].cuda())
            ev.update(out["depth"]["final_depth"], b["gt_full"].cuda())
    m.train()
    assert ev.frames() == 6
    for cap in (100.0, 50.0):
        assert ext["extended"][cap] == ev.result(cap) and set(ext["extended"][cap]) == {
            "MAE", "RMSE", "AbsRel", "SqRel", "RMSElog", "SILog", "iMAE", "iRMSE", "delta1", "delta2", "delta3"}
    assert ext["by_range"] == ev.by_range() and len(ext["by_range"]) == 10
    assert all(set(r) == {"lo", "hi", "metrics"} for r in ext["by_range"])
    other = tr.test(extended=True, caps=(80.0, 30.0, 10.0))
    assert set(other["extended"]) == {80.0, 30.0, 10.0} and other["extended"][80.0] == ev.result(80.0)
    assert other["max_depth_100"] == plain["max_depth_100"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_merge_and_all_gather_in_a_one_rank_group():
    """merge() and all_gather() in an RCCL group of one, in a fresh child process: the same numbers as a single instance."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "depth_eval_child.py"), _free_port()], capture_output=True, text=True,
                       timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["frames"] == [4, 4, 4] and res["merged_equal"] and res["gathered_equal"] and res["pooled_equal"], res
