"""CPU checks of the depth-criterion zoo (MaskedL1Loss, MaskedHuberLoss, MaskedRMSELoss, MaskedBerHuLoss, SmoothnessLoss):
the reference-pinned fixture against an independent fp64 statement of every formula, the generator's reproducibility, the
criteria TrainStep refuses, and -- gloo world 2 with CPU stand-ins for the HIP graphs -- where the collectives of a BerHu step
run.  The kernels themselves are checked on the GPU (tests/test_gpu_loss_zoo.py)."""
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.loss_zoo_cases import CASES, depth_pair, grad_view, smooth_pair
from tests.util import load_npz

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(REPO, "tests", "golden", "make_loss_zoo_golden.py")


# ---- independent fp64 statements of the formulas (the issue's table; not the reference's code) -----------------------------
def f64_depth(name, pred, target, thresh=0.2):
    m = target > 0
    d = (pred - target)[m]
    ad = d.abs()
    if name == "l1":
        return ad.mean()
    if name == "huber":                                  # delta = 1
        return torch.where(ad < 1, 0.5 * d * d, ad - 0.5).mean()
    if name == "rmse":
        return torch.sqrt((d * d).mean())
    if name == "berhu":
        # c is a constant of the backward; the edges are the reference's fp32 comparisons: |d| against fp32(c), and fp32(|d|^2)
        # (rounded before the subtraction) against fp32(c^2)
        c = thresh * float(ad.max())
        ad32 = ad.float()
        lin_on = ad32 < np.float32(c)
        quad_on = ~lin_on & ((ad32 * ad32) - np.float32(c * c) > 0)
        lin = torch.where(lin_on, ad, torch.zeros_like(ad))
        quad = torch.where(quad_on, d * d, torch.zeros_like(ad)) / (2 * c)
        return (lin + quad).mean()
    raise ValueError(name)


def f64_smooth(pred, image):
    n = pred / (pred.mean(dim=(2, 3), keepdim=True) + 1e-7)
    wx = torch.exp(-(image[..., :, 1:] - image[..., :, :-1]).abs().mean(1, keepdim=True))
    wy = torch.exp(-(image[..., 1:, :] - image[..., :-1, :]).abs().mean(1, keepdim=True))
    return ((n[..., :, 1:] - n[..., :, :-1]).abs() * wx).mean() + ((n[..., 1:, :] - n[..., :-1, :]).abs() * wy).mean()


def f64_case(case, name):
    """-> (loss, gradient as stored in the fixture) of the fp64 statement on the case's inputs."""
    if name == "smooth":
        p, im = smooth_pair(case)
        x = torch.from_numpy(p).double().requires_grad_(True)
        loss = f64_smooth(x, torch.from_numpy(im).double())
    else:
        p, t = depth_pair(case)
        x = torch.from_numpy(p).double().requires_grad_(True)
        loss = f64_depth(name, x, torch.from_numpy(t).double())
    loss.backward()
    return float(loss.detach()), grad_view(case, x.grad.numpy())


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ["l1", "huber", "rmse", "berhu", "smooth"])
def test_fixture_matches_fp64_statement(case, name):
    g = load_npz("loss_zoo.npz")
    p, t = depth_pair(case)
    np.testing.assert_array_equal(g[f"{case}__inputs_sum"], [p.astype(np.float64).sum(), t.astype(np.float64).sum()])
    loss, grad = f64_case(case, name)
    ref_loss, ref_grad = float(g[f"{case}__{name}__loss"]), g[f"{case}__{name}__grad"]
    if np.isnan(ref_loss):
        assert np.isnan(loss), (case, name, loss)
    else:
        assert loss == pytest.approx(ref_loss, rel=1e-6, abs=1e-7), (case, name)
    assert grad.shape == ref_grad.shape
    np.testing.assert_array_equal(np.isnan(grad), np.isnan(ref_grad))
    ok = ~np.isnan(ref_grad)
    scale = float(np.abs(ref_grad[ok]).max()) if ok.any() else 0.0
    np.testing.assert_allclose(grad[ok], ref_grad[ok], rtol=1e-4, atol=1e-5 * scale + 1e-12)


def test_fixture_edge_cases():
    """The pinned edges: BerHu is NaN at c = 0 with a zero gradient, |d| == c contributes nothing, d = 0 gets no gradient;
    RMSE's gradient is NaN on the mask when every d is 0."""
    g = load_npz("loss_zoo.npz")
    assert np.isnan(g["equal__berhu__loss"]) and not np.any(g["equal__berhu__grad"])
    p, t = depth_pair("equal")
    gr = g["equal__rmse__grad"].reshape(t.shape)
    assert np.isnan(gr[t > 0]).all() and not np.any(gr[t <= 0])
    p, t = depth_pair("edge")
    at_c = (t > 0) & (np.abs(p - t) == 1.0)
    assert at_c.sum() >= 16 and not np.any(g["edge__berhu__grad"].reshape(p.shape)[at_c])
    p, t = depth_pair("edge_f32")                      # fp32(c)^2 != fp32(c^2): an FMA would move these elements into part 2
    c = 0.2 * float(np.abs(p - t)[t > 0].max())
    cf, c2 = np.float32(c), np.float32(c * c)
    assert np.float32(cf * cf) - c2 == 0 and float(cf) ** 2 - float(c2) > 0      # (float(cf) ** 2 is exact in fp64)
    at_c = (t > 0) & (np.abs(p - t) == cf)
    assert at_c.sum() == 16 and not np.any(g["edge_f32__berhu__grad"].reshape(p.shape)[at_c])
    p, t = depth_pair("dzero")
    dz = (t > 0) & (p == t)
    assert dz.sum() > 10
    for name in ("l1", "berhu"):
        assert not np.any(g[f"dzero__{name}__grad"].reshape(p.shape)[dz])


def _reference_dir():
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    try:
        from make_golden import REF
    finally:
        sys.path.pop(0)
    return REF


@pytest.mark.skipif(not os.path.isdir(os.path.join(_reference_dir(), "src", "utils")), reason="the reference source is not present")
def test_generator_reproduces_fixture_bit_for_bit():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "loss_zoo.npz")
        subprocess.run([sys.executable, GEN, "--out", out], check=True, capture_output=True, timeout=600)
        new, old = dict(np.load(out)), load_npz("loss_zoo.npz")
        assert sorted(new) == sorted(old)
        for k in old:
            np.testing.assert_array_equal(new[k], old[k], err_msg=k)


# ---- TrainStep(criterion=...) -----------------------------------------------------------------------------------------------
def test_criterion_modes():
    from camradepth_amd import losses as HL
    from camradepth_amd.trainer import depth_criterion_mode
    assert depth_criterion_mode(None) == ("smooth_l1", None)
    for d, mode in ((HL.MaskedSmoothL1Loss(), "smooth_l1"), (HL.MaskedHuberLoss(), "smooth_l1"), (HL.MaskedL1Loss(), "l1"),
                    (HL.MaskedRMSELoss(), "rmse")):
        assert depth_criterion_mode({"depth": d, "seg": HL.MaskedFocalLoss()}) == (mode, None)
    assert depth_criterion_mode({"depth": HL.MaskedBerHuLoss(), "seg": HL.MaskedFocalLoss()}) == ("berhu", 0.2)
    assert depth_criterion_mode({"depth": HL.MaskedBerHuLoss(0.5), "seg": HL.MaskedFocalLoss()}) == ("berhu", 0.5)


def test_train_step_refuses_unsupported_criteria_before_any_launch(monkeypatch):
    from camradepth_amd import lib as L
    from camradepth_amd import losses as HL
    from camradepth_amd.model import CamRaDepth
    from camradepth_amd.trainer import TrainStep

    def no_launch(*a, **k):
        raise AssertionError("the HIP library was touched before the criterion was checked")
    monkeypatch.setattr(L, "load", no_launch)
    m = CamRaDepth(input_channels=7, depths=(1, 1, 1, 1)).train()
    focal = HL.MaskedFocalLoss()
    bad = [{"depth": HL.MaskedMSELoss(), "seg": focal}, {"depth": HL.SmoothnessLoss(), "seg": focal},
           {"depth": torch.nn.L1Loss(), "seg": focal}, {"depth": HL.MaskedBerHuLoss(thresh=0.0), "seg": focal},
           {"depth": HL.MaskedBerHuLoss(thresh=-0.2), "seg": focal}, {"depth": HL.MaskedBerHuLoss(thresh=float("nan")), "seg": focal},
           {"depth": HL.MaskedL1Loss(), "seg": HL.MaskedSmoothL1Loss()}, {"depth": HL.MaskedL1Loss()},
           {"depth": HL.MaskedL1Loss(), "seg": focal, "extra": focal}, [HL.MaskedL1Loss(), focal]]
    for crit in bad:
        with pytest.raises(L.CrdError):
            TrainStep(m, 2, 64, 96, criterion=crit)


# ---- collectives of a BerHu step (gloo world 2, stand-ins for the HIP graphs) -------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


MAXIMA = ((3.0, 1.0, 2.0), (1.5, 4.0, 2.5))      # per rank, per depth level: max |d|


def _scenario(rank, world, mode, late, log, holder):
    import contextlib
    from camradepth_amd.trainer import GradSync
    from tests.trainstep_stub import stub_model, stub_trainstep
    ts = stub_trainstep(stub_model(), dist_active=True, k=2, world=world, late=late)
    holder["ts"] = ts
    if mode == "berhu":
        ts._depth_mode, ts._berhu_thresh = "berhu", 0.2
        ts.maxbits = torch.zeros(4, dtype=torch.int32)
        ts.berhu_acc = torch.zeros(8, dtype=torch.int64)
    seen_c = []

    def fwd():
        log.append(("fwd",))
        ts.acc.zero_()
        ts.acc[1::4] += rank + 1
        if mode == "berhu":
            ts.maxbits.zero_()
            ts.berhu_acc.zero_()
            ts.maxbits[:3].copy_(torch.tensor(MAXIMA[rank], dtype=torch.float32).view(torch.int32))

    def bwd(key):
        log.append(("bwd", key))
        if mode == "berhu" and key == GradSync.ORDER[0]:          # phase (b) runs at the head of the backward
            seen_c.append((ts._berhu_thresh * ts.maxbits[:3].view(torch.float32).double()).tolist())
            ts.berhu_acc[0] += rank + 1
    ts._forward_and_loss_partials, ts._loss_backward, ts._optimizer = fwd, lambda: None, lambda key=None: None
    ts.plan.backward = lambda tags=None: bwd(tags)
    if late:
        ts.late_stream = "late"
        ts._current_stream = lambda: "main"
        ts._stream_wait = lambda waiter, on: None
        ts._on_stream = lambda stream: contextlib.nullcontext()

        class G:
            def __init__(self, fns):
                self.fns = list(fns)

            def replay(self):
                for fn in self.fns:
                    fn()
        ts._graph = lambda fns, stream=None: G(fns)
        ts.graphs = {}
        for ts._zero in (True, False):             # the trainer's own capture of every variant
            for ts._opt in (True, False):
                ts._capture_iteration()
    for it in range(2):
        ts.step()
    return ts, seen_c


def _worker_collectives(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        results = {}
        orig = dist.all_reduce
        for mode in ("default", "berhu"):
            for late in (False, True):
                log, holder = [], {}

                def logged(t, op=dist.ReduceOp.SUM, group=None, async_op=False):
                    ts = holder["ts"]
                    name = "bucket"
                    if t is ts.acc:
                        name = "acc"
                    elif t is getattr(ts, "maxbits", None):
                        name = "max"
                    elif t is getattr(ts, "berhu_acc", None):
                        name = "berhu_sums"
                    log.append(("allreduce", name, "max" if op == dist.ReduceOp.MAX else "sum"))
                    return orig(t, op=op, group=group, async_op=async_op)
                dist.all_reduce = logged
                try:
                    ts, seen_c = _scenario(rank, world, mode, late, log, holder)
                finally:
                    dist.all_reduce = orig
                results[(mode, late)] = (log, seen_c, ts.maxbits.tolist() if mode == "berhu" else None,
                                         ts.berhu_acc.tolist() if mode == "berhu" else None)
        q.put((rank, results))
    finally:
        dist.destroy_process_group()


def test_berhu_max_reduction_runs_at_the_loss_point_world2():
    from camradepth_amd.trainer import GradSync
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_collectives, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    buckets = [("allreduce", "bucket", "sum")] * len(GradSync.ORDER)
    bwd = [("bwd", k) for k in GradSync.ORDER]
    for late in (False, True):
        # default criterion: one SUM of the loss partials per iteration, the bucket all-reduces on the window's closing iteration
        for rank in (0, 1):
            log = res[rank][("default", late)][0]
            calls = [e for e in log if e[0] == "allreduce"]
            assert calls == [("allreduce", "acc", "sum")] + [("allreduce", "acc", "sum")] + buckets, (late, calls)
        # BerHu: the MAX of the maxima right behind the SUM, before any backward segment; the loss sums at the end
        for rank in (0, 1):
            log, seen_c, maxbits, sums = res[rank][("berhu", late)]
            it = [("fwd",), ("allreduce", "acc", "sum"), ("allreduce", "max", "max")]
            first = it + bwd + [("allreduce", "berhu_sums", "sum")]            # accumulating iteration: no bucket all-reduce
            second = it + [e for k in GradSync.ORDER for e in (("bwd", k), ("allreduce", "bucket", "sum"))] + \
                [("allreduce", "berhu_sums", "sum")]
            assert log == first + second, (late, log)
            glob = [max(a, b) for a, b in zip(*MAXIMA)]
            assert seen_c == [[0.2 * v for v in glob]] * 2, seen_c          # both iterations' gradients use the global c
            assert np.array(maxbits[:3], dtype=np.int32).view(np.float32).tolist() == glob
            assert sums[0] == 1 + 2                                           # loss sums of both ranks
        assert res[0][("berhu", late)][1] == res[1][("berhu", late)][1]      # both ranks: the same c
