"""CPU: which C entries the depth criteria call, in which order and with which arguments -- for the eager loss modules
(camradepth_amd.losses) and for TrainStep's loss point (_forward_and_loss_partials, _loss_backward, _level_losses).  A stand-in
object replaces the HIP library; it records every call as (entry name, arguments) with each pointer rewritten as (buffer name,
byte offset), and fills the sums it is handed so that the values the callers form from them are finite and can be checked
against the criterion's formula.  The kernels themselves are checked on the GPU (tests/test_gpu_loss_zoo.py)."""
import ctypes as C
import math
import struct
import types

import pytest
import torch

from camradepth_amd import lib as L
from camradepth_amd import losses as HL
from camradepth_amd.trainer import LOSS_W

ONE = 1 << L.STAT_FRAC_BITS
STREAM = "stream"
# argument roles of the recorded entries (include/camradepth_hip.h)
ROLES = {
    "crd_masked_l1_fwd": ("pred", "tgt", "n", "acc", "stream"),
    "crd_masked_dist_fwd": ("pred", "tgt", "n", "acc", "stream"),
    "crd_masked_berhu_max": ("pred", "tgt", "n", "acc", "mx", "stream"),
    "crd_masked_l1_bwd": ("pred", "tgt", "n", "acc", "gout", "gmul", "d", "stream"),
    "crd_masked_dist_bwd": ("pred", "tgt", "n", "acc", "gout", "gmul", "mode", "d", "stream"),
    "crd_masked_berhu": ("pred", "tgt", "n", "acc", "mx", "thresh", "ls", "gout", "gmul", "d", "stream"),
    "crd_ce_fwd": ("logits", "labels", "B", "C", "HW", "acc", "stream"),
    "crd_ce_focal_bwd": ("logits", "labels", "B", "C", "HW", "acc", "gout", "gmul", "d", "stream"),
    "crd_nonfinite_status": ("mode", "stream"),
}
POINTERS = {"pred", "tgt", "acc", "mx", "ls", "gout", "d", "logits", "labels"}
# what the stand-in leaves in the buffers it is handed
ACC = (3 * ONE, 2 * ONE, 8 * ONE, 0)         # (sum, count, sum d^2, -)
MAX_ABS = 2.0
LS = (5 * ONE, 7 * ONE)                      # BerHu: (sum part1, sum of part2's numerators)


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]      # as a C float argument arrives


class FakeLib:
    """Stands in for libcamradepth_hip.so.  buffers: name -> tensor, the memory the test knows; a pointer into one of them is
    recorded as (name, byte offset).  Any other pointer belongs to a tensor its caller made: it is recorded as (its argument's
    role, 0), or (role + "'", 0) if that role was seen with another address before -- the backward must hand back the
    forward's acc and max word, not copies."""

    def __init__(self, buffers=None):
        self.calls, self.buffers, self.seen = [], dict(buffers or {}), {}

    def name_of(self, role, p):
        if p is None:
            return None
        for name, t in self.buffers.items():
            if t.data_ptr() <= p < t.data_ptr() + max(t.numel() * t.element_size(), 1):
                return (name, p - t.data_ptr())
        return (role, 0) if self.seen.setdefault(role, p) == p else (role + "'", 0)

    def __getattr__(self, entry):
        roles = ROLES[entry]                 # KeyError: an entry this test does not expect

        def call(*args):
            assert len(args) == len(roles) == len(L._SIGS[entry]), (entry, args)
            a = dict(zip(roles, args))
            rec = tuple(self.name_of(r, v) if r in POINTERS else (f32(v) if r == "gmul" else v) for r, v in a.items())
            self.calls.append((entry, rec))
            if entry in ("crd_masked_l1_fwd", "crd_masked_dist_fwd", "crd_masked_berhu_max"):
                (C.c_int64 * 4).from_address(a["acc"])[:] = ACC
            if entry == "crd_masked_berhu_max":
                C.c_float.from_address(a["mx"]).value = MAX_ABS
            if entry == "crd_masked_berhu" and a["ls"] is not None:
                (C.c_int64 * 2).from_address(a["ls"])[:] = LS
            if a.get("d") is not None and entry != "crd_ce_focal_bwd":
                C.memset(a["d"], 0, 4 * a["n"])
            return 0
        return call


@pytest.fixture
def fake(monkeypatch):
    lb = FakeLib()
    monkeypatch.setattr(L, "load", lambda: lb)
    monkeypatch.setattr(L, "stream", lambda: STREAM)
    return lb


# ---- (a) the eager modules -------------------------------------------------------------------------------------------------------
N = 2 * 1 * 3 * 5
P, T, A, MX, LSUM, G, D = ("pred", 0), ("tgt", 0), ("acc", 0), ("mx", 0), ("ls", 0), ("gout", 0), ("d", 0)
STATUS = ("crd_nonfinite_status", (0, STREAM))
HALF = L.f64_bits(0.5)
A64 = [v / ONE for v in ACC]
MODULES = {
    "smooth_l1": (HL.MaskedSmoothL1Loss, (), A64[0] / A64[1],
                  [("crd_masked_l1_fwd", (P, T, N, A, STREAM)), STATUS, ("crd_masked_l1_bwd", (P, T, N, A, G, 1.0, D, STREAM))]),
    "huber": (HL.MaskedHuberLoss, (), A64[0] / A64[1],
              [("crd_masked_l1_fwd", (P, T, N, A, STREAM)), STATUS, ("crd_masked_l1_bwd", (P, T, N, A, G, 1.0, D, STREAM))]),
    "l1": (HL.MaskedL1Loss, (), A64[0] / A64[1],
           [("crd_masked_dist_fwd", (P, T, N, A, STREAM)), STATUS, ("crd_masked_dist_bwd", (P, T, N, A, G, 1.0, 0, D, STREAM))]),
    "rmse": (HL.MaskedRMSELoss, (), math.sqrt(A64[2] / A64[1]),
             [("crd_masked_dist_fwd", (P, T, N, A, STREAM)), STATUS, ("crd_masked_dist_bwd", (P, T, N, A, G, 1.0, 1, D, STREAM))]),
    "berhu": (HL.MaskedBerHuLoss, (0.5,), float(HL.berhu_value(LS[0] / ONE, LS[1] / ONE, A64[1], MAX_ABS, 0.5)),
              [("crd_masked_berhu_max", (P, T, N, A, MX, STREAM)),
               ("crd_masked_berhu", (P, T, N, A, MX, HALF, LSUM, None, 0.0, None, STREAM)), STATUS,
               ("crd_masked_berhu", (P, T, N, A, MX, HALF, None, G, 1.0, D, STREAM))]),
    "mse": (HL.MaskedMSELoss, (), A64[2] / A64[1], [("crd_masked_l1_fwd", (P, T, N, A, STREAM)), STATUS]),
}


@pytest.mark.parametrize("name", list(MODULES))
def test_eager_module_calls(fake, name):
    cls, args, value, expected = MODULES[name]
    g = torch.Generator().manual_seed(0)
    pred = torch.rand((2, 1, 3, 5), generator=g).requires_grad_(True)
    target = torch.rand((2, 1, 3, 5), generator=g)
    fake.buffers.update(pred=pred, tgt=target)
    module = cls(*args)
    loss = module(pred, target)
    assert loss.dtype == torch.float32 and float(loss.detach()) == float(torch.tensor(value, dtype=torch.float64).float())
    if name in ("l1", "rmse", "mse"):
        assert module.loss is loss
    if name != "mse":
        loss.backward()
        assert pred.grad is not None and pred.grad.shape == pred.shape
    else:
        assert not loss.requires_grad
    assert fake.calls == expected


# ---- (b) TrainStep ---------------------------------------------------------------------------------------------------------------
B, H, W = 2, 8, 12
LEVELS = ((5, "full", 1), (4, "half", 2), (3, "quarter", 4))
GRAD_ENTRY = {"smooth_l1": "crd_masked_l1_bwd", "l1": "crd_masked_dist_bwd", "rmse": "crd_masked_dist_bwd", "berhu": "crd_masked_berhu"}
FWD_ENTRY = {"smooth_l1": "crd_masked_l1_fwd", "l1": "crd_masked_dist_fwd", "rmse": "crd_masked_dist_fwd", "berhu": "crd_masked_berhu_max"}
THRESH = 0.3


@pytest.fixture(scope="module")
def model():
    from tests.trainstep_stub import stub_model
    return stub_model()


def loss_point_trainstep(model, fake, mode, sup, k):
    from tests.trainstep_stub import stub_trainstep
    ts = stub_trainstep(model, k=k)
    nc = model.cfg.num_classes
    ts.lib, ts.B, ts.H, ts.W, ts.sup = fake, B, H, W, sup
    ts.gt = {key: torch.zeros((B, 1, H // s, W // s)) for _, key, s in LEVELS}
    ts.gt["seg"] = torch.zeros((B, H, W), dtype=torch.int64)
    out = {}
    for j, key, s in LEVELS:
        out[j] = types.SimpleNamespace(t=torch.zeros((B, 1, H // s, W // s)))
        out[("grad", j)] = types.SimpleNamespace(t=torch.zeros((B, 1, H // s, W // s)))
    ts.plan = types.SimpleNamespace(out_depth=out, seg_out=torch.zeros((B, nc, H, W)), seg_grad_in=torch.zeros((B, nc, H, W)),
                                    forward=lambda pack=True: None)
    ts._depth_mode = mode
    if mode == "berhu":
        ts._berhu_thresh = THRESH
        ts.maxbits = torch.zeros(4, dtype=torch.int32)
        ts.berhu_acc = torch.zeros(8, dtype=torch.int64)
        fake.buffers.update(maxbits=ts.maxbits, berhu_acc=ts.berhu_acc)
    fake.buffers.update(acc=ts.acc, seg_out=ts.plan.seg_out, seg_grad_in=ts.plan.seg_grad_in, gt_seg=ts.gt["seg"])
    for j, key, s in LEVELS:
        fake.buffers.update({f"out{j}": out[j].t, f"grad{j}": out[("grad", j)].t, f"gt_{key}": ts.gt[key]})
    return ts


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sup", [False, True])
@pytest.mark.parametrize("mode", list(FWD_ENTRY))
def test_trainstep_loss_point_calls(fake, model, mode, sup, k):
    ts = loss_point_trainstep(model, fake, mode, sup, k)
    nc = model.cfg.num_classes
    ts._forward_and_loss_partials()
    ts._loss_backward()
    expected = []
    for i, (j, key, s) in enumerate(LEVELS):
        n = B * (H // s) * (W // s)
        head = ((f"out{j}", 0), (f"gt_{key}", 0), n, ("acc", 32 * i))
        expected.append((FWD_ENTRY[mode], head + ((("maxbits", 4 * i),) if mode == "berhu" else ()) + (STREAM,)))
    if sup:
        expected.append(("crd_ce_fwd", (("seg_out", 0), ("gt_seg", 0), B, nc, H * W, ("acc", 96), STREAM)))
    for i, (j, key, s) in enumerate(LEVELS):
        n = B * (H // s) * (W // s)
        head = ((f"out{j}", 0), (f"gt_{key}", 0), n, ("acc", 32 * i))
        gmul, d = f32(LOSS_W[i] / sum(LOSS_W) / k), (f"grad{j}", 0)
        tail = {"smooth_l1": (None, gmul, d), "l1": (None, gmul, 0, d), "rmse": (None, gmul, 1, d),
                "berhu": (("maxbits", 4 * i), L.f64_bits(THRESH), ("berhu_acc", 16 * i), None, gmul, d)}[mode]
        expected.append((GRAD_ENTRY[mode], head + tail + (STREAM,)))
    if sup:
        expected.append(("crd_ce_focal_bwd", (("seg_out", 0), ("gt_seg", 0), B, nc, H * W, ("acc", 96), None,
                                              f32(LOSS_W[3] / sum(LOSS_W) / k), ("seg_grad_in", 0), STREAM)))
    assert fake.calls == expected


@pytest.mark.parametrize("mode", list(FWD_ENTRY))
def test_level_losses(fake, model, mode):
    ts = loss_point_trainstep(model, fake, mode, False, 1)
    sums = [(3.0, 2.0, 8.0), (1.5, 4.0, 9.0), (7.0, 8.0, 2.0)]          # per level: (sum, count, sum d^2)
    for i, s in enumerate(sums):
        ts.acc[4 * i:4 * i + 3] = torch.tensor([int(v * ONE) for v in s])
    maxima, parts = (2.0, 0.5, 4.0), [(5.0, 7.0), (1.0, 0.25), (0.0, 3.0)]
    if mode == "berhu":
        ts.maxbits[:3] = torch.tensor(maxima, dtype=torch.float32).view(torch.int32)
        ts.berhu_acc[:6] = torch.tensor([int(v * ONE) for p in parts for v in p])
    want = {"smooth_l1": [s[0] / s[1] for s in sums], "l1": [s[0] / s[1] for s in sums],
            "rmse": [math.sqrt(s[2] / s[1]) for s in sums],
            "berhu": [(p[0] + p[1] / (2.0 * THRESH * m)) / s[1] for s, p, m in zip(sums, parts, maxima)]}[mode]
    got = ts._level_losses(L.stat_value(ts.acc))
    assert all(isinstance(v, float) for v in got) and got == want
    assert fake.calls == []


# ---- (c) the table ---------------------------------------------------------------------------------------------------------------
def test_every_accepted_class_has_a_record():
    from camradepth_amd.trainer import depth_criterion_mode
    assert set(HL.CRITERIA) == set(FWD_ENTRY)
    accepted = [HL.MaskedSmoothL1Loss, HL.MaskedHuberLoss, HL.MaskedL1Loss, HL.MaskedRMSELoss, HL.MaskedBerHuLoss]
    assert set(HL.DepthCriterion.__subclasses__()) == set(accepted)
    for cls in accepted:
        mode, _ = depth_criterion_mode({"depth": cls(), "seg": HL.MaskedFocalLoss()})
        assert mode == cls.mode and mode in HL.CRITERIA
