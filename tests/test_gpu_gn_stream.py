"""GPU: the three streaming GroupNorm passes (crd_gn_apply, crd_gn_bwd_reduce, crd_gn_bwd_apply) against float64 torch
(F.group_norm, F.gelu, autograd), at the shapes where their pipelined loop and the partition of crd_gn_launch_shape have an edge:
one pixel, a batch minus / plus one, whole batches with a ragged rest, a capped grid of several batches per workgroup, idle threads
in a workgroup, one pixel lane, the channel-sliced reduce with and without scratch.  Every shape runs with and without GELU, with
and without a mask, with bf16 and fp32 x; every tensor has a row stride wider than C and a channel offset, and what lies outside
the written slice must stay as it was.  Tolerances are those of test_gpu_ops.py::test_groupnorm_forward_backward."""
import pytest
import torch
import torch.nn.functional as F

from tests.util import zsum

pytestmark = pytest.mark.gpu

TPB, CAP = 256, 2048                       # camradepth_amd/csrc/norm.hip
PAD, OFF = 16, 8                           # row stride = C + PAD, channel offset = OFF (both multiples of 8)
SENTINEL = 7.0


def lanes(C):
    return max(1, TPB // (C // 8))


def bwd_batch(C):
    """Pixels of one batch of crd_gn_bwd_apply (2 per lane); crd_gn_apply's is twice that."""
    return 2 * lanes(C)


_B128 = bwd_batch(128)
# id: (C, gmul, B, P)
SHAPES = {
    "C16_P1": (16, 1, 2, 1),
    "C128_batch-1": (128, 1, 2, _B128 - 1),
    "C128_batch": (128, 1, 2, _B128),
    "C128_batch+1": (128, 1, 2, _B128 + 1),
    "C128_3batch+quarter": (128, 1, 2, 3 * _B128 + _B128 // 4),
    "C128_applybatch-1": (128, 1, 2, 2 * _B128 - 1),
    "C128_applybatch": (128, 1, 2, 2 * _B128),
    "C128_applybatch+1": (128, 1, 2, 2 * _B128 + 1),
    "C128_3applybatch+quarter": (128, 1, 2, 6 * _B128 + _B128 // 2),
    "C128_fills_chip": (128, 1, 2, 16384 + 77),        # not a small grid, below the cap: four batches per workgroup
    "C128_B16_capped": (128, 1, 16, 33001),            # ~135 MB per bf16 tensor: the cap is active, nine batches per workgroup
    "C320_idle_threads": (320, 1, 2, 77),
    "C2048_one_lane": (2048, 4, 2, 37),
    "C512_sliced_reduce": (512, 8, 2, 333),
    "C512_fills_chip": (512, 8, 2, 4099),
}


def L():
    from camradepth_amd import lib
    return lib, lib.load()


def ptr(t):
    return None if t is None else t.data_ptr()


def ok(rc, what):
    lib, _ = L()
    lib.check(rc, what)
    torch.cuda.synchronize()


def close(got, ref, what, rel, elem):
    """assert_close of tests/test_gpu_igemm.py, on the device and in float64; prints the figures before it asserts."""
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    rl2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    print(f"{what}: max err {err:.3e} (scale {scale:.3e}, bound {elem * scale:.3e}), rel-L2 {rl2:.3e} (bound {rel:.1e})")
    assert err <= elem * scale and rl2 < rel, f"{what}: max err {err:.3e} (scale {scale:.3e}), rel-L2 {rl2:.3e}"


def wide(values, dtype):
    """[B][P][C] values inside a [B][P][C + PAD] buffer of sentinels, at channel offset OFF -> (buffer, the slice's view)."""
    B, Pn, C = values.shape
    buf = torch.full((B, Pn, C + PAD), SENTINEL, dtype=dtype, device="cuda")
    buf[..., OFF:OFF + C] = values.to(dtype)
    return buf, buf[..., OFF:OFF + C]


def untouched(buf, C, what):
    assert bool((buf[..., :OFF] == SENTINEL).all()) and bool((buf[..., OFF + C:] == SENTINEL).all()), f"{what}: bytes outside the slice changed"


class Problem:
    """Inputs of one case on the device, their float64 reference, and the statistics crd_gn_stats leaves for them."""

    def __init__(self, C, gmul, B, Pn, act, masked, xf32):
        lib, lb = L()
        g = torch.Generator(device="cuda").manual_seed(1000 * C + 10 * Pn + 4 * act + 2 * masked + xf32)
        self.C, self.gmul, self.B, self.P, self.act, self.xf32 = C, gmul, B, Pn, act, xf32
        self.ld = C + PAD
        self.groups = C // (16 * gmul)
        xdt = torch.float32 if xf32 else torch.bfloat16
        x = (torch.randn(B, Pn, C, generator=g, device="cuda") * 1.5 + 0.3).to(xdt)
        dy = torch.randn(B, Pn, C, generator=g, device="cuda").to(torch.bfloat16)
        self.gamma = 1 + 0.1 * torch.randn(C, generator=g, device="cuda")
        self.beta = 0.1 * torch.randn(C, generator=g, device="cuda")
        self.mask = ((torch.rand(B, C, generator=g, device="cuda") < 0.8).float() / 0.8) if masked else None
        self.xbuf, self.x = wide(x, xdt)
        self.dybuf, self.dy = wide(dy, torch.bfloat16)
        # float64 reference
        xr = x.double().permute(0, 2, 1).contiguous().requires_grad_(True)
        gr, br = self.gamma.double().requires_grad_(True), self.beta.double().requires_grad_(True)
        y = F.group_norm(xr, self.groups, gr, br, 1e-5)
        if act:
            y = F.gelu(y)
        if masked:
            y = y * self.mask.double().view(B, C, 1)
        y.backward(dy.double().permute(0, 2, 1))
        self.y_ref = y.detach().permute(0, 2, 1)
        self.dx_ref = xr.grad.permute(0, 2, 1)
        self.dgamma_ref, self.dbeta_ref = gr.grad, br.grad
        del xr, y
        self.stats = zsum(B, C // 16, 2)
        ok(lb.crd_gn_stats(ptr(self.xbuf), xf32, self.ld, OFF, B, Pn, C, ptr(self.stats), None, lib.stream()), "gn_stats")

    def head(self):
        """The arguments every backward entry starts with."""
        return [ptr(self.xbuf), self.xf32, self.ld, OFF, ptr(self.dybuf), 0, self.ld, OFF, self.B, self.P, self.C, ptr(self.stats),
                self.gmul, ptr(self.gamma), ptr(self.beta), self.act, ptr(self.mask)]

    def reduce(self, scratch=None):
        lib, lb = L()
        r = zsum(self.B * self.C * 2 + self.B * self.groups * 2)
        ok(lb.crd_gn_bwd_reduce(*self.head(), ptr(r), ptr(scratch), scratch.numel() if scratch is not None else 0, lib.stream()),
           "gn_bwd_reduce")
        return r

    def bwd_apply(self, r, dgamma, dbeta, dxbuf, dx_f32, acc, dx2=None, dx2_ld=0, scale2=None):
        lib, lb = L()
        ok(lb.crd_gn_bwd_apply(*self.head(), ptr(r), ptr(dgamma), ptr(dbeta), ptr(dxbuf), dx_f32, self.ld, OFF, acc, ptr(dx2), dx2_ld,
                               ptr(scale2), lib.stream()), "gn_bwd_apply")


@pytest.mark.parametrize("xf32", [0, 1], ids=["x_bf16", "x_fp32"])
@pytest.mark.parametrize("masked", [0, 1], ids=["nomask", "mask"])
@pytest.mark.parametrize("act", [0, 1], ids=["linear", "gelu"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gn_streaming_passes(shape, act, masked, xf32):
    lib, lb = L()
    C, gmul, B, Pn = SHAPES[shape]
    # the shape runs the edge of the partition it is here for
    for kind in (0, 1):
        nblk, chunk, batch = lib.gn_launch_shape(Pn, C, B, kind)
        assert batch == bwd_batch(C) * (2 if kind == 0 else 1)
        if shape == "C128_B16_capped":
            assert nblk * B > CAP // 2 and chunk >= 3 * batch and Pn % batch != 0 and (nblk - 1) * chunk < Pn, (nblk, chunk, batch)
        if shape.endswith("fills_chip"):
            assert chunk % batch == 0 and chunk >= 8 * lanes(C) and nblk * B >= 256, (nblk, chunk, batch)
    if shape == "C320_idle_threads":
        assert lanes(C) * (C // 8) < TPB
    if shape == "C2048_one_lane":
        assert lanes(C) == 1
    q = Problem(C, gmul, B, Pn, act, masked, xf32)
    ld = q.ld

    # ---- forward: bf16 and fp32 output
    ybuf, y = wide(torch.zeros(B, Pn, C, device="cuda"), torch.bfloat16)
    ok(lb.crd_gn_apply(ptr(q.xbuf), xf32, ld, OFF, B, Pn, C, ptr(q.stats), gmul, ptr(q.gamma), ptr(q.beta), act, ptr(q.mask), ptr(ybuf),
                       0, ld, OFF, lib.stream()), "gn_apply")
    close(y, q.y_ref, "gn_apply bf16", rel=4e-3, elem=1e-2)
    untouched(ybuf, C, "gn_apply bf16")
    yfbuf, yf = wide(torch.zeros(B, Pn, C, device="cuda"), torch.float32)
    ok(lb.crd_gn_apply(ptr(q.xbuf), xf32, ld, OFF, B, Pn, C, ptr(q.stats), gmul, ptr(q.gamma), ptr(q.beta), act, ptr(q.mask), ptr(yfbuf),
                       1, ld, OFF, lib.stream()), "gn_apply f32")
    close(yf, q.y_ref, "gn_apply fp32", rel=1e-4, elem=1e-4)
    untouched(yfbuf, C, "gn_apply fp32")
    del ybuf, y, yfbuf, yf

    # ---- backward, phase 1: both reduction paths (atomics, channel-sliced from 256 channels on; per-workgroup partials in scratch)
    r = q.reduce()
    assert torch.equal(q.reduce(), r), "r: two calls on the same inputs differ"
    scratch = torch.full((B * 1024 * 2 * C,), 3.0, device="cuda")
    r_scratch = q.reduce(scratch)
    assert torch.equal(q.reduce(scratch), r_scratch), "r (scratch path): two calls on the same inputs differ"
    del scratch

    # ---- phase 2: bf16 dx written once, parameter gradients on
    def grads():
        return torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")

    dgam, dbet = grads()
    dxbuf, dx = wide(torch.zeros(B, Pn, C, device="cuda"), torch.bfloat16)
    q.bwd_apply(r, dgam, dbet, dxbuf, 0, 0)
    close(dx, q.dx_ref, "dx bf16", rel=6e-3, elem=2e-2)
    close(dgam, q.dgamma_ref, "dgamma", rel=2e-3, elem=4e-3)
    close(dbet, q.dbeta_ref, "dbeta", rel=2e-3, elem=4e-3)
    untouched(dxbuf, C, "dx bf16")
    dgam2, dbet2 = grads()
    dxbuf2, dx2nd = wide(torch.zeros(B, Pn, C, device="cuda"), torch.bfloat16)
    q.bwd_apply(r, dgam2, dbet2, dxbuf2, 0, 0)
    assert torch.equal(dxbuf2, dxbuf) and torch.equal(dgam2, dgam) and torch.equal(dbet2, dbet), "two calls on the same inputs differ"
    # the sums of the scratch path give the same gradients within the same bounds
    dgam_s, dbet_s = grads()
    q.bwd_apply(r_scratch, dgam_s, dbet_s, dxbuf2, 0, 0)
    close(dx2nd, q.dx_ref, "dx bf16 (scratch-path sums)", rel=6e-3, elem=2e-2)
    close(dgam_s, q.dgamma_ref, "dgamma (scratch-path sums)", rel=2e-3, elem=4e-3)
    close(dbet_s, q.dbeta_ref, "dbeta (scratch-path sums)", rel=2e-3, elem=4e-3)
    del dxbuf2, dx2nd

    # ---- dx aliasing dy (the in-place form of the Mlp backward), parameter gradients off: the same bits, dy's padding untouched
    dy_keep = q.dybuf.clone()
    q.bwd_apply(r, None, None, q.dybuf, 0, 0)
    assert torch.equal(q.dybuf, dxbuf), "dx written over dy differs from dx written next to it"
    q.dybuf.copy_(dy_keep)
    del dy_keep

    # ---- accumulate into bf16
    g = torch.Generator(device="cuda").manual_seed(7)
    base = torch.randn(B, Pn, C, generator=g, device="cuda").to(torch.bfloat16)
    accbuf, acc = wide(base, torch.bfloat16)
    q.bwd_apply(r, None, None, accbuf, 0, 1)
    close(acc, base.double() + q.dx_ref, "dx accumulated into bf16", rel=6e-3, elem=2e-2)
    untouched(accbuf, C, "dx accumulated into bf16")
    del accbuf, acc

    # ---- fp32 dx: written once, accumulated, accumulated with the scaled bf16 copy
    fbuf, f = wide(torch.full((B, Pn, C), 5.0, device="cuda"), torch.float32)
    q.bwd_apply(r, None, None, fbuf, 1, 0)
    close(f, q.dx_ref, "dx fp32", rel=1e-3, elem=2e-3)
    untouched(fbuf, C, "dx fp32")
    base32 = base.float()
    fbuf, f = wide(base32, torch.float32)
    q.bwd_apply(r, None, None, fbuf, 1, 1)
    close(f - base32, q.dx_ref, "dx accumulated into fp32", rel=1e-3, elem=2e-3)
    untouched(fbuf, C, "dx accumulated into fp32")
    fbuf2, f2 = wide(base32, torch.float32)
    copybuf = torch.full((B, Pn, C + 8), SENTINEL, dtype=torch.bfloat16, device="cuda")
    scale2 = torch.tensor([0.5 + 0.25 * i for i in range(B)], device="cuda")
    dgam3, dbet3 = grads()
    q.bwd_apply(r, dgam3, dbet3, fbuf2, 1, 1, copybuf, C + 8, scale2)
    assert torch.equal(fbuf2, fbuf), "dx fp32 with the copy differs from dx fp32 without it"
    assert torch.equal(copybuf[..., :C], (f2 * scale2.view(B, 1, 1)).to(torch.bfloat16)), "dx2 is not bf16(scale2 * dx)"
    assert bool((copybuf[..., C:] == SENTINEL).all()), "dx2: bytes outside the slice changed"
    assert torch.equal(dgam3, dgam) and torch.equal(dbet3, dbet), "parameter gradients depend on the output form"
