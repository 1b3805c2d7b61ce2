"""GPU: crd_bicubic2x, crd_bicubic2x_fp8 and crd_bicubic2x_bwd against a float64 reference built here from the matrices of the
bicubic x2 (PyTorch's upsample_bicubic2d, A = -0.75, clamped borders): y = By x Bx^T, dx (+)= By^T dy Bx.  The reference never calls
the code under test.  B = 2 at small, odd and border-only maps, and B = 64 or 128 at the maps that reach every band height of the
row-walking kernels: a workgroup walks a band of R = 8 input rows, halved down to 2 while the grid would have fewer than 256
workgroups, and covers S = 256 / (C / 8) columns; on a grid smaller still the forward runs its one-thread-per-pixel form (bicubic.hip,
tiling).  H = R + 1 and 2R - 1 and W = S + 1 are among the shapes of every band height, in the banded forward too.
Every shape runs with x_ld = C + 8, x_coff = 8 and y_ld = C + 16, the transpose with accumulate 0 and 1:
  1. integer inputs in [-8, 8]: every partial sum is a multiple of 2^-16 below 2^7, exact in fp32 in any order, so the output equals
     bf16(float64 result) bit for bit
  2. random inputs: |got - v| <= 2^-8 |v| + n 2^-23 A, A the same product of absolute values, n = 16 terms forward and 100 backward
     (half a bf16 ulp; an fp32 sum of n terms)
  3. sentinels in the padding columns and in a guard row behind every output stay untouched
  4. a second run is bit-equal to the first
  5. on two shapes both forms of crd_bicubic2x_fp8 equal crd_quant_fp8 of the bf16 output."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WO = (-0.10546875, 0.87890625, 0.26171875, -0.03515625)         # odd output 2k + 1: inputs k - 1 .. k + 2
WE = (-0.03515625, 0.26171875, 0.87890625, -0.10546875)         # even output 2k: inputs k - 2 .. k + 1
SENTINEL = 123.0
SHAPES = [(2, 1, 1, 8), (2, 1, 5, 8), (2, 2, 3, 16), (2, 3, 4, 8), (2, 4, 4, 24), (2, 5, 7, 16), (2, 8, 13, 256), (2, 9, 16, 40),
          (2, 7, 17, 136), (2, 16, 26, 128), (2, 19, 37, 72), (2, 33, 18, 136),
          # R = 2, 4, 8 on grids of 256 workgroups: H = R + 1 and 2R - 1, all with W = S + 1 (S = 32 columns at C = 64)
          (64, 3, 33, 64), (64, 5, 33, 64), (64, 7, 33, 64), (64, 9, 33, 64), (64, 15, 33, 64),
          # the banded forms at a ragged channel count (17 granules, R = 4) and on maps lower than one band (R = 8)
          (64, 6, 17, 136), (128, 1, 9, 256), (128, 3, 9, 256)]
FP8_SHAPES = [(2, 7, 17, 136), (2, 16, 26, 128)]


def tiling(B, H, W, C):
    """The band height bicubic.hip picks and whether the forward runs its small-map form (tiling there), to see that the shapes reach
    each of them."""
    wgs = -(-W * (C // 8) // 256) * B
    R = 8
    while R > 2 and -(-H // R) * wgs < 256:
        R //= 2
    return R, -(-H // R) * wgs < 256


def test_shapes_reach_every_band_height_and_a_second_strip():
    for banded_forward in (False, True):
        by_r = {}
        for s in SHAPES:
            R, small = tiling(*s)
            if not (banded_forward and small):
                by_r.setdefault(R, []).append(s)
        assert sorted(by_r) == [2, 4, 8]
        for R, shapes in by_r.items():
            hs = {s[1] for s in shapes}
            assert R + 1 in hs and 2 * R - 1 in hs, (R, hs)
            # more than one workgroup across a row, the last one partly filled
            assert any(s[2] * (s[3] // 8) > 256 and s[2] * (s[3] // 8) % 256 for s in shapes), R
    assert any(tiling(*s)[1] for s in SHAPES)
    assert any(256 % (C // 8) == 0 and W == 256 // (C // 8) + 1 for _, _, W, C in SHAPES)         # W = S + 1


def matrix(n):
    m = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        k = o // 2
        for t in range(4):
            i = (k - 1 if o & 1 else k - 2) + t
            m[o, min(max(i, 0), n - 1)] += (WO if o & 1 else WE)[t]
    return m


def forward64(x, H, W):
    """x [B, H, W, C] float64 -> y [B, 2H, 2W, C] and the same product of absolute values."""
    By, Bx = matrix(H), matrix(W)
    y = torch.einsum("oh,bhwc->bowc", By, x)
    a = torch.einsum("oh,bhwc->bowc", By.abs(), x.abs())
    return torch.einsum("pw,bowc->bopc", Bx, y) + 0.0, torch.einsum("pw,bowc->bopc", Bx.abs(), a)


def backward64(dy, H, W):
    """dy [B, 2H, 2W, C] float64 -> dx [B, H, W, C] and the same product of absolute values."""
    By, Bx = matrix(H), matrix(W)
    d = torch.einsum("oh,bopc->bhpc", By, dy)
    a = torch.einsum("oh,bopc->bhpc", By.abs(), dy.abs())
    return torch.einsum("pw,bhpc->bhwc", Bx, d) + 0.0, torch.einsum("pw,bhpc->bhwc", Bx.abs(), a)


def L():
    from camradepth_amd import lib
    return lib, lib.load()


def guarded(B, rows, ld, fill=SENTINEL):
    """[B * rows + guard rows, ld] bf16 on the GPU, all sentinel; the view of the B * rows payload rows and the whole buffer."""
    guard = 4
    buf = torch.full((B * rows + guard, ld), fill, dtype=torch.bfloat16, device="cuda")
    return buf[:B * rows].view(B, rows, ld), buf


def bits(t):
    return t.contiguous().view(torch.int16)


def draw(shape, exact, g):
    if exact:
        return torch.randint(-8, 9, shape, generator=g).to(torch.float64)
    return torch.randn(shape, generator=g).to(torch.bfloat16).to(torch.float64)


def run_forward(x64, B, H, W, C):
    lib, lb = L()
    xd = torch.full((B, H * W, C + 8), SENTINEL, dtype=torch.bfloat16, device="cuda")
    xd[..., 8:] = x64.reshape(B, H * W, C).to(torch.bfloat16).cuda()
    outs = []
    for _ in range(2):
        y, buf = guarded(B, 4 * H * W, C + 16)
        lib.check(lb.crd_bicubic2x(xd.data_ptr(), C + 8, 8, B, H, W, C, buf.data_ptr(), C + 16, 0, lib.stream()), "bicubic")
        torch.cuda.synchronize()
        assert bool((buf[B * 4 * H * W:] == SENTINEL).all()) and bool((y[..., C:] == SENTINEL).all()), "forward wrote outside its columns"
        outs.append(y[..., :C].cpu().reshape(B, 2 * H, 2 * W, C))
    assert torch.equal(bits(outs[0]), bits(outs[1])), "the second forward run differs"
    assert bool((xd[..., :8] == SENTINEL).all())
    return outs[0]


def run_backward(dy64, old64, B, H, W, C, accumulate):
    lib, lb = L()
    dyd = torch.full((B, 4 * H * W, C + 16), SENTINEL, dtype=torch.bfloat16, device="cuda")
    dyd[..., :C] = dy64.reshape(B, 4 * H * W, C).to(torch.bfloat16).cuda()
    outs = []
    for _ in range(2):
        dx, buf = guarded(B, H * W, C + 8)
        dx[..., 8:] = old64.reshape(B, H * W, C).to(torch.bfloat16).cuda() if accumulate else -SENTINEL
        lib.check(lb.crd_bicubic2x_bwd(dyd.data_ptr(), C + 16, 0, B, H, W, C, buf.data_ptr(), C + 8, 8, accumulate, lib.stream()), "bicubic_bwd")
        torch.cuda.synchronize()
        assert bool((buf[B * H * W:] == SENTINEL).all()) and bool((dx[..., :8] == SENTINEL).all()), "backward wrote outside its columns"
        outs.append(dx[..., 8:].cpu().reshape(B, H, W, C))
    assert torch.equal(bits(outs[0]), bits(outs[1])), "the second backward run differs"
    return outs[0]


def check_exact(got, ref64, what):
    want = ref64.to(torch.float32).to(torch.bfloat16)               # (the bf16 rounding is the only one: ref64 is exact in fp32)
    assert torch.equal(ref64.to(torch.float32).to(torch.float64), ref64), what + ": the reference is not exact in fp32"
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from bf16(float64), first at {bad.nonzero()[0].tolist()}"


def check_random(got, ref64, abs64, n, what):
    err = (got.to(torch.float64) - ref64).abs()
    bound = 2.0 ** -8 * ref64.abs() + n * 2.0 ** -23 * abs64
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest error / bound {worst:.3f}, largest |error| {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: error / bound up to {worst:.3f}"


@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_forward_and_transpose_against_float64(B, H, W, C):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C)
    for exact in (True, False):
        x = draw((B, H, W, C), exact, g)
        ref, a = forward64(x, H, W)
        got = run_forward(x, B, H, W, C)
        if exact:
            check_exact(got, ref, f"forward {H} x {W} x {C}")
        else:
            check_random(got, ref, a, 16, f"forward {H} x {W} x {C}")
        dy, old = draw((B, 2 * H, 2 * W, C), exact, g), draw((B, H, W, C), exact, g)
        ref, a = backward64(dy, H, W)
        for accumulate in (0, 1):
            got = run_backward(dy, old, B, H, W, C, accumulate)
            want, wa = (ref + old + 0.0, a + old.abs()) if accumulate else (ref, a)
            if exact:
                check_exact(got, want, f"transpose {H} x {W} x {C} accumulate {accumulate}")
            else:
                check_random(got, want, wa, 100, f"transpose {H} x {W} x {C} accumulate {accumulate}")


@pytest.mark.parametrize("B,H,W,C", FP8_SHAPES)
def test_fp8_forms_equal_the_quantised_bf16_output(B, H, W, C):
    lib, lb = L()
    g = torch.Generator().manual_seed(77 + H)
    x = (torch.randn(B, H * W, C + 8, generator=g) * 2).to(torch.bfloat16).cuda()
    scale, ld8, rows = 0.013, -(-(C + 16) // 16) * 16, B * 4 * H * W
    y16 = torch.zeros(B, 4 * H * W, C + 16, dtype=torch.bfloat16, device="cuda")
    lib.check(lb.crd_bicubic2x(x.data_ptr(), C + 8, 8, B, H, W, C, y16.data_ptr(), C + 16, 0, lib.stream()), "bicubic")
    ref8 = torch.full((rows + 4, ld8), 0x55, dtype=torch.uint8, device="cuda")
    lib.check(lb.crd_quant_fp8(y16.data_ptr(), rows, C + 16, 0, C, ref8.data_ptr(), ld8, 8, scale, lib.stream()), "quant")
    got8 = torch.full_like(ref8, 0x55)
    lib.check(lb.crd_bicubic2x_fp8(x.data_ptr(), C + 8, 8, B, H, W, C, got8.data_ptr(), ld8, 8, scale, None, 0, 0, lib.stream()), "bicubic_fp8")
    torch.cuda.synchronize()
    assert torch.equal(got8, ref8) and int((ref8[:rows, 8:8 + C] != 0x55).sum()) > rows
    got8.fill_(0x55)
    both, buf = guarded(B, 4 * H * W, C + 16)
    lib.check(lb.crd_bicubic2x_fp8(x.data_ptr(), C + 8, 8, B, H, W, C, got8.data_ptr(), ld8, 8, scale, buf.data_ptr(), C + 16, 0, lib.stream()),
              "bicubic_fp8 with the bf16 output")
    torch.cuda.synchronize()
    assert torch.equal(got8, ref8) and torch.equal(bits(both[..., :C]), bits(y16[..., :C]))
    assert bool((both[..., C:] == SENTINEL).all()) and bool((buf[rows:] == SENTINEL).all())
