"""CPU: the float64 stage reference of the fused Mlp (tests/mlp_ref.py) and its bounds, without a GPU.

* the stage functions agree with torch's own float64 group_norm / conv / gelu (an independent formulation: layouts, tap order);
* a "device" that rounds every stage's reference value exactly where the definition does passes every stage bound and the sums check;
* each mutant of mlp_ref.MUTANTS -- a kernel wrong in one subtle way -- is REJECTED by the bound of its stage (or by the sums check),
  while the stages it does not touch still pass: the bounds can fail;
* the erf / rsqrt allowances of the module docstring are measured here against float64;
* the facts of every GPU case (supported value, instantiation, row tiles, LDS bytes, the partition of crd_mlp_reduce) are evaluated from
  the formulas, and crd_mlp_fused_supported of the built library agrees with its Python transcription."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import mlp_ref as R

B, H, W, C = 3, 5, 7, 32                      # N = 35: not a multiple of 32 (NP = 64), W > 1, three samples with distinct dp


@pytest.fixture(scope="module")
def inp():
    return R.make_inputs(B, H, W, C)


@pytest.fixture(scope="module")
def honest(inp):
    return R.fake_device(inp)


def test_stage_functions_agree_with_torch_float64(inp, honest):
    d, hid, N = honest, inp["hid"], inp["N"]

    def cl(t):                                # [B][N][C] -> [B][C][N]
        return t.double().permute(0, 2, 1)

    def same(v, ref, tol=2e-6):
        assert (v - ref.permute(0, 2, 1)).abs().max().item() <= tol * (1 + ref.abs().max().item())

    same(R.stage_xn(inp["x1"], inp["x1_stats"], inp["g0"], inp["b0"])[0], F.group_norm(cl(inp["x1"]), C // 16, inp["g0"].double(), inp["b0"].double(), 1e-5))
    same(R.stage_h1(d["xn"], inp["w1"], inp["b1"])[0], F.conv1d(cl(d["xn"]), inp["w1"].double().unsqueeze(-1), inp["b1"].double()))
    n = R.bf16(F.group_norm(cl(d["h1"]), hid // 16, inp["g1"].double(), inp["b1n"].double(), 1e-5))
    wd = inp["w9"].double().t().reshape(hid, 1, 3, 3)
    ref = F.conv2d(n.reshape(B, hid, H, W), wd, inp["bd"].double(), padding=1, groups=hid).reshape(B, hid, N)
    v, _, extra = R.stage_h2(d["h1"], d["h1_stats"], inp["g1"], inp["b1n"], inp["w9"], inp["bd"], H, W)
    assert bool(((v - ref.permute(0, 2, 1)).abs() <= extra + 2e-6 * (1 + ref.abs().max())).all())
    same(R.stage_h3(d["h2"], d["h2_stats"], inp["g2"], inp["b2n"])[0], F.gelu(F.group_norm(cl(d["h2"]), hid // 64, inp["g2"].double(), inp["b2n"].double(), 1e-5)))
    part = R.stage_part(d["h3"], inp["w2"])[0]
    same(part.sum(0), F.conv1d(cl(d["h3"]), inp["w2"].double().unsqueeze(-1)), 1e-12)
    x2 = R.stage_x2(d["part"], inp["x1"], inp["b2"], inp["dp"])[0]
    same(x2, cl(inp["x1"]) + inp["dp"].double().view(B, 1, 1) * (cl(d["part"].sum(0)) + inp["b2"].double().view(1, C, 1)), 1e-12)


def test_exactly_rounded_stages_pass_every_bound(inp, honest):
    ratios = R.stage_ratios(inp, honest)
    print("max |got - v| / bound:", {k: round(v, 4) for k, v in ratios.items()})
    assert set(ratios) == set(R.STAGES)
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
        assert v > 0.5 or k in ("part", "x2"), (k, v)                # the bf16 term is not slack: a rounding reaches most of it
    for k, (ok, e, r) in R.sums_ratios(honest).items():
        assert ok, (k, e, r)


REJECTED_BY = {
    "mirror_x": ("h2",), "pad_before_norm1": ("h2",), "norm2_over_16": ("h3",), "count_np": ("xn", "h2", "h3"),
    "sums_with_pad_rows": ("h1 sums",), "dp_on_residual": ("x2",), "prev_sample_sums": ("xn", "h2", "h3"), "gelu_tanh": ("h3",)}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_rejected(inp, mutant):
    assert float(inp["b1"].abs().min()) > 0 and R.np_of(inp["N"]) != inp["N"]
    dev = R.fake_device(inp, mutant)
    res = dict(R.stage_ratios(inp, dev))
    res.update({k: (0.0 if ok else max(e, r, 1.0 + 1e-9)) for k, (ok, e, r) in R.sums_ratios(dev).items()})
    print(mutant, {k: round(v, 3) for k, v in res.items()})
    for k, v in res.items():
        if k in REJECTED_BY[mutant]:
            assert v > 1.0, f"{mutant} passes the {k} check ({v:.3f} of its bound)"
        else:
            assert v <= 1.0, f"{mutant} should not disturb {k} ({v:.3f} of its bound)"


def test_allowances_measured_against_float64():
    x = torch.linspace(-12, 12, 2_000_001, dtype=torch.float64).float()
    xd, s = x.double(), math.sqrt(0.5)
    e64 = torch.erf(xd * s)
    lib_erf = (torch.erf(x * s).double() - e64).abs().max().item() / R.U

    def as_erf(t_, dt):
        v = t_.to(dt)
        z = v.abs() * torch.tensor(0.70710678118654752440, dtype=dt)
        E = torch.exp(-z * z)
        t = 1.0 / (1.0 + torch.tensor(0.3275911, dtype=dt) * z)
        c = [torch.tensor(k, dtype=dt) for k in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)]
        poly = t * (c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * c[4]))))
        return torch.copysign(1.0 - poly * E, v).double()

    formula = (as_erf(x, torch.float64) - e64).abs().max().item() / R.U
    fp32 = (as_erf(x, torch.float32) - e64).abs().max().item() / R.U
    print(f"units of 2^-23: torch.erf fp32 {lib_erf:.2f}, A-S 7.1.26 in fp64 {formula:.2f}, in fp32 {fp32:.2f}; ERF_UNITS {R.ERF_UNITS}")
    assert lib_erf <= 0.6 and formula <= 1.26 and fp32 <= 4.6 and fp32 + 3 <= R.ERF_UNITS
    v = torch.rand(1_000_000, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 10 + 1e-5
    r = 1.0 / torch.sqrt(v)
    rs = (((r.float().double() - r).abs() / r).max().item()) / R.U
    print(f"fp32(1 / sqrt) against fp64: {rs:.3f} of 2^-23 relative")
    assert rs <= 0.5
    assert R.C_H3 == 14 and R.C_AFFINE == 7 and R.C_STENCIL == 10 and R.C_PART == 64


def test_facts_of_the_gpu_cases():
    seen = set()
    for name, (Cc, Hh, Ww, Bb, inst, NT) in R.PATH_CASES.items():
        sup, inst_f, NT_f, lds, second = R.path_facts(Cc, Hh, Ww)
        assert sup == 4 * Cc // 64 and inst_f == inst and NT_f == NT and lds <= 160 * 1024, (name, sup, inst_f, NT_f, lds)
        seen.add(inst)
    assert seen == {(n, 1) for n in (1, 2, 4, 5, 8)} | {(n, 4) for n in (1, 2, 4, 5)}                     # every instantiation
    assert R.path_facts(160, 16, 26)[3] == 153088 and max(R.path_facts(c, h, w)[3] for c, h, w, *_ in R.PATH_CASES.values()) == 153088
    assert R.path_facts(160, 11, 23)[4] == 0 and R.path_facts(160, 257, 1)[4] == 1                       # NT = 8 / 9: the second row tile
    assert R.path_facts(64, 1, 128)[1:3] == ((2, 1), 4) and R.path_facts(32, 3, 43)[1] == (1, 4)           # N = 128 / 129
    P = {k: R.reduce_partition(b, n, c) for k, (b, n, c, s) in R.REDUCE_CASES.items()}
    assert P["one_pixel_128_lanes"]["PL"] == 128 and P["one_pixel_128_lanes"]["nblk"] == 1
    assert P["two_workgroups_ragged"]["nblk"] == 2 and 129 % P["two_workgroups_ragged"]["chunk"] != 0
    assert P["idle_threads"]["idle"] == 16
    assert P["one_lane_two_passes"]["PL"] == 1 and R.REDUCE_CASES["one_lane_two_passes"][3] == 5          # slabs 5: passes of 4 + 1
    assert P["production"] == dict(PL=8, idle=0, want=7, cap=341, nblk=7, chunk=15)
    assert P["capped"]["want"] == 10 > P["capped"]["cap"] == 8 and P["capped"]["chunk"] == 5 and P["capped"]["nblk"] == 8
    assert {s % 4 for *_, s in R.REDUCE_CASES.values()} >= {1, 2, 3, 0}                                   # every fill of the last pass


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_predicate_of_the_library(built):
    L = built.load()
    for (Hh, Ww, Cc, hid) in ((1, 129, 256, 1024), (3, 43, 256, 1024), (1, 417, 32, 128), (139, 3, 64, 256), (5, 7, 96, 384), (5, 7, 16, 64),
                              (5, 7, 64, 128), (5, 7, 64, 512), (5, 7, 160, 320), (5, 7, 160, 1280)):
        assert L.crd_mlp_fused_supported(Hh, Ww, Cc, hid) == 0 == R.fused_supported(Hh, Ww, Cc, hid), (Hh, Ww, Cc, hid)
    for name, (Cc, Hh, Ww, *_rest) in R.PATH_CASES.items():
        assert L.crd_mlp_fused_supported(Hh, Ww, Cc, 4 * Cc) == 4 * Cc // 64, name
    for Cc in range(16, 289, 16):
        for N in (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 415, 416, 417):
            for mult in (2, 4, 8):
                assert L.crd_mlp_fused_supported(1, N, Cc, mult * Cc) == R.fused_supported(1, N, Cc, mult * Cc), (Cc, N, mult)


def test_unsupported_shape_is_refused_before_any_launch(built):
    """An argument check: the unsupported status, a message that names the entry, nothing read or written (host memory here)."""
    L = built.load()
    buf = (ctypes.c_ubyte * 4096)(*([0xA5] * 4096))
    a = (ctypes.addressof(buf) + 15) & ~15
    d = built.MlpDesc()
    for n, _t in d._fields_[:20]:
        setattr(d, n, a)
    d.B, d.H, d.W, d.C, d.hidden = 2, 1, 129, 256, 1024
    rc = L.crd_mlp_fwd(ctypes.byref(d), None)
    assert rc == -2 and b"crd_mlp_fwd" in L.crd_last_error(), (rc, L.crd_last_error())
    assert bytes(buf) == b"\xa5" * 4096
    with pytest.raises(built.CrdError):
        built.check(rc, "crd_mlp_fwd")
