"""CPU: the DESIGN of the train-mode mask generator, checked on its numpy restatement (tests/dropout_ref.py).  test_gpu_dropout.py pins
crd_dropout_masks and the live path of Plan.forward to that restatement bit for bit, so what holds here holds for the masks training
draws: per-block keep rates, independence of successive steps, of data-parallel ranks and of the DropPath / Dropout2d streams of one
step, uniformity of u, and the exact value set.

Every bound is a condition from the statistics of independent Bernoulli / uniform draws, fixed before looking at the generator: 4 sigma
of a rate (sigma = sqrt(k (1 - k) / n)), 4 / sqrt(n) for the Pearson correlation of two keep patterns of n elements (its standard
deviation under independence is 1 / sqrt(n)), and the 0.1 % point of chi-square with 15 degrees of freedom.  The generator is
deterministic, so these tests cannot flake: they either hold for the three seeds or they do not."""
import itertools

import numpy as np
import pytest

from camradepth_amd.config import ModelConfig
from tests import dropout_ref as ref

SEEDS = (0, 1234, 777)
CHI2_15_P001 = 37.70          # chi-square, 15 degrees of freedom, upper 0.1 % point


def pearson(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def d2_pattern(seed, epoch, rows=40):
    """Keep pattern (0 / 1) of one Dropout2d draw: rows x 128 at keep 0.8."""
    return (ref.masks(np.full(rows, 0.8, dtype=np.float32), rows, 128, seed, epoch) > 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_drop_path_keep_rate_per_block(seed):
    """Full config (34 blocks, keep 1.0 ... 0.9), B = 8, the DropPath draws of 2000 consecutive steps (counters 0, 2, ..., 3998)."""
    cfg = ModelConfig.variant("base")
    keep = np.array([1.0 - r for r in cfg.drop_path_rates], dtype=np.float32)
    nblk, B, draws = len(keep), 8, 2000
    assert nblk == 34
    kept = np.zeros(nblk)
    for t in range(draws):
        m = ref.masks(keep, nblk, B, seed, 2 * t)
        assert np.all(m[0] == np.float32(1.0)), f"block 0 (keep 1.0) dropped a sample in draw {t}"
        kept += (m > 0).sum(axis=1)
    n = draws * B
    rate = kept / n
    k = keep.astype(np.float64)
    sigma = np.sqrt(k * (1 - k) / n)
    z = np.abs(rate[1:] - k[1:]) / sigma[1:]
    print(f"seed {seed}: DropPath keep rate per block, worst |z| {z.max():.2f} (block {1 + int(z.argmax())})")
    assert rate[0] == 1.0
    assert np.all(z < 4.0), (z.max(), int(z.argmax()) + 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_dropout2d_keep_rate_single_and_pooled(seed):
    n1 = 40 * 128
    sigma1 = np.sqrt(0.8 * 0.2 / n1)
    one = d2_pattern(seed, 1).mean()
    z1 = abs(one - 0.8) / sigma1
    draws = [d2_pattern(seed, c) for c in range(1, 400, 2)]
    assert len(draws) == 200
    pooled = np.mean([d.mean() for d in draws])
    zp = abs(pooled - 0.8) / np.sqrt(0.8 * 0.2 / (200 * n1))
    print(f"seed {seed}: Dropout2d keep rate one draw {one:.4f} (|z| {z1:.2f}), 200 draws {pooled:.5f} (|z| {zp:.2f})")
    assert z1 < 4.0, (one, z1)
    assert zp < 4.0, (pooled, zp)


@pytest.mark.parametrize("seed", SEEDS)
def test_successive_draws_are_uncorrelated(seed):
    """The Dropout2d patterns of consecutive steps (counters c and c + 2)."""
    draws = [d2_pattern(seed, c) for c in range(1, 400, 2)]
    rho = [abs(pearson(a, b)) for a, b in zip(draws[:-1], draws[1:])]
    bound = 4.0 / np.sqrt(5120)
    print(f"seed {seed}: max |rho| of successive Dropout2d draws {max(rho):.4f} (bound {bound:.4f})")
    assert all(not np.array_equal(a, b) for a, b in zip(draws[:-1], draws[1:]))
    assert max(rho) < bound, (max(rho), int(np.argmax(rho)))


@pytest.mark.parametrize("seed", SEEDS)
def test_rank_streams_are_independent(seed):
    """Ranks 0 .. 7 with the engine's seed derivation: the Dropout2d draws of four steps each (20480 elements)."""
    pats = []
    for rank in range(8):
        s = (ref.rank_seed(seed, rank) + 1) & ref.M64
        pats.append(np.concatenate([d2_pattern(s, c).ravel() for c in (1, 3, 5, 7)]))
    assert pats[0].size == 20480
    bound = 4.0 / np.sqrt(20480)
    rho = {}
    for a, b in itertools.combinations(range(8), 2):
        assert not np.array_equal(pats[a], pats[b]), (a, b)
        rho[(a, b)] = abs(pearson(pats[a], pats[b]))
    worst = max(rho, key=rho.get)
    print(f"seed {seed}: max |rho| between ranks {rho[worst]:.4f} {worst} (bound {bound:.4f})")
    assert rho[worst] < bound, (worst, rho[worst])


@pytest.mark.parametrize("seed", SEEDS)
def test_u_is_uniform(seed):
    u = ref.uniforms(1 << 20, seed, 0)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.all(u * np.float32(2.0 ** 24) == np.floor(u * np.float32(2.0 ** 24)))          # multiples of 2^-24
    counts = np.bincount((u * 16).astype(np.int64), minlength=16)
    e = u.size / 16
    chi2 = float(((counts - e) ** 2 / e).sum())
    print(f"seed {seed}: chi-square(15) of 2^20 values of u in 16 bins {chi2:.1f}")
    assert chi2 < CHI2_15_P001, chi2


@pytest.mark.parametrize("seed", SEEDS)
def test_drop_path_and_dropout2d_streams_of_a_step_are_uncorrelated(seed):
    """The engine draws DropPath from (s, c) and Dropout2d from (s + 1, c + 1); the next step's DropPath comes from (s, c + 2).  Compared
    as keep patterns of the same shape and keep (40 x 128, 0.8) so that element i of one stream meets element i of the other."""
    bound = 4.0 / np.sqrt(5120)
    worst = 0.0
    for c in range(0, 16, 2):
        d2 = d2_pattern((seed + 1) & ref.M64, c + 1)
        for cc in (c, c + 2):
            dp = d2_pattern(seed, cc)
            assert not np.array_equal(dp, d2)
            worst = max(worst, abs(pearson(dp, d2)))
    print(f"seed {seed}: max |rho| DropPath stream vs Dropout2d stream {worst:.4f} (bound {bound:.4f})")
    assert worst < bound, worst


def test_engine_streams_of_one_step_differ_at_the_engine_shapes():
    """engine_masks itself: shapes, the u of the two streams at the same element indices differ, and the two extra Dropout2d
    applications of the segmentation variants extend the draw without moving the first five."""
    cfg = ModelConfig.variant("base")
    u_dp = ref.uniforms(34 * 8, ref.rank_seed(5, 0), 10)
    u_d2 = ref.uniforms(34 * 8, ref.rank_seed(5, 0) + 1, 11)
    assert float(np.mean(u_dp == u_d2)) < 0.01
    dp, d2 = ref.engine_masks(cfg, 8, 5, 0, 10)
    assert dp.shape == (34, 8) and d2.shape == (5, 8, 128) and dp.dtype == np.float32 and d2.dtype == np.float32
    dp_seg, d2_seg = ref.engine_masks(ModelConfig.variant("supervised_seg"), 8, 5, 0, 10)
    assert d2_seg.shape == (7, 8, 128) and np.array_equal(dp_seg, dp) and np.array_equal(d2_seg[:5], d2)
    assert not np.array_equal(d2_seg[5], d2_seg[6])
    # rank 0 keeps the constructor's seed; the counter and the seed wrap mod 2^64
    assert ref.rank_seed(1234, 0) == 1234 and ref.rank_seed(ref.M64, 1) == ref.RANK_MUL - 1
    a = ref.masks(np.full(4, 0.8, dtype=np.float32), 4, 16, 3, ref.M64 + 1 + 7)
    assert np.array_equal(a, ref.masks(np.full(4, 0.8, dtype=np.float32), 4, 16, 3 + (1 << 64), 7))


@pytest.mark.parametrize("keep", [0.8, 0.9, 1.0 - 0.1 * 7 / 33, 2.0 ** -20, 1.0 / 3.0])
def test_values_are_zero_or_reciprocal_keep(keep):
    k32 = np.float32(keep)
    m = ref.masks(np.full(64, k32), 64, 333, 1234, 5)
    assert m.dtype == np.float32
    vals = set(np.unique(m).tolist())
    assert vals <= {0.0, float(np.float32(1.0) / k32)}, vals
    if keep > 0.1:
        assert len(vals) == 2


def test_keep_one_and_keep_zero():
    ones = ref.masks(np.ones(16, dtype=np.float32), 16, 1000, 777, 3)
    assert np.all(ones == np.float32(1.0))
    zeros = ref.masks(np.zeros(16, dtype=np.float32), 16, 1000, 777, 3)
    assert np.all(np.isfinite(zeros)) and np.all(zeros == 0.0)
    mixed = ref.masks(np.array([1.0, 0.0, 0.8], dtype=np.float32), 3, 4096, 777, 3)
    assert np.all(mixed[0] == 1.0) and np.all(mixed[1] == 0.0) and np.all(np.isfinite(mixed))
    assert set(np.unique(mixed[2]).tolist()) == {0.0, float(np.float32(1.0) / np.float32(0.8))}


def test_known_answer_of_the_hash():
    """splitmix64's published first outputs for state 0 (Vigna's splitmix64.c: the reference vectors every implementation quotes), so a
    slip in the restatement's constants or shifts is caught here and not only by the GPU comparison."""
    assert ref.mix_int(0) == 0xE220A8397B1DCDAF
    assert ref.mix_int(ref.GAMMA) == 0x6E789E6AA1B965F4
    assert int(ref.mix(np.array([0, ref.GAMMA], dtype=np.uint64))[1]) == 0x6E789E6AA1B965F4
