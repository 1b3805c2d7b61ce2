"""numpy restatement of the train-mode mask generator (crd_dropout_masks, include/camradepth_hip.h) and of the way the engine
derives its two streams, shared by test_dropout_ref_cpu.py and test_gpu_dropout.py.

The generator is counter-based and has no state but (seed, epoch): element i of a draw hashes to
    h = mix(mix(seed ^ epoch * 0xD1342543DE82EF95) + i)          (mix = the splitmix64 finaliser, everything mod 2^64)
its top 24 bits give a uniform u = (h >> 40) * 2^-24 in [0, 1), and out[r][c] = u < keep[r] ? 1 / keep[r] : 0 in fp32, i = r * cols + c:
timm DropPath's per-sample and nn.Dropout2d's per-sample-per-channel Bernoulli(keep) scaled by 1 / keep.  Every step of that is exact
integer or exactly-rounded fp32 arithmetic, so the kernel can be compared with this module bit for bit."""
import numpy as np

M64 = (1 << 64) - 1
EPOCH_MUL = 0xD1342543DE82EF95
RANK_MUL = 0x632BE59BD9B4E019          # engine.py: one stream per data-parallel rank
GAMMA, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MID_CHANNELS = 128
D2_KEEP = 0.8                          # nn.Dropout2d(0.2)


def mix_int(x):
    """splitmix64 of one Python integer."""
    x = (x + GAMMA) & M64
    x = ((x ^ (x >> 30)) * MUL1) & M64
    x = ((x ^ (x >> 27)) * MUL2) & M64
    return x ^ (x >> 31)


def mix(x):
    """splitmix64 of a uint64 array (numpy's unsigned arithmetic wraps mod 2^64)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(GAMMA)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(MUL1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(MUL2)
    return x ^ (x >> np.uint64(31))


def uniforms(n, seed, epoch):
    """u of elements 0 .. n-1 of the draw (seed, epoch): float32, multiples of 2^-24 in [0, 1)."""
    seed, epoch = int(seed) & M64, int(epoch) & M64
    base = mix_int(seed ^ ((epoch * EPOCH_MUL) & M64))
    with np.errstate(over="ignore"):
        h = mix(np.uint64(base) + np.arange(n, dtype=np.uint64))
    top = (h >> np.uint64(40)).astype(np.float32)              # < 2^24: exact in fp32
    return top * np.float32(2.0 ** -24)


def masks(keep, rows, cols, seed, epoch):
    """-> float32 [rows, cols]; keep: one keep probability per row (taken as float32)."""
    keep = np.asarray(keep, dtype=np.float32).reshape(rows)
    u = uniforms(rows * cols, seed, epoch).reshape(rows, cols)
    with np.errstate(divide="ignore"):
        scale = np.float32(1.0) / keep                         # fp32 division, correctly rounded; keep = 0 is never selected
    return np.where(u < keep[:, None], scale[:, None], np.float32(0.0)).astype(np.float32)


def rank_seed(seed, rank):
    return (int(seed) + int(rank) * RANK_MUL) & M64


def engine_masks(cfg, B, seed, rank, counter):
    """The two draws at the top of one train-mode Plan.forward whose counter reads `counter` -> (DropPath [blocks, B],
    Dropout2d [n_drop, B, 128]); the counter reads counter + 2 afterwards."""
    s = rank_seed(seed, rank)
    dp_keep = np.array([1.0 - r for r in cfg.drop_path_rates], dtype=np.float32)      # the subtraction in double, then rounded
    nblk = len(dp_keep)
    n_drop = 5 + (2 if (cfg.supervised_seg or cfg.unsupervised_seg) else 0)
    dp = masks(dp_keep, nblk, B, s, counter)
    d2 = masks(np.full(n_drop * B, D2_KEEP, dtype=np.float32), n_drop * B, MID_CHANNELS, (s + 1) & M64, (int(counter) + 1) & M64)
    return dp, d2.reshape(n_drop, B, MID_CHANNELS)
