"""GPU: the LIVE DropPath / Dropout2d masks -- crd_dropout_masks (k_dropout_masks + k_counter_inc, csrc/train_ops.hip) and the two
launches at the top of Plan.forward -- against the numpy restatement of the generator (tests/dropout_ref.py), bit for bit.

Every training-parity test injects synth.make_masks and switches the live draw off (plan.training_masks_fixed); what users train with is
the live draw.  Checked here: (a) the kernel over shapes below and above its 64-workgroup grid cap, keep edge values, 64-bit seeds and
counters, the counter increment and the stream; (b) the engine's seed / rank / counter derivation through model.forward; (c) a fresh
draw per step, in counter order, under HIP-graph replay, across the captured variants of an accumulation schedule and per plan;
(d) a live training run equals, to the bit, the same run with its recorded masks injected -- the injected-mask path is the one every
parity test validates -- including the late-stream weight gradients at the benchmark size; (e) eval mode ignores the masks.

Equality is exact everywhere: the hash is integer arithmetic, u = (h >> 40) * 2^-24 is exact in fp32, 1.0f / keep is an IEEE division
(the library is built without fast-math flags), and the training step is bit-reproducible (test_training_iteration_is_bit_reproducible).

Counter offsets (read from the plan and printed by the step tests, pytest -s; nothing here assumes them).  As the code reads: a plan's
counter is 0 after construction; the eager step leaves it at 2k after k steps; the graph step's capture warm-up iteration draws once
and is not rolled back, so the k-th replayed step draws from counter 2k (the first from 2) where the k-th eager step draws from
2(k - 1)."""
import dataclasses
import gc

import numpy as np
import pytest
import torch

from camradepth_amd import synth
from camradepth_amd.config import ModelConfig
from camradepth_amd.params import param_specs
from tests import dropout_ref as ref

pytestmark = pytest.mark.gpu

M64 = ref.M64
TINY = (1, 1, 1, 1)
GUARD = 256                          # floats behind every output buffer that the kernel must leave alone
SENTINEL = -7.0


# ------------------------------------------------------------------------------------------------------------ helpers
def to_i64(v):
    """A uint64 value as the int64 the counter tensor holds."""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def set_counter(t, v):
    t.fill_(to_i64(v))


def get_counter(t):
    return int(t.item()) & M64


def draw(lib, keep, rows, cols, seed, counter, out=None):
    """One crd_dropout_masks call on torch's current stream -> the whole output buffer (rows * cols values + guard)."""
    from camradepth_amd import lib as L
    if out is None:
        out = torch.full((rows * cols + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(lib.crd_dropout_masks(out.data_ptr(), keep.data_ptr(), rows, cols, seed, counter.data_ptr(), L.stream()), "crd_dropout_masks")
    return out


def assert_draw(out, keep_host, rows, cols, seed, epoch, what):
    n = rows * cols
    want = torch.from_numpy(ref.masks(keep_host, rows, cols, seed, epoch)).reshape(-1).cuda()
    got = out[:n]
    if not torch.equal(got, want):
        bad = (got != want).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {n} values differ from the restatement; first at element {i} (row {i // cols}, "
                             f"col {i % cols}): kernel {float(got[i])!r}, restatement {float(want[i])!r}")
    assert bool((out[n:] == SENTINEL).all()), f"{what}: the kernel wrote behind its {n} outputs"


def keep_vectors(rows):
    """name -> float32 [rows].  The special values sit on every third row (on the only row when rows == 1) among rows of 0.8."""
    rates = ModelConfig.variant("base").drop_path_rates
    assert len(rates) == 34
    out = {"drop_path": np.array([1.0 - rates[r % 34] for r in range(rows)], dtype=np.float32),
           "const_0.8": np.full(rows, 0.8, dtype=np.float32)}
    for name, v in (("rows_of_1", 1.0), ("rows_of_0", 0.0), ("rows_of_2^-20", 2.0 ** -20)):
        k = np.full(rows, 0.8, dtype=np.float32)
        k[::3] = v
        out[name] = k
    return out


SHAPES = [(1, 1), (34, 8), (34, 16), (34, 3), (40, 128), (112, 128), (7, 333),
          (40, 1000),            # 40000 elements > the 64 workgroups x 256 threads of the launch: the grid-stride loop runs
          (1024, 1024)]
SEEDS = (0, 1234, (1 << 63) + 5, M64, ref.rank_seed(0, 7))
COUNTERS = (0, 1, (1 << 32) + 3, (1 << 63) + 1)


def build(cfg, sd=None, train=True, seed=0):
    from camradepth_amd.model import CamRaDepth
    m = CamRaDepth(input_channels=cfg.input_channels, depths=cfg.depths, supervised_seg=cfg.supervised_seg,
                   unsupervised_seg=cfg.unsupervised_seg, seed=seed)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda().train(train)


def config(variant, depths=TINY):
    cfg = ModelConfig.variant(variant)
    return cfg if depths is None else dataclasses.replace(cfg, depths=depths)


def assert_plan_masks(plan, cfg, B, seed, rank, counter, what):
    """plan.dp_masks / plan.d2_masks are the engine's two draws for a forward that began with the plan's counter at `counter`."""
    dp, d2 = ref.engine_masks(cfg, B, seed, rank, counter)
    for name, got, want in (("DropPath", plan.dp_masks, dp), ("Dropout2d", plan.d2_masks, d2)):
        want = torch.from_numpy(want).cuda()
        assert got.shape == want.shape, (what, name, tuple(got.shape), tuple(want.shape))
        if not torch.equal(got, want):
            raise AssertionError(f"{what}: {name} masks differ from the restatement at counter {counter} in "
                                 f"{int((got != want).sum())} of {want.numel()} values")


def cuda_batches(B, H, W, n, seed0):
    return [{k: v.cuda() for k, v in synth.make_batch(B, H, W, seed=seed0 + i).items()} for i in range(n)]


def snap(plan):
    return plan.dp_masks.clone(), plan.d2_masks.clone()


# ------------------------------------------------------------------------------------------------------------ (a) the kernel
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_kernel_equals_restatement(rows, cols):
    from camradepth_amd import lib as L
    lib = L.load()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    n = 0
    for name, keep_host in keep_vectors(rows).items():
        keep = torch.from_numpy(keep_host).cuda()
        for seed in SEEDS:
            for c in COUNTERS:
                set_counter(counter, c)
                out = draw(lib, keep, rows, cols, seed, counter)
                assert_draw(out, keep_host, rows, cols, seed, c, f"{rows}x{cols} keep={name} seed={seed:#x} counter={c:#x}")
                assert get_counter(counter) == (c + 1) & M64, (name, hex(seed), hex(c), hex(get_counter(counter)))
                n += 1
    assert n == 5 * len(SEEDS) * len(COUNTERS)


def test_kernel_special_rows_hold_their_exact_values():
    """keep = 1 rows are all ones, keep = 0 rows all zeros and finite, the others exactly {0, fp32(1) / fp32(keep)} -- on the kernel's
    output itself, not only through the restatement."""
    from camradepth_amd import lib as L
    lib = L.load()
    rows, cols = 34, 1000
    keep_host = np.array([1.0 - r for r in ModelConfig.variant("base").drop_path_rates], dtype=np.float32)
    keep_host[5], keep_host[6] = 0.0, 2.0 ** -20
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    set_counter(counter, 12345)
    out = draw(lib, torch.from_numpy(keep_host).cuda(), rows, cols, 777, counter)[:rows * cols].reshape(rows, cols).cpu().numpy()
    assert np.all(np.isfinite(out))
    assert np.all(out[0] == 1.0) and np.all(out[5] == 0.0)
    for r in range(rows):
        if keep_host[r] > 0:
            assert set(np.unique(out[r]).tolist()) <= {0.0, float(np.float32(1.0) / keep_host[r])}, r


def test_two_calls_back_to_back_use_consecutive_counters():
    """The increment is a launch of its own behind the draw, on the same stream: the second call reads counter + 1 without any host
    synchronisation in between (this is what Plan.forward does)."""
    from camradepth_amd import lib as L
    lib = L.load()
    keep_a = np.array([1.0 - r for r in ModelConfig.variant("base").drop_path_rates], dtype=np.float32)
    keep_b = np.full(40, 0.8, dtype=np.float32)
    ka, kb = torch.from_numpy(keep_a).cuda(), torch.from_numpy(keep_b).cuda()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    for c in (0, (1 << 32) - 1, M64):                   # (the last one wraps to 0)
        set_counter(counter, c)
        a = draw(lib, ka, 34, 8, 99, counter)
        b = draw(lib, kb, 40, 128, 100, counter)
        a2 = draw(lib, ka, 34, 8, 99, counter)
        assert_draw(a, keep_a, 34, 8, 99, c, f"first call at {c:#x}")
        assert_draw(b, keep_b, 40, 128, 100, (c + 1) & M64, f"second call at {c:#x}")
        assert_draw(a2, keep_a, 34, 8, 99, (c + 2) & M64, f"third call at {c:#x}")
        assert get_counter(counter) == (c + 3) & M64
        assert not torch.equal(a, a2)


def test_kernel_runs_on_the_stream_it_is_given():
    """On a non-default stream, eagerly and captured into a HIP graph on that stream: a launch that ignored the stream argument would
    execute during the capture (or break it) instead of being recorded.  Capturing executes nothing; every replay reads the counter on
    the device and so draws the next masks."""
    from camradepth_amd import lib as L
    lib = L.load()
    rows, cols, seed = 40, 128, (1 << 63) + 5
    keep_host = np.full(rows, 0.8, dtype=np.float32)
    keep = torch.from_numpy(keep_host).cuda()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    set_counter(counter, 10)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = draw(lib, keep, rows, cols, seed, counter)
    s.synchronize()
    assert_draw(out, keep_host, rows, cols, seed, 10, "eager call on a side stream")
    assert get_counter(counter) == 11
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        draw(lib, keep, rows, cols, seed, counter, out=out)
    torch.cuda.synchronize()
    assert get_counter(counter) == 11 and bool((out == SENTINEL).all()), "the call executed while it was being captured"
    seen = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert_draw(out, keep_host, rows, cols, seed, 11 + k, f"graph replay {k}")
        assert get_counter(counter) == 12 + k
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ------------------------------------------------------------------------------------------------------------ (b) model draws
@pytest.mark.parametrize("variant,depths,n_drop", [("base", TINY, 5), ("supervised_seg", TINY, 7), ("base", None, 5)])
def test_model_forward_draws_the_engine_streams(variant, depths, n_drop):
    """One eager train-mode forward: both mask buffers equal the restatement of the engine's derivation for the model's seed, its
    data-parallel rank (the constructor's default, 0, 1, 7) and the plan's counter, which advances by 2."""
    cfg = config(variant, depths)
    B, seed = 2, 0x1234567890ABCDEF
    m = build(cfg, seed=seed)
    assert m.seed == seed
    x = synth.make_batch(B, 64, 96, seed=3)["image"].cuda()
    plan = m._plan_for(x)
    assert plan.dp_masks.shape == (sum(cfg.depths), B) and plan.d2_masks.shape == (n_drop, B, 128)
    drawn = []
    for rank in (None, 0, 1, 7):
        if rank is not None:
            m.rng_rank = rank
        c0 = get_counter(plan.rng_counter)
        m(x)
        torch.cuda.synchronize()
        assert m._plans[m._plan_key(x)] is plan
        assert_plan_masks(plan, cfg, B, seed, rank or 0, c0, f"{variant} rank {rank}")
        assert get_counter(plan.rng_counter) == c0 + 2, (rank, c0, get_counter(plan.rng_counter))
        assert bool((plan.dp_masks[0] == 1.0).all()), "the first block (keep 1.0) dropped a sample"
        drawn.append(snap(plan))
    for i in range(len(drawn)):
        for j in range(i + 1, len(drawn)):
            assert not torch.equal(drawn[i][1], drawn[j][1]), (i, j)
    # a counter beyond 32 bits and another seed reach the kernel whole (ctypes binding, engine arithmetic)
    m.seed, m.rng_rank = M64 - 2, 7
    set_counter(plan.rng_counter, (1 << 32) + 3)
    m(x)
    torch.cuda.synchronize()
    assert_plan_masks(plan, cfg, B, M64 - 2, 7, (1 << 32) + 3, f"{variant} 64-bit seed and counter")
    assert get_counter(plan.rng_counter) == (1 << 32) + 5


# ------------------------------------------------------------------------------------------------------------ (c) every step fresh
def live_steps(ts, m, cfg, B, batches, what):
    """Runs one step that captures (graph path) and then len(batches) - 1 more, checking each step's masks against the restatement
    at the counter read before the FIRST of them + 2k.  Returns the recorded masks."""
    plan = ts.plan
    c_built = get_counter(plan.rng_counter)
    ts.set_batch(batches[0])
    ts.step()
    torch.cuda.synchronize()
    c = get_counter(plan.rng_counter)
    print(f"{what}: counter {c_built} after construction, {c} after the first step (warm-up offset {c - c_built - 2})")
    assert_plan_masks(plan, cfg, B, m.seed, 0, (c - 2) & M64, f"{what} first step")
    rec = [snap(plan)]
    for k, b in enumerate(batches[1:]):
        ts.set_batch(b)
        ts.step()
        torch.cuda.synchronize()
        assert_plan_masks(plan, cfg, B, m.seed, 0, c + 2 * k, f"{what} step {k}")
        assert get_counter(plan.rng_counter) == c + 2 * (k + 1), (what, k)
        rec.append(snap(plan))
    # no two steps share their masks.  (Stated on the Dropout2d buffer, n_drop x B x 128 values: the DropPath buffer of the shallow
    # configurations is 4 x B values at keep >= 0.9, where two independent draws coincide -- all ones -- more often than not.)
    for i in range(len(rec)):
        for j in range(i + 1, len(rec)):
            assert not torch.equal(rec[i][1], rec[j][1]), (what, "Dropout2d", i, j)
    return rec


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (3, 96, 160)])
def test_every_training_step_draws_fresh_masks_in_counter_order(B, H, W, use_graph):
    from camradepth_amd.trainer import TrainStep
    cfg = config("base")
    m = build(cfg, seed=31337)
    ts = TrainStep(m, B, H, W, lr=1e-3, use_graph=use_graph)
    rec = live_steps(ts, m, cfg, B, cuda_batches(B, H, W, 6, 400), f"{B}x{H}x{W} graph={use_graph}")
    assert len(rec) == 6          # the capturing step + 5


@pytest.mark.parametrize("use_graph", [True, False])
def test_counter_runs_on_across_the_graphs_of_an_accumulation_schedule(use_graph):
    """update_interval = 3 as in test_gradient_accumulation_matches_oracle_and_reference_loop: the iterations of a window replay three
    different captured variants (zero / accumulate / accumulate + optimizer); the counter lives in the plan, not in a graph."""
    from camradepth_amd.trainer import TrainStep
    cfg = config("base")
    B = 2
    m = build(cfg, seed=5)
    ts = TrainStep(m, B, 64, 96, lr=1e-3, update_interval=3, use_graph=use_graph)
    batches = cuda_batches(B, 64, 96, 8, 50)
    ran = []
    orig_step = ts.step

    def step(*a, **k):
        ran.append(orig_step(*a, **k))
        return ran[-1]
    ts.step = step
    live_steps(ts, m, cfg, B, batches, f"accumulation graph={use_graph}")
    assert ran == [False, False, True, False, False, True, False, False]
    if use_graph:
        assert set(ts.graphs) == {(True, False), (False, False), (False, True)}


@pytest.mark.parametrize("use_graph", [True, False])
def test_second_train_step_on_a_ragged_batch_draws_for_its_own_plan(use_graph):
    """The last batch of an epoch is smaller (TrainState is shared, the plan is not): the second TrainStep's masks are the restatement
    for ITS rows x cols = B' and ITS counter, and the first one's stream is not disturbed by it."""
    from camradepth_amd.trainer import TrainStep
    cfg = config("supervised_seg")
    m = build(cfg, seed=2024)
    ts = TrainStep(m, 3, 64, 96, lr=1e-3, use_graph=use_graph)
    big = cuda_batches(3, 64, 96, 4, 60)
    live_steps(ts, m, cfg, 3, big[:2], f"ragged: full batch graph={use_graph}")
    c_big = get_counter(ts.plan.rng_counter)
    ts2 = TrainStep(m, 1, 64, 96, use_graph=use_graph, state=ts.state)
    assert ts2.plan is not ts.plan and ts2.plan.rng_counter.data_ptr() != ts.plan.rng_counter.data_ptr()
    assert ts2.plan.dp_masks.shape == (4, 1) and ts2.plan.d2_masks.shape == (7, 1, 128)
    live_steps(ts2, m, cfg, 1, cuda_batches(1, 64, 96, 3, 70), f"ragged: last batch graph={use_graph}")
    assert get_counter(ts.plan.rng_counter) == c_big
    for k, b in enumerate(big[2:]):
        ts.set_batch(b)
        ts.step()
        torch.cuda.synchronize()
        assert_plan_masks(ts.plan, cfg, 3, m.seed, 0, c_big + 2 * k, f"ragged: full batch again, step {k}")
    assert get_counter(ts.plan.rng_counter) == c_big + 4


# ------------------------------------------------------------------------------------------------------------ (d) live = injected
def run_live(cfg, sd, B, H, W, batches, use_graph, lr):
    from camradepth_amd.trainer import TrainStep
    m = build(cfg, sd)
    ts = TrainStep(m, B, H, W, lr=lr, use_graph=use_graph)
    rec = []
    for b in batches:
        ts.set_batch(b)
        assert ts.step() is True
        torch.cuda.synchronize()
        rec.append((snap(ts.plan), ts.losses(), m.flat_grad.clone()))
    return m, ts, rec, m.flat.clone()


def run_injected(cfg, sd, B, H, W, batches, use_graph, lr, masks):
    from camradepth_amd.trainer import TrainStep
    m = build(cfg, sd)
    ts = TrainStep(m, B, H, W, lr=lr, use_graph=use_graph)
    ts.plan.training_masks_fixed = True
    rec = []
    for b, (dp, d2) in zip(batches, masks):
        ts.plan.dp_masks.copy_(dp)
        ts.plan.d2_masks.copy_(d2)
        ts.set_batch(b)
        assert ts.step() is True
        torch.cuda.synchronize()
        rec.append((snap(ts.plan), ts.losses(), m.flat_grad.clone()))
    assert get_counter(ts.plan.rng_counter) == 0, "the injected-mask run drew masks"
    return m, ts, rec, m.flat.clone()


def assert_same_run(live, inj, what):
    (_, _, rl, pl), (_, _, ri, pi) = live, inj
    for k, ((ml, ll, gl), (mi, li, gi)) in enumerate(zip(rl, ri)):
        assert torch.equal(ml[0], mi[0]) and torch.equal(ml[1], mi[1]), (what, k)
        assert ll == li, (what, k, ll, li)
        assert all(np.isfinite(v) for v in ll.values()), (what, k, ll)
        if not torch.equal(gl, gi):
            d = (gl.double() - gi.double()).norm() / gi.double().norm()
            raise AssertionError(f"{what}: the gradient of step {k} with live masks differs from the one with the same masks injected "
                                 f"(rel-L2 {float(d):.3e})")
        assert float(gl.abs().sum()) > 0
    assert torch.equal(pl, pi), f"{what}: the weights after {len(rl)} steps differ between live and injected masks"


@pytest.mark.parametrize("variant", ["base", "supervised_seg"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_live_masks_equal_the_same_masks_injected(use_graph, variant):
    """Three live steps, then the same three steps from the same weights with each step's recorded masks copied in and the live draw
    switched off: losses and gradients of every step and the final weights are the same bits.  The backward and the late-stream weight
    gradients of step N therefore saw step N's masks, and the live path is the injected-mask path with another mask source."""
    cfg = config(variant)
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batches = cuda_batches(2, 64, 96, 3, 70)
    live = run_live(cfg, sd, 2, 64, 96, batches, use_graph, 1e-3)
    masks = [r[0] for r in live[2]]
    assert not torch.equal(masks[0][1], masks[1][1]) and not torch.equal(masks[1][1], masks[2][1])
    inj = run_injected(cfg, sd, 2, 64, 96, batches, use_graph, 1e-3, masks)
    assert_same_run(live, inj, f"{variant} graph={use_graph}")


def test_live_masks_equal_injected_at_benchmark_size_with_the_late_stream():
    """8 x 7 x 256 x 416, full depth, graph step with the weight gradients on the late stream, two steps: the late stream's kernels of
    step 1 still run while the main stream is at the tail of that step -- they must be done before step 2 redraws the masks."""
    cfg = config("base", None)
    B, H, W = 8, 256, 416
    m0 = build(cfg)
    sd = {k: v.detach().cpu().clone() for k, v in m0.state_dict().items()}
    del m0
    batches = cuda_batches(B, H, W, 2, 1234)
    live = run_live(cfg, sd, B, H, W, batches, True, 6e-5)
    assert live[1].late_wgrad
    c = get_counter(live[1].plan.rng_counter)
    assert_plan_masks(live[1].plan, cfg, B, live[0].seed, 0, c - 2, "benchmark size, second step")
    masks = [r[0] for r in live[2]]
    assert not torch.equal(masks[0][0], masks[1][0]) and not torch.equal(masks[0][1], masks[1][1])
    final_live = (live[2], live[3])
    live = (None, None, final_live[0], final_live[1])       # drop the first model and its graphs before building the second
    gc.collect()
    torch.cuda.empty_cache()
    inj = run_injected(cfg, sd, B, H, W, batches, True, 6e-5, masks)
    assert inj[1].late_wgrad
    assert_same_run(live, inj, "benchmark size, late stream")


# ------------------------------------------------------------------------------------------------------------ (e) eval ignores them
@pytest.mark.parametrize("use_graph", [True, False])
def test_eval_forward_ignores_the_masks(use_graph):
    cfg = config("supervised_seg")
    sd = synth.fill_state_dict({n: s for n, s in param_specs(cfg)}, 0)
    batches = cuda_batches(2, 64, 96, 3, 70)
    m, ts, _, _ = run_live(cfg, sd, 2, 64, 96, batches, use_graph, 1e-3)
    c = get_counter(ts.plan.rng_counter)
    x = batches[0]["image"]
    m.eval()
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    assert get_counter(ts.plan.rng_counter) == c, "an eval forward drew masks"
    fresh = build(cfg, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, train=False, seed=99)
    with torch.no_grad():
        want = fresh(x)
    torch.cuda.synchronize()
    assert torch.equal(out["depth"]["final_depth"], want["depth"]["final_depth"])
    for a, b in zip(out["depth"]["intermediate_depths"][2:], want["depth"]["intermediate_depths"][2:]):
        assert torch.equal(a, b)
    assert torch.equal(out["seg"]["final_seg"], want["seg"]["final_seg"])
    assert bool(torch.isfinite(out["depth"]["final_depth"]).all())
