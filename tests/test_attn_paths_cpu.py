"""Which launch path the attention backward kernels take at the shapes tests/test_gpu_attention.py runs, pinned through the two
host-side queries of the C ABI (no GPU: the queries are host arithmetic).  The launchers pick a kernel's geometry from the problem
size, so a retune of those rules can move a GPU test off the path it was written for without failing it; it fails here instead.

Path classes of k_attn_scores_bwd: `parts` workgroups per sample (0: the global-atomics fallback), each with a chunk of
ceil(N / parts) pixels and ceil(chunk / 32) mask words per (head, key).  Of k_attn_out_bwd: workgroups per sample, chunk as above;
a chunk above 32 pixels is the 256-pixel branch, parts * B == 1024 the workgroup cap."""
import pytest


def cdiv(a, b):
    return -(-a // b)


# (B, N, M, heads, d) -> (parts, chunk, mask words, pixels of the last chunk)
SCORE_BWD_CASES = {
    (2, 600, 104, 2, 32): (10, 60, 2, 60),
    (2, 641, 104, 2, 32): (11, 59, 2, 51),          # a ragged last chunk
    (64, 130, 35, 2, 32): (2, 65, 3, 65),           # bit 0 of the third word only
    (16, 1000, 104, 1, 64): (8, 125, 4, 125),       # the production geometry of stages 1 and 2
    (16, 1000, 5, 1, 64): (8, 125, 4, 125),         # the same with few keys: every mask word dense
    (64, 4300, 35, 2, 8): (32, 135, 5, 115),        # the 2048 / B workgroup cap
    (1, 200, 4200, 8, 8): (0, None, None, None),    # the masks do not fit in LDS: global-atomics fallback
}

# (B, N) -> (workgroups per sample, chunk)
OUT_BWD_CASES = {
    (2, 150): (5, 30),             # small grid: 32-pixel target
    (16, 2050): (9, 228),          # the 256-pixel branch
    (128, 2304): (8, 288),         # the 1024 / B workgroup cap
    (1, 1): (1, 1),
}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib.load()


def score_bwd_class(L, B, N, M, heads, d):
    """(parts, chunk, words, last) of crd_attn_scores_bwd at this shape, from the library's own rule."""
    parts = L.crd_attn_scores_bwd_partials(B, N, M, heads, d)
    if parts == 0:
        return 0, None, None, None
    chunk = cdiv(N, parts)
    return parts, chunk, cdiv(chunk, 32), N - (parts - 1) * chunk


def out_bwd_class(L, B, N, C):
    """(workgroups per sample, chunk) of crd_attn_out_bwd / crd_attn_out_bwd_gn at this shape."""
    blocks = L.crd_attn_out_bwd_blocks(B, N, C)
    return blocks, cdiv(N, blocks)


@pytest.mark.parametrize("shape", list(SCORE_BWD_CASES), ids=lambda s: "x".join(map(str, s)))
def test_score_backward_path_class(L, shape):
    assert score_bwd_class(L, *shape) == SCORE_BWD_CASES[shape]
    parts, chunk, _, last = SCORE_BWD_CASES[shape]
    if parts:
        assert 0 < last <= chunk and (parts - 1) * chunk + last == shape[1]


def test_score_backward_cases_cover_the_mask_word_counts():
    """One word (the existing op tests), and every count the training step runs (2 and 4) plus an odd one and one above."""
    assert {w for _, _, w, _ in SCORE_BWD_CASES.values()} == {2, 3, 4, 5, None}
    assert SCORE_BWD_CASES[(64, 4300, 35, 2, 8)][0] * 64 == 2048


@pytest.mark.parametrize("C", [8, 16, 64, 160, 320, 512])
@pytest.mark.parametrize("shape", list(OUT_BWD_CASES), ids=lambda s: "x".join(map(str, s)))
def test_output_backward_path_class(L, shape, C):
    assert out_bwd_class(L, *shape, C) == OUT_BWD_CASES[shape]          # (the channel count does not enter the rule)


def test_output_backward_classes():
    assert OUT_BWD_CASES[(2, 150)][1] <= 32 < OUT_BWD_CASES[(16, 2050)][1] <= 256
    assert OUT_BWD_CASES[(128, 2304)][0] * 128 == 1024 and OUT_BWD_CASES[(128, 2304)][1] > 256


def test_queries_refuse_empty_problems(L):
    assert L.crd_attn_out_bwd_blocks(0, 10, 64) == 0 and L.crd_attn_out_bwd_blocks(2, 0, 64) == 0
