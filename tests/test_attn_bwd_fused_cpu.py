"""CPU: the head of a Block's attention backward in the dry plan (no GPU: a plan is pure recording, as tests/test_plan_dry.py builds it).
With the stage's bit of plan_values.ATTN_BWD_FUSED set a Block records crd_attn_bwd_fused + crd_attn_dk_fold; without it the three
launches crd_attn_out_bwd_gn, crd_attn_bwd, crd_sum_partials_bf16.  One chain launch per Block is the whole difference."""
import os
import re

import pytest

from camradepth_amd import lib, plan_values
from camradepth_amd.engine import LATE, Plan
from camradepth_amd.model import CamRaDepth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = ("crd_attn_out_bwd_gn", "crd_attn_out_bwd", "crd_attn_bwd", "crd_sum_partials_bf16")
NEW = ("crd_attn_bwd_fused", "crd_attn_dk_fold")
QUERY = "crd_attn_bwd_fused_supported"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def _plan(mask, monkeypatch, depths=(1, 1, 1, 1)):
    monkeypatch.setattr(plan_values, "ATTN_BWD_FUSED", mask)
    m = CamRaDepth(input_channels=7, depths=depths)
    m.train(True)
    m._ensure_grad_views()
    return Plan(m, 2, 64, 96, True)


def _chain(p):
    return [op.name for op in p.bwd if p.live(op) and op.stream != LATE]


def _blocks(p):
    """The backward op names of every Block: the slices between two heads of the attention backward."""
    names = [op.name for op in p.bwd if p.live(op)]
    heads = [i for i, n in enumerate(names) if n in ("crd_attn_bwd_fused", "crd_attn_out_bwd_gn", "crd_attn_out_bwd")]
    return [names[a:b] for a, b in zip(heads, heads[1:] + [len(names)])]


@pytest.mark.parametrize("depths", [(1, 1, 1, 1), (2, 1, 2, 1)])
def test_fused_plan_replaces_the_three_launches(built, monkeypatch, depths):
    nblocks = sum(depths)
    on, off = _plan(15, monkeypatch, depths), _plan(0, monkeypatch, depths)
    blocks = _blocks(on)
    assert len(blocks) == nblocks
    for names in blocks:
        assert [names.count(n) for n in NEW] == [1, 1], names
        assert names.index("crd_attn_dk_fold") == names.index("crd_attn_bwd_fused") + 1        # right behind the launch that completes t
        assert not any(n in names for n in OLD), names
    blocks = _blocks(off)
    assert len(blocks) == nblocks
    for names in blocks:
        assert not any(n in names for n in NEW), names
        assert [names.count(n) for n in ("crd_attn_out_bwd_gn", "crd_attn_bwd", "crd_sum_partials_bf16")] == [1, 1, 1], names
    # one dependent launch less per Block, nothing else moved
    a, b = _chain(on), _chain(off)
    assert len(b) - len(a) == nblocks
    assert [n for n in a if n not in NEW] == [n for n in b if n not in OLD]
    assert [op.name for op in on.fwd] == [op.name for op in off.fwd]
    for p in (on, off):
        zero = sorted({op.name for op in p.fwd + p.bwd if p.live(op) and p.op_bytes(op) <= 0})
        assert not zero, f"launches without algorithmic bytes: {zero}"


def test_fused_ops_carry_the_bytes_of_the_launches_they_replace(built, monkeypatch):
    """The sum of what the replaced ops declared, minus the write and the read of dS (float [B][N])."""
    on, off = _plan(15, monkeypatch), _plan(0, monkeypatch)
    B = 2

    def by(p, names):
        return [sum(p.op_bytes(op) for op in blk) for blk in _split(p, names)]

    new, old = by(on, NEW), by(off, OLD)
    npix = [(64 // s) * (96 // s) for s in (32, 16, 8, 4)]          # the backward visits stage 4 first
    assert len(new) == len(old) == 4
    for n, o, px in zip(new, old, npix):
        assert o - n == 2 * B * px * 4, (n, o, px)


def _split(p, names):
    """Per Block (in backward order) the live ops whose name is in `names`."""
    out, cur = [], None
    for op in p.bwd:
        if not p.live(op):
            continue
        if op.name in ("crd_attn_bwd_fused", "crd_attn_out_bwd_gn", "crd_attn_out_bwd"):
            cur = []
            out.append(cur)
        if cur is not None and op.name in names:
            cur.append(op)
    return out


def test_mask_selects_stages(built, monkeypatch):
    for mask in (1, 4, 10):
        p = _plan(mask, monkeypatch)
        got = ["crd_attn_bwd_fused" in names for names in _blocks(p)]          # backward order: stage 4 first
        assert got == [bool((mask >> s) & 1) for s in (3, 2, 1, 0)], (mask, got)
    assert 0 <= plan_values.ATTN_BWD_FUSED <= 15


def test_header_and_binding_declare_both_entries():
    with open(os.path.join(REPO, "include", "camradepth_hip.h")) as f:
        hdr = f.read()
    for name in NEW + (QUERY,):
        assert re.search(r"^int %s\(" % name, hdr, re.M), f"{name} is not declared in include/camradepth_hip.h"
        assert name in lib._SIGS and name in lib.EXPORTS
    assert len(lib._SIGS["crd_attn_bwd_fused"]) == 26 and len(lib._SIGS["crd_attn_dk_fold"]) == 14          # arguments of the C declarations
    assert re.search(r"#define CRD_ABI_VERSION 13\b", hdr) and lib.ABI_VERSION == 13


def test_support_query_is_the_rule_of_the_plan_and_of_the_entry(built):
    """crd_attn_bwd_fused_supported: the score backward's workgroups per sample where the fused entry takes the shape, 0 where it refuses
    -- also in the last 4 KB of LDS, where the score backward's chunk still fits and the 2 * C channel sums of the output backward do not."""
    L = lib.load()
    for shape in [(2, 600, 104, 2, 32), (64, 130, 35, 2, 32), (2, 416, 104, 4, 40), (1, 1, 4, 1, 8), (2, 150, 104, 8, 64), (8, 6656, 104, 1, 64)]:
        assert L.crd_attn_bwd_fused_supported(*shape) == L.crd_attn_scores_bwd_partials(*shape) > 0, shape
    assert L.crd_attn_scores_bwd_partials(1, 200, 4200, 8, 8) == 0 and L.crd_attn_bwd_fused_supported(1, 200, 4200, 8, 8) == 0
    B, N, M, heads, d = gap = (1, 550, 1000, 8, 64)
    parts = L.crd_attn_scores_bwd_partials(*gap)
    chunk, C_ = -(-N // parts), heads * d
    need = chunk * C_ * 2 + chunk * 4 + heads * M * (-(-chunk // 32)) * 4 + 16          # LDS of a chunk of the score backward (attn_bwd_lds, attention.hip)
    assert parts == 9 and need <= 128 * 1024 < need + 2 * C_ * 4
    assert L.crd_attn_bwd_fused_supported(*gap) == 0
    assert L.crd_attn_bwd_fused_supported(1, 8, 4, 5, 104) == 0 and L.crd_attn_scores_bwd_partials(1, 8, 4, 5, 104) > 0      # C = 520
    for bad in [(0, 8, 4, 1, 8), (1, 0, 4, 1, 8), (1, 8, 0, 1, 8), (1, 8, 4, 0, 8), (1, 8, 4, 1, 12), (1, 8, 4, 1, 0)]:
        assert L.crd_attn_bwd_fused_supported(*bad) == 0, bad
