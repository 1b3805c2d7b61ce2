"""CPU: tools/plan_fingerprint.py -- the canonical text of an execution plan that a refactor of the plan engine is compared by.
It must not depend on addresses (two builds of one configuration give the same text) and must depend on everything a launch
depends on: one scalar argument, one descriptor stride, one pointer offset, the order of two ops."""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "plan_fingerprint", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "plan_fingerprint.py"))
fp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fp)


def _build():
    return fp.build(2, 64, 96, depths=(1, 1, 1, 1))


@pytest.fixture(scope="module")
def base():
    plan = _build()
    return plan, fp.fingerprint(plan)


def _first(plan, pred):
    for op in plan.fwd:
        for j, a in enumerate(op.args):
            if pred(op, a):
                return op, j
    raise AssertionError("no such argument in the forward list")


def test_two_builds_give_the_same_text(base):
    assert fp.fingerprint(_build()) == base[1]
    assert base[1].count("\n") > 400 and " problem[0] WgradDesc{" in base[1]


def test_text_sees_one_scalar_argument(base):
    plan, text = base
    op, j = _first(plan, lambda op, a: op.name == "crd_gn_stats" and isinstance(a, int) and 0 < a < 1 << 16)
    op.args[j] += 1
    try:
        assert fp.fingerprint(plan) != text
    finally:
        op.args[j] -= 1
    assert fp.fingerprint(plan) == text


def test_text_sees_one_descriptor_stride(base):
    plan, text = base
    op, j = _first(plan, lambda op, a: op.name == "crd_conv_igemm" and hasattr(a, "_obj"))
    op.args[j]._obj.x_ld += 8
    try:
        assert fp.fingerprint(plan) != text
    finally:
        op.args[j]._obj.x_ld -= 8


def test_text_sees_one_pointer_offset(base):
    plan, text = base
    op, j = _first(plan, lambda op, a: op.name == "crd_gn_stats" and isinstance(a, int) and a >= 1 << 32)
    op.args[j] += 2
    try:
        assert fp.fingerprint(plan) != text
    finally:
        op.args[j] -= 2
    d = _first(plan, lambda op, a: op.name == "crd_conv_igemm" and hasattr(a, "_obj"))[0].args[0]._obj
    d.y += 16
    try:
        assert fp.fingerprint(plan) != text
    finally:
        d.y -= 16


def test_text_sees_two_ops_swapped(base):
    plan, text = base
    i = next(i for i in range(len(plan.bwd) - 1) if plan.bwd[i].name != plan.bwd[i + 1].name)
    plan.bwd[i], plan.bwd[i + 1] = plan.bwd[i + 1], plan.bwd[i]
    try:
        assert fp.fingerprint(plan) != text
    finally:
        plan.bwd[i], plan.bwd[i + 1] = plan.bwd[i + 1], plan.bwd[i]
    assert fp.fingerprint(plan) == text


def test_pointer_outside_every_known_buffer_is_an_error(base):
    plan, _ = base
    op, j = _first(plan, lambda op, a: op.name == "crd_gn_stats" and isinstance(a, int) and a >= 1 << 32)
    keep, op.args[j] = op.args[j], (1 << 62) + 8
    try:
        with pytest.raises(ValueError, match="no known buffer"):
            fp.fingerprint(plan)
    finally:
        op.args[j] = keep
