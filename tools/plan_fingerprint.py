#!/usr/bin/env python3
"""Canonical text of an execution plan (camradepth_amd.engine.Plan): everything a launch depends on, and no address.

A plan is pure recording, so it builds on a CPU in about a second; after Plan._finalise every op argument is an int, a float,
None or a ctypes.byref of a descriptor struct.  This tool prints, one line per item:

  * every op of plan.fwd and plan.bwd in order: name, stream, cond, region (id(...) members replaced by their order of first
    appearance), meta, Plan.op_bytes(op) and every argument.  Scalars as they are; a descriptor passed by reference expanded
    field by field from its _fields_; a raw pointer -- op argument or pointer-typed descriptor field -- as
    <shape dtype #k +byte offset>, where the buffer is found by address range among plan.buffers, the two zero arenas, the
    weight arena, the model's flat parameter / gradient buffers, x_in / seg_out / seg_grad_in / unsup_map, the cmap tensors and
    the pack / unpack / group tables, and #k is the order of the buffer's FIRST USE in this text (not its allocation order: a
    buffer no launch references may come or go without changing the text).  An integer >= 2^32 that lies in no known buffer
    is an error, not a scalar;
  * bwd_segments, fwd_marks, unpack_ranges, pack_offs, pack_elems, n_pack, n_unpack, max_unpack;
  * the pack and unpack tables, read back entry by entry, pointers canonicalised the same way;
  * each grouped weight-gradient launch: its WgradGroupInfo fields and meta (with the op) and the byte length of its device
    table.  The table's bytes are not compared (addresses, and padding the library leaves unset).  The per-problem WgradDesc
    structs ARE printed for plans built by this tool (build()): the plan does not keep them, so build() records what the
    plan hands to crd_wgrad_group_build, in call order = order of the grouped ops in fwd + bwd.

Usage:
    python tools/plan_fingerprint.py --out DIR [--only NAME ...]     one DIR/NAME.txt per configuration
    python tools/plan_fingerprint.py --compare DIR_A DIR_B           "NAME identical" / "NAME DIFFERENT" per configuration
    python tools/plan_fingerprint.py --list
"""
import argparse
import bisect
import contextlib
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from camradepth_amd import lib as L  # noqa: E402


class _Buffers:
    """Known allocations by address range; labels are handed out in order of first use."""

    def __init__(self, plan):
        m = plan.model
        ts = list(plan.buffers) + [plan.zf_arena, plan.zb_arena, plan.w_arena, m.flat, m.flat_grad, plan.x_in,
                                   getattr(plan, "seg_out", None), getattr(plan, "seg_grad_in", None), plan.unsup_map,
                                   plan.pack_table, plan.unpack_table]
        ts += [cw.cmap_dev for cw in plan.convs]
        spans = {}
        for t in ts:
            if t is None or t.numel() == 0:
                continue
            st = t.untyped_storage()
            spans.setdefault(st.data_ptr(), (st.data_ptr(), st.data_ptr() + st.nbytes(), t))
        self.spans = sorted(spans.values(), key=lambda s: s[0])
        self.starts = [s[0] for s in self.spans]
        for a, b in zip(self.spans, self.spans[1:]):
            assert a[1] <= b[0], "known buffers overlap"
        self.labels = {}

    def find(self, p):
        i = bisect.bisect_right(self.starts, p) - 1
        if i >= 0 and p < self.spans[i][1]:
            return self.spans[i]
        return None

    def canon(self, p, where):
        """Pointer (or None / scalar) -> text."""
        if p is None:
            return "null"
        if isinstance(p, float):
            return repr(p)
        p = int(p)
        span = self.find(p)
        if span is None:
            if p >= 1 << 32:
                raise ValueError(f"{where}: {p:#x} looks like a pointer but lies in no known buffer")
            return str(p)
        start, _, t = span
        if start not in self.labels:
            self.labels[start] = f"{tuple(t.shape)} {str(t.dtype).replace('torch.', '')} #{len(self.labels)}"
        return f"<{self.labels[start]} +{p - start}>"


def _struct(s, bufs, where):
    out = []
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if ctype is C.c_void_p:
            out.append(f"{name}={bufs.canon(v, where + '.' + name)}")
        elif isinstance(v, C.Array):
            out.append(f"{name}={list(v)}")
        else:
            out.append(f"{name}={v!r}")
    return type(s).__name__ + "{" + " ".join(out) + "}"


def _arg(a, bufs, where):
    if hasattr(a, "_obj"):                 # ctypes.byref(descriptor)
        return _struct(a._obj, bufs, where)
    if a is None or isinstance(a, (int, float)):
        return bufs.canon(a, where)
    raise ValueError(f"{where}: unresolved argument {type(a).__name__}")


def _region(region, ids):
    if region is None:
        return "None"
    out = []
    for r in region:
        if isinstance(r, int) and r >= 1 << 32:          # id(tensor) of the gradient buffer the region lives in
            out.append(f"id#{ids.setdefault(r, len(ids))}")
        else:
            out.append(repr(r))
    return "(" + ", ".join(out) + ")"


def fingerprint(plan):
    """The canonical text of a built plan (its current state: tests mutate a plan and compare)."""
    bufs, ids, lines = _Buffers(plan), {}, []
    groups = iter(getattr(plan, "group_descs", None) or [])
    for lname, ops in (("fwd", plan.fwd), ("bwd", plan.bwd)):
        for i, op in enumerate(ops):
            where = f"{lname}[{i}] {op.name}"
            meta = None if op.meta is None else sorted(op.meta.items())
            args = [_arg(a, bufs, f"{where} arg {j}") for j, a in enumerate(op.args)]
            lines.append(f"{where} stream={op.stream} cond={op.cond!r} live={plan.live(op)} region={_region(op.region, ids)} meta={meta!r} "
                         f"bytes={plan.op_bytes(op)} args=[{', '.join(args)}]")
            if op.name == "crd_conv_wgrad_grouped":
                table = bufs.find(int(op.args[0]))[2]
                lines.append(f"{where} table bytes={table.numel()}")
                for j, d in enumerate(next(groups, [])):
                    lines.append(f"{where} problem[{j}] " + _struct(d, bufs, f"{where} problem[{j}]"))
    for name in ("bwd_segments", "fwd_marks", "unpack_ranges", "pack_offs", "pack_elems", "n_pack", "n_unpack", "max_unpack"):
        v = getattr(plan, name)
        if isinstance(v, dict):
            v = sorted(v.items())
        lines.append(f"{name}={v!r}")
    for tname, table, n, cls in (("pack", plan.pack_table, plan.n_pack, L.PackEntry), ("unpack", plan.unpack_table, plan.n_unpack, L.UnpackEntry)):
        raw = bytes(table.cpu().numpy().tobytes())
        for i in range(n):
            e = cls.from_buffer_copy(raw, i * C.sizeof(cls))
            lines.append(f"{tname}[{i}] " + _struct(e, bufs, f"{tname}[{i}]"))
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ configurations
def _model(depths=None, train=True, frozen=(), attrs=None, **variant):
    from camradepth_amd.model import CamRaDepth
    m = CamRaDepth(input_channels=7, **({"depths": depths} if depths else {}), **variant)
    m.train(train)
    for n in frozen:
        m._param(n).requires_grad_(False)
    for k, v in (attrs or {}).items():
        m.__dict__[k] = v
    if train:
        m._ensure_grad_views()
    return m


@contextlib.contextmanager
def _capture_groups():
    """Records the WgradDesc arrays the plan hands to crd_wgrad_group_build (the fill calls, not the size queries)."""
    lib, got = L.load(), []
    orig = lib.crd_wgrad_group_build

    def spy(descs, n, host, capacity, info):
        if host is not None:
            got.append([L.WgradDesc.from_buffer_copy(descs[i]) for i in range(n)])
        return orig(descs, n, host, capacity, info)
    lib.crd_wgrad_group_build = spy
    try:
        yield got
    finally:
        lib.crd_wgrad_group_build = orig


def build(B, H, W, train=True, fp8_jit=None, **kw):
    """Plan of a fresh model (keywords: _model) with the per-problem descriptors of its grouped launches in plan.group_descs."""
    from camradepth_amd.engine import Plan
    with _capture_groups() as got:
        p = Plan(_model(train=train, **kw), B, H, W, train)
    p.group_descs = got
    if fp8_jit is not None:
        p.fp8_jit = fp8_jit
    return p


SMALL = dict(depths=(1, 1, 1, 1))
FROZEN = ("depth_upsample.2.conv.layers.1.model.0.weight", "dest_encoder.block2.0.norm1.weight")
FP8 = dict(fp8_scales={"depth_upsample.3": 0.01, "depth_upsample.4": 0.01}, fp8_train=True, fp8_grad=True)
CONFIGS = {
    "small_train_base": lambda: build(2, 64, 96, **SMALL),
    "small_train_seg": lambda: build(2, 64, 96, supervised_seg=True, **SMALL),
    "small_train_seg_unsup": lambda: build(2, 64, 96, supervised_seg=True, unsupervised_seg=True, **SMALL),
    "small_eval_base": lambda: build(2, 64, 96, train=False, **SMALL),
    "small_train_frozen2": lambda: build(2, 64, 96, frozen=FROZEN, **SMALL),
    "small_train_late160": lambda: build(2, 64, 96, attrs={"w3_total_wgs": 160}, **SMALL),
    "fp8_grad_jit": lambda: build(8, 128, 192, attrs=FP8, fp8_jit=True, **SMALL),
    "fp8_grad_delayed": lambda: build(8, 128, 192, attrs=FP8, fp8_jit=False, **SMALL),
    "fp8_inference_nograd": lambda: build(8, 128, 192, train=False, attrs={"fp8_scales": FP8["fp8_scales"], "_need_grad": False}, **SMALL),
    "full_train_base_b1": lambda: build(1, 256, 416),
    "full_train_base_b8": lambda: build(8, 256, 416),
    "full_train_seg_b1": lambda: build(1, 256, 416, supervised_seg=True),
    "full_eval_416x800": lambda: build(1, 416, 800, train=False),
    "full_inference_nograd": lambda: build(1, 256, 416, train=False, attrs={"_need_grad": False}),
    "full_train_late160_b8": lambda: build(8, 256, 416, attrs={"w3_total_wgs": 160}),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="directory that receives one text per configuration")
    ap.add_argument("--only", nargs="*", help="configurations to build (default: all)")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    if a.list:
        print("\n".join(CONFIGS))
        return 0
    if a.compare:
        bad = 0
        for name in CONFIGS:
            fa, fb = (os.path.join(d, name + ".txt") for d in a.compare)
            if not (os.path.exists(fa) and os.path.exists(fb)):
                print(f"{name} MISSING")
                bad += 1
                continue
            same = open(fa).read() == open(fb).read()
            print(f"{name} {'identical' if same else 'DIFFERENT'}")
            bad += not same
        return 1 if bad else 0
    if not a.out:
        ap.error("one of --out, --compare, --list")
    os.makedirs(a.out, exist_ok=True)
    for name in a.only or CONFIGS:
        text = fingerprint(CONFIGS[name]())
        with open(os.path.join(a.out, name + ".txt"), "w") as f:
            f.write(text)
        print(f"{name}: {text.count(chr(10))} lines", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
