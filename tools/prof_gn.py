#!/usr/bin/env python3
"""Microbenchmark of the three streaming GroupNorm passes (crd_gn_apply, crd_gn_bwd_reduce, crd_gn_bwd_apply), B = 8: the time of one
launch (50 launches per graph replay, the fastest and slowest of --repeats replays) and the algorithmic GB/s next to the 6.3 TB/s
a streaming kernel sustains on the chip.

    python tools/prof_gn.py             encoder and decoder shapes, every form the training step uses
    python tools/prof_gn.py --plan      every distinct launch of the C2 plan (base, 8 x 256 x 416) with its launch count, and the
                                        summed time of all of them (shape time x count)
"""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import camradepth_amd.lib as L
from tests.util import to_stat, zsum

HBM_GBS = 6300.0
lb = L.load()
P = lambda t: t.data_ptr() if t is not None else None
B = 8


def timed(fn, n=50, repeats=3):
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    out = []
    with torch.cuda.stream(s):
        fn(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(n):
                fn()
        g.replay()
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / n * 1e3)
    return min(out), max(out)


# One launch: entry, pixels, channels, gmul, act, x fp32, mask, and what the entry writes:
#   apply:  out_f32;  bwd_apply:  out_f32 (dx), acc, dx2, pgrad (parameter gradients), inplace (dx is dy)
Spec = collections.namedtuple("Spec", "entry Pn C gmul act xf32 mask out_f32 acc dx2 pgrad inplace", defaults=(0, 0, 0, 0, 0, 0))


def esize(f32):
    return 4 if f32 else 2


def nbytes(s):
    """Algorithmic bytes of a launch: every tensor read or written once."""
    n = B * s.Pn * s.C
    if s.entry == "crd_gn_apply":
        return n * (esize(s.xf32) + esize(s.out_f32))
    if s.entry == "crd_gn_bwd_reduce":
        return n * (esize(s.xf32) + 2)
    return n * (esize(s.xf32) + 2 + esize(s.out_f32) * (2 if s.acc else 1) + (2 if s.dx2 else 0))


def launcher(s):
    Pn, C, gmul = s.Pn, s.C, s.gmul
    x = torch.randn(B, Pn, C, device="cuda") if s.xf32 else torch.randn(B, Pn, C, device="cuda").to(torch.bfloat16)
    dy = torch.randn(B, Pn, C, device="cuda").to(torch.bfloat16)
    G = C // (16 * gmul)
    stats = to_stat(torch.stack([torch.zeros(B, C // 16), torch.ones(B, C // 16) * Pn * 16], -1)).cuda()
    gam, bet = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    mask = torch.ones(B, C, device="cuda") if s.mask else None
    r = zsum(B * C * 2 + B * G * 2)
    out = torch.zeros(B, Pn, C, dtype=torch.float32 if s.out_f32 else torch.bfloat16, device="cuda")
    st = L.stream
    keep = [x, dy, stats, gam, bet, mask, r, out]
    if s.entry == "crd_gn_apply":
        fn = lambda: lb.crd_gn_apply(P(x), s.xf32, C, 0, B, Pn, C, P(stats), gmul, P(gam), P(bet), s.act, P(mask), P(out), s.out_f32, C, 0, st())
    elif s.entry == "crd_gn_bwd_reduce":
        fn = lambda: lb.crd_gn_bwd_reduce(P(x), s.xf32, C, 0, P(dy), 0, C, 0, B, Pn, C, P(stats), gmul, P(gam), P(bet), s.act, P(mask), P(r), None, 0, st())
    else:
        dgam, dbet = (torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")) if s.pgrad else (None, None)
        dx = dy if s.inplace else out
        dx2 = torch.zeros(B, Pn, C, dtype=torch.bfloat16, device="cuda") if s.dx2 else None
        keep += [dgam, dbet, dx2]
        fn = lambda: lb.crd_gn_bwd_apply(P(x), s.xf32, C, 0, P(dy), 0, C, 0, B, Pn, C, P(stats), gmul, P(gam), P(bet), s.act, P(mask), P(r),
                                         P(dgam), P(dbet), P(dx), s.out_f32, C, 0, s.acc, P(dx2), C if s.dx2 else 0, None, st())
    return fn, keep


def label(s):
    form = []
    if s.entry == "crd_gn_bwd_apply":
        form = ["dx fp32" if s.out_f32 else "dx bf16"] + (["+="] if s.acc else []) + (["dx2"] if s.dx2 else []) + \
               (["dgamma,dbeta"] if s.pgrad else []) + (["in place"] if s.inplace else [])
    elif s.entry == "crd_gn_apply":
        form = ["y fp32" if s.out_f32 else "y bf16"]
    return f"{s.entry[4:]:13s} {B}x{s.Pn}x{s.C} gmul {s.gmul} {'gelu' if s.act else 'lin '} x {'fp32' if s.xf32 else 'bf16'}" \
           f"{' mask' if s.mask else ''} {' '.join(form)}"


def shapes_table():
    out = []
    for (Pn, C, gmul, act, xf32) in [(104, 512, 1, 0, 1), (104, 2048, 4, 1, 0), (416, 320, 1, 0, 1), (416, 1280, 4, 1, 0), (416, 1280, 1, 0, 0),
                                     (1664, 1024, 8, 1, 0), (6656, 512, 8, 1, 0), (6656, 64, 1, 0, 1),
                                     # decoder ConvLayers (GELU) at 256 x 416, 128 x 208, 64 x 104
                                     (106496, 128, 1, 1, 0), (26624, 128, 1, 1, 0), (6656, 128, 1, 1, 0)]:
        out.append(Spec("crd_gn_apply", Pn, C, gmul, act, xf32))
        out.append(Spec("crd_gn_bwd_reduce", Pn, C, gmul, act, xf32))
        out.append(Spec("crd_gn_bwd_apply", Pn, C, gmul, act, xf32, pgrad=1))
        out.append(Spec("crd_gn_bwd_apply", Pn, C, gmul, act, xf32))
        if xf32:        # Block.norm: the gradient is added to the fp32 residual gradient
            out.append(Spec("crd_gn_bwd_apply", Pn, C, gmul, act, xf32, out_f32=1, acc=1, pgrad=1))
        else:           # the dx-accumulate form
            out.append(Spec("crd_gn_bwd_apply", Pn, C, gmul, act, xf32, acc=1, pgrad=1))
    return [(s, 1) for s in out]


def shapes_plan():
    """Every distinct launch of the three entries in the C2 plan, with how often the step launches it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("plan_fingerprint_prof", os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    plan = fp.build(B, 256, 416)
    count = collections.Counter()
    for op in list(plan.fwd) + list(plan.bwd):
        a = op.args
        if op.name == "crd_gn_apply":
            count[Spec(op.name, a[5], a[6], a[8], a[11], a[1], int(a[12] is not None), out_f32=a[14])] += 1
        elif op.name == "crd_gn_bwd_reduce":
            count[Spec(op.name, a[9], a[10], a[12], a[15], a[1], int(a[16] is not None))] += 1
        elif op.name == "crd_gn_bwd_apply":
            count[Spec(op.name, a[9], a[10], a[12], a[15], a[1], int(a[16] is not None), out_f32=a[21], acc=int(bool(a[24])),
                       dx2=int(a[25] is not None), pgrad=int(a[18] is not None), inplace=int(a[20] == a[4]))] += 1
    del plan
    return sorted(count.items())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    rows = shapes_plan() if args.plan else shapes_table()
    total = collections.defaultdict(lambda: [0.0, 0.0, 0.0, 0])
    print(f"{'launch':92s} {'n':>3s} {'us (min .. max)':>18s} {'GB/s':>7s} {'of 6.3 TB/s':>11s}")
    for s, n in rows:
        fn, keep = launcher(s)
        lo, hi = timed(fn, repeats=args.repeats)
        gb = nbytes(s) / 1e9
        print(f"{label(s):92s} {n:3d} {lo:8.2f} .. {hi:7.2f} {gb / (lo * 1e-6):7.0f} {100 * gb / (lo * 1e-6) / HBM_GBS:10.0f}%", flush=True)
        t = total[s.entry]
        t[0] += n * lo; t[1] += n * hi; t[2] += n * gb; t[3] += n
        del fn, keep
    if args.plan:
        for entry, (lo, hi, gb, n) in sorted(total.items()):
            print(f"sum {entry:18s} {n:3d} launches {gb:6.2f} GB  {lo / 1e3:7.3f} .. {hi / 1e3:7.3f} ms  {gb / (lo * 1e-6):6.0f} GB/s   floor at 6.3 TB/s {gb / HBM_GBS * 1e3:6.3f} ms")
        lo, hi, gb, n = [sum(t[i] for t in total.values()) for i in range(4)]
        print(f"sum {'all three':18s} {n:3d} launches {gb:6.2f} GB  {lo / 1e3:7.3f} .. {hi / 1e3:7.3f} ms  {gb / (lo * 1e-6):6.0f} GB/s   floor at 6.3 TB/s {gb / HBM_GBS * 1e3:6.3f} ms")
