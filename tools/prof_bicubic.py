#!/usr/bin/env python3
"""Microbenchmark of the bicubic x2 launches of the C2 plan (base, 8 x 256 x 416): crd_bicubic2x / crd_bicubic2x_fp8 and
crd_bicubic2x_bwd at every decoder level, with the plan's own leading dimensions and channel offsets.  One launch is timed as 50
launches per graph replay, the fastest and slowest of --repeats replays, with the algorithmic GB/s next to the 6.3 TB/s a streaming
kernel sustains on the chip.

    python tools/prof_bicubic.py                          the library in the tree (or CRD_LIB)
    python tools/prof_bicubic.py --ab PARENT.so BRANCH.so  both libraries back to back, each in a process of its own; a launch
                                                          whose fastest branch time is above the parent's slowest is marked SLOWER
"""
import argparse
import collections
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
HBM_GBS = 6300.0
B = 8
Spec = collections.namedtuple("Spec", "entry H W C x_ld x_coff y_ld y_coff f8_ld f8_coff keep acc", defaults=(0, 0, 0, 0))


def nbytes(s):
    """Algorithmic bytes of a launch: every tensor read or written once."""
    n = B * s.H * s.W * s.C
    if s.entry == "crd_bicubic2x":
        return n * 2 * 5
    if s.entry == "crd_bicubic2x_fp8":
        return n * 2 + 4 * n + (8 * n if s.keep else 0)
    return n * 2 * (5 + (1 if s.acc else 0))


def label(s):
    form = {"crd_bicubic2x": "y bf16", "crd_bicubic2x_fp8": "y e4m3" + (" + bf16" if s.keep else ""),
            "crd_bicubic2x_bwd": "dx +=" if s.acc else "dx ="}[s.entry]
    return f"{s.entry[4:]:14s} {B}x{s.H}x{s.W}x{s.C} ld {s.x_ld}+{s.x_coff} -> {s.y_ld}+{s.y_coff} {form}"


def shapes_plan():
    """Every distinct bicubic launch of the C2 plan, with how often the step launches it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("plan_fingerprint_prof", os.path.join(HERE, "plan_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    plan = fp.build(B, 256, 416)
    count = collections.Counter()
    for op in list(plan.fwd) + list(plan.bwd):
        a = op.args
        if op.name == "crd_bicubic2x":
            count[Spec(op.name, a[4], a[5], a[6], a[1], a[2], a[8], a[9])] += 1
        elif op.name == "crd_bicubic2x_fp8":
            count[Spec(op.name, a[4], a[5], a[6], a[1], a[2], a[12], a[13], a[8], a[9], int(a[11] is not None))] += 1
        elif op.name == "crd_bicubic2x_bwd":
            count[Spec(op.name, a[4], a[5], a[6], a[1], a[2], a[8], a[9], acc=int(bool(a[10])))] += 1
    del plan
    return sorted(count.items())


def measure(repeats):
    import torch
    import camradepth_amd.lib as L
    lb = L.load()

    def timed(fn, n=50):
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

    rows = []
    for s, n in shapes_plan():
        small = torch.randn(B, s.H * s.W, s.x_ld, device="cuda").to(torch.bfloat16)            # the input-sized map: x, or dx
        st = L.stream
        if s.entry == "crd_bicubic2x_bwd":
            big = torch.randn(B, 4 * s.H * s.W, s.x_ld, device="cuda").to(torch.bfloat16)       # dy (x_ld / x_coff are dy's)
            small = torch.zeros(B, s.H * s.W, s.y_ld, dtype=torch.bfloat16, device="cuda")
            keep = [big, small]
            fn = lambda: lb.crd_bicubic2x_bwd(big.data_ptr(), s.x_ld, s.x_coff, B, s.H, s.W, s.C, small.data_ptr(), s.y_ld, s.y_coff, s.acc, st())
        elif s.entry == "crd_bicubic2x":
            big = torch.zeros(B, 4 * s.H * s.W, s.y_ld, dtype=torch.bfloat16, device="cuda")
            keep = [big, small]
            fn = lambda: lb.crd_bicubic2x(small.data_ptr(), s.x_ld, s.x_coff, B, s.H, s.W, s.C, big.data_ptr(), s.y_ld, s.y_coff, st())
        else:
            big8 = torch.zeros(B, 4 * s.H * s.W, s.f8_ld, dtype=torch.uint8, device="cuda")
            big = torch.zeros(B, 4 * s.H * s.W, s.y_ld, dtype=torch.bfloat16, device="cuda") if s.keep else None
            keep = [big, big8, small]
            fn = lambda: lb.crd_bicubic2x_fp8(small.data_ptr(), s.x_ld, s.x_coff, B, s.H, s.W, s.C, big8.data_ptr(), s.f8_ld, s.f8_coff, 0.01,
                                              big.data_ptr() if s.keep else None, s.y_ld, s.y_coff, st())
        lo, hi = timed(fn)
        rows.append(dict(label=label(s), n=n, lo=lo, hi=hi, gb=nbytes(s) / 1e9))
        del fn, keep
    return rows


def table(rows, against=None):
    lines = [f"{'launch':78s} {'n':>3s} {'us (min .. max)':>18s} {'GB/s':>7s} {'of 6.3 TB/s':>11s}"]
    for i, r in enumerate(rows):
        mark = "   SLOWER than the parent" if against and r["lo"] > against[i]["hi"] else ""
        lines.append(f"{r['label']:78s} {r['n']:3d} {r['lo']:8.2f} .. {r['hi']:7.2f} {r['gb'] / (r['lo'] * 1e-6):7.0f} "
                     f"{100 * r['gb'] / (r['lo'] * 1e-6) / HBM_GBS:10.0f}%{mark}")
    for name in ("crd_bicubic2x", "crd_bicubic2x_bwd"):
        sel = [r for r in rows if r["label"].startswith(name[4:] + " ") or (name == "crd_bicubic2x" and r["label"].startswith("bicubic2x_fp8"))]
        if sel:
            lo, hi, gb = (sum(r["n"] * r[k] for r in sel) for k in ("lo", "hi", "gb"))
            lines.append(f"sum {name:18s} {sum(r['n'] for r in sel):3d} launches {gb:6.3f} GB  {lo / 1e3:7.4f} .. {hi / 1e3:7.4f} ms  "
                         f"{gb / (lo * 1e-6):6.0f} GB/s   floor at 6.3 TB/s {gb / HBM_GBS * 1e3:6.4f} ms")
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", action="store_true", help="print the rows as one JSON line (the form --ab reads)")
    ap.add_argument("--ab", nargs=2, metavar=("PARENT_LIB", "BRANCH_LIB"))
    ap.add_argument("--out", help="with --ab: also write the report to this file")
    args = ap.parse_args()
    if args.ab:
        got = []
        for path in args.ab:                         # a process per library: the library is chosen when camradepth_amd.lib is imported
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--json", "--repeats", str(args.repeats)],
                               env=dict(os.environ, CRD_LIB=os.path.abspath(path)), capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"{path}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            got.append(json.loads(r.stdout.strip().splitlines()[-1]))
        assert [r["label"] for r in got[0]] == [r["label"] for r in got[1]]
        slower = sum(b["lo"] > a["hi"] for a, b in zip(*got))
        text = "\n\n".join([f"parent ({args.ab[0]})\n" + table(got[0]), f"branch ({args.ab[1]})\n" + table(got[1], got[0]),
                            f"{slower} of {len(got[0])} launches marked slower (fastest branch time above the parent's slowest)"])
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
    else:
        rows = measure(args.repeats)
        print(json.dumps(rows) if args.json else table(rows))
