"""Times crd_input_grad (x.grad: the stage-0 patch embed's stride-4 transposed convolution + the last decoder stage's x columns)
at 8 x 256 x 416 and 2 x 416 x 800 (Cin 7, depth + seg columns), with its algorithmic bytes, FLOPs and floors, and -- as a
comparison point, in the same process -- the patch-embed half as the generic strided data-gradient gather of crd_conv_igemm
(K = 49 x 64 per pixel, 8 of a tile's columns used).  Run under `rocprofv3 --kernel-trace --stats` for per-kernel device times.

    python tools/bench_input_grad.py [--reps 50]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from camradepth_amd import lib  # noqa: E402

HBM_TBS, FP32_TFLOPS = 6.3, 157.0


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    L = lib.load()
    st = lib.stream()
    for (B, H, W) in ((8, 256, 416), (2, 416, 800)):
        Cin, ld, col0 = 7, 304, 136
        Hs, Ws = H // 4, W // 4
        g = torch.Generator(device="cuda").manual_seed(0)
        draw = torch.randn(B, Hs * Ws, 64, device="cuda", generator=g).to(torch.bfloat16)
        wpe = (torch.randn(64, 49, 8, device="cuda", generator=g) / 20).to(torch.bfloat16)
        dcb = torch.randn(B, H * W, ld, device="cuda", generator=g).to(torch.bfloat16)
        dcb_s = torch.randn(B, H * W, ld, device="cuda", generator=g).to(torch.bfloat16)
        dx = torch.empty(B, Cin, H, W, device="cuda")
        for seg in (False, True):
            def run():
                lib.check(L.crd_input_grad(draw.data_ptr(), wpe.data_ptr(), dcb.data_ptr(), dcb_s.data_ptr() if seg else None, ld, col0,
                                           B, H, W, Cin, dx.data_ptr(), st), "crd_input_grad")
            us = timed(run, a.reps)
            nsrc = 2 if seg else 1
            alg = draw.numel() * 2 + B * H * W * Cin * 2 * nsrc + dx.numel() * 4 + wpe.numel() * 2
            fetched = draw.numel() * 2 + B * H * W * 64 * nsrc + dx.numel() * 4      # x columns: one 64-byte sector per pixel and source
            flops = 2.0 * B * Cin * 64 * (7 * Hs - 3) * (7 * Ws - 3)
            byte_us, fetched_us, flop_us = alg / HBM_TBS / 1e6, fetched / HBM_TBS / 1e6, flops / FP32_TFLOPS / 1e6
            print(f"crd_input_grad B{B} {H}x{W} Cin{Cin} seg{int(seg)}: {us:7.1f} us | algorithmic {alg / 1e6:6.1f} MB "
                  f"({byte_us:5.1f} us), sectors {fetched / 1e6:6.1f} MB ({fetched_us:5.1f} us), {flops / 1e9:5.2f} GFLOP "
                  f"({flop_us:5.1f} us at the FP32 vector peak) | {us / max(byte_us, flop_us):4.2f}x the larger floor", flush=True)
        # comparison: the patch-embed half alone as the generic strided data-gradient gather (k_igemm, 64-column tiles)
        wd = torch.zeros(64, 49, 64, dtype=torch.bfloat16, device="cuda")           # [ci][tap][co] (crd_pack_entry.dst_dgrad), a whole tile of rows
        wd[:Cin] = wpe[:, :, :Cin].permute(2, 1, 0)
        y = torch.empty(B, H * W, 64, dtype=torch.bfloat16, device="cuda")          # row stride 64: the tile's columns stay in the row
        d = lib.ConvDesc()
        d.x, d.x_ld, d.x_coff, d.B, d.IH, d.IW, d.Cin = draw.data_ptr(), 64, 0, B, Hs, Ws, 64
        d.w, d.Cout, d.KH, d.KW, d.stride, d.pad, d.OH, d.OW = wd.data_ptr(), 8, 7, 7, 4, 3, H, W
        d.gather_mode, d.y, d.y_ld, d.y_coff, d.y_f32 = 1, y.data_ptr(), 64, 0, 0
        us = timed(lambda: lib.check(L.crd_conv_igemm(lib.C.byref(d), st),
                                     "crd_conv_igemm"), a.reps)
        print(f"  comparison: crd_conv_igemm strided gather, patch-embed half only (bf16 pixel-major out): {us:7.1f} us", flush=True)


if __name__ == "__main__":
    main()
