// Gradient with respect to the model input x (CamRaDepth.forward's argument, src/models/CamRaDepth.py:99-176 under autograd).
// x reaches the loss along two edges:
//   * the stage-0 patch embed (dest_encoder.patch_embed1.proj: 7x7, stride 4, pad 3, Cin -> 64, simplified_attention.py:158,185),
//     whose data gradient is the stride-4 transposed convolution of d(raw) = `draw` (bf16, pixel-major [B][H/4 * W/4][64]) with the
//     forward-packed weight Wpe [64 co][49 taps][8 ci];
//   * the skip connection of the last decoder stage (depth_upsample.4, and seg_upsample.1 when it has a loss), whose write-once
//     K-concatenated data gradient already holds d(x) in the concat gradient's x columns [col0, col0 + Cin).
//
// Phase decomposition.  Input row iy = 4 m + ry takes taps ky = ry + 3 from draw row m and, when ry >= 1, ky = ry - 1 from row
// m + 1 (the same for columns).  So a 4 x 4 block of input pixels (m, t) reads exactly the four draw pixels (m | m+1, t | t+1): for
// a fixed row phase ry the block's 4 columns x 8 channels are ONE dense GEMM row of K = (doy, dox, co) <= 256 against a weight
// matrix A[M = (c, rx)][K] that depends on ry only (zero where a tap does not exist).  One wave per ry; its A operands (K 256 x
// M 32 = 16 fragments of v_mfma_f32_16x16x32_bf16) stay in registers, the pixel blocks stream through as B operands, 16 per tile:
// lane (l & 15) = pixel block, k = 8 (l >> 4) .. + 7 = a 16-byte piece of a draw row.  D lane l holds rows M = 4 (l >> 4) + i =
// channel (l >> 4) (+ 4), column rx = i: four consecutive input columns of one channel -- one float4 store into NCHW dx.
// The decoder's x columns are read as one 16-byte piece per pixel (all 8 columns); a lane keeps channels (l >> 4) and 4 + (l >> 4).
// Two groups of 4 waves share the workgroup's LDS copy of the weight and walk alternate tiles; the weight's 13 KB-per-group fill is
// issued as one batch of loads (a loop of dependent ones cost a memory latency per iteration).
// No atomics; every element of dx is written once; the sum order is fixed (MFMA, then the depth columns, then the seg columns).
#include "common.h"

namespace {

constexpr int IG_GROUPS = 2;                    // tile groups per workgroup
constexpr int IG_TPB = 256 * IG_GROUPS;         // a group = 4 waves: row phases 0..3 of the same 16 pixel blocks
constexpr int IG_TAPS = 49;
constexpr int IG_FILL = (IG_TAPS * 64 + IG_TPB - 1) / IG_TPB;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// channels c and c + 4 (c = 0..3) of a pixel's 8 x columns
__device__ __forceinline__ void x_cols(const bf16_t* p, int c, float& a, float& b) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(__builtin_assume_aligned(p, 16));
  const unsigned lo = (c & 2) ? v[1] : v[0], hi = (c & 2) ? v[3] : v[2];
  const int sh = (c & 1) * 16;
  a = __uint_as_float(((lo >> sh) & 0xffffu) << 16);
  b = __uint_as_float(((hi >> sh) & 0xffffu) << 16);
}

__global__ __launch_bounds__(IG_TPB) void k_input_grad(const bf16_t* __restrict__ draw, const bf16_t* __restrict__ wpe,
                                                       const bf16_t* __restrict__ dcb0, const bf16_t* __restrict__ dcb1, int ld, int col0,
                                                       int B, int H, int W, int Cin, float* __restrict__ dx, int ntiles) {
  __shared__ __attribute__((aligned(16))) bf16_t sW[IG_TAPS * 8 * 64];     // [tap][ci][co]: 8 consecutive co = one A fragment piece
  const int l = threadIdx.x & 63;
  const int ry = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 3);
  const int grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
  const int Hs = H >> 2, Ws = W >> 2;
  const long long P = (long long)B * Hs * Ws;                               // pixel blocks

  // ---- the weight, transposed through LDS (co on the lanes: conflict-free 2-byte writes) ----
  {
    u16x8 v[IG_FILL];
#pragma unroll
    for (int k = 0; k < IG_FILL; ++k) {
      const int i = threadIdx.x + k * IG_TPB, tap = i >> 6, co = i & 63;
      if (i < IG_TAPS * 64) v[k] = *reinterpret_cast<const u16x8*>(__builtin_assume_aligned(wpe + ((long long)co * IG_TAPS + tap) * 8, 16));
    }
#pragma unroll
    for (int k = 0; k < IG_FILL; ++k) {
      const int i = threadIdx.x + k * IG_TPB, tap = i >> 6, co = i & 63;
      if (i < IG_TAPS * 64) {
#pragma unroll
        for (int c = 0; c < 8; ++c) sW[(tap * 8 + c) * 64 + co] = v[k][c];
      }
    }
  }
  __syncthreads();

  // ---- this wave's A operands: row M = l & 15 -> (c = 4 mb + M / 4, rx = M % 4); k step s = (doy, dox, co half) ----
  const int kq = l >> 4, rxa = l & 3, cla = (l & 15) >> 2;
  const int nmb = Cin > 4 ? 2 : 1;
  const int ns = ry == 0 ? 4 : 8;                                           // ry = 0 has no tap in draw row m + 1
  bf16x8 wf[8][2];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int doy = s >> 2, dox = (s >> 1) & 1, half = s & 1;
    const int ky = ry + 3 - 4 * doy, kx = rxa + 3 - 4 * dox;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int c = 4 * mb + cla;
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (s < ns && ky >= 0 && kx >= 0 && c < Cin)
        v = *reinterpret_cast<const u16x8*>(&sW[((ky * 7 + kx) * 8 + c) * 64 + half * 32 + kq * 8]);
      wf[s][mb] = __builtin_bit_cast(bf16x8, v);
    }
  }

  for (int tile = blockIdx.x * IG_GROUPS + grp; tile < ntiles; tile += gridDim.x * IG_GROUPS) {
    const long long q = (long long)tile * 16 + (l & 15);                    // this lane's pixel block (B column / D column)
    const bool qv = q < P;
    const long long qq = qv ? q : 0;
    const int t = (int)(qq % Ws);
    const long long r = qq / Ws;
    const int m = (int)(r % Hs), b = (int)(r / Hs);
    const int iy = 4 * m + ry, ix0 = 4 * t;
    const long long pix = ((long long)b * H + iy) * W + ix0;               // first of the lane's 4 input pixels
    // the decoder's columns, requested ahead of the MFMAs: channels kq and kq + 4 of the 4 pixels
    float dec[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dec[0][i] = dec[1][i] = 0.f;
      if (qv) {
        const long long o = (pix + i) * ld + col0;
        x_cols(dcb0 + o, kq, dec[0][i], dec[1][i]);
        if (dcb1) {
          float a, b2;
          x_cols(dcb1 + o, kq, a, b2);
          dec[0][i] += a;
          dec[1][i] += b2;
        }
      }
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s >= ns) continue;                                                // (wave-uniform)
      const int doy = s >> 2, dox = (s >> 1) & 1, half = s & 1;
      const int oy = m + doy, ox = t + dox;
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (qv && oy < Hs && ox < Ws)
        v = *reinterpret_cast<const u16x8*>(__builtin_assume_aligned(draw + (((long long)b * Hs + oy) * Ws + ox) * 64 + half * 32 + kq * 8, 16));
      const bf16x8 bv = __builtin_bit_cast(bf16x8, v);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][0], bv, acc[0], 0, 0, 0);
      if (nmb > 1) acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][1], bv, acc[1], 0, 0, 0);
    }
    if (!qv) continue;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int c = 4 * mb + kq;
      if (mb >= nmb || c >= Cin) continue;
      f32x4 o = acc[mb];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] += dec[mb][i];
      *reinterpret_cast<f32x4*>(__builtin_assume_aligned(dx + (((long long)b * Cin + c) * H + iy) * W + ix0, 16)) = o;
    }
  }
}

}  // namespace

extern "C" int crd_input_grad(const void* draw, const void* wpe, const void* dcb_depth, const void* dcb_seg, int32_t dcb_ld, int32_t col0,
                              int32_t B, int32_t H, int32_t W, int32_t Cin, float* dx, crd_stream_t stream) {
  CRD_CHECK_ARG(draw && wpe && dcb_depth && dx, "crd_input_grad: null pointer");
  CRD_CHECK_ARG(((uintptr_t)draw & 15) == 0 && ((uintptr_t)wpe & 15) == 0 && ((uintptr_t)dx & 15) == 0,
                "crd_input_grad: draw, wpe and dx must be 16-byte aligned");
  CRD_CHECK_ARG(B > 0 && H > 0 && W > 0 && col0 >= 0 && dcb_ld > 0, "crd_input_grad: bad shape (B %d, H %d, W %d, col0 %d, ld %d)",
                B, H, W, col0, dcb_ld);
  CRD_UNSUPPORTED(Cin >= 1 && Cin <= 8, "crd_input_grad: Cin %d outside 1..8", Cin);
  CRD_UNSUPPORTED(H % 4 == 0 && W % 4 == 0, "crd_input_grad: H %d and W %d must be multiples of 4 (the stride of the patch embed)", H, W);
  CRD_CHECK_ARG(col0 % 8 == 0 && dcb_ld % 8 == 0 && col0 + 8 <= dcb_ld && ((uintptr_t)dcb_depth & 15) == 0 && ((uintptr_t)dcb_seg & 15) == 0,
                "crd_input_grad: the x columns [%d, %d) must be a 16-byte aligned piece of the %d-column rows", col0, col0 + 8, dcb_ld);
  CRD_UNSUPPORTED((long long)B * H * W * (dcb_ld > Cin ? dcb_ld : Cin) < (1ll << 40) && (long long)B * H * W / 16 < (1ll << 30),
                  "crd_input_grad: tensor too large");
  const long long P = (long long)B * (H / 4) * (W / 4);
  const int ntiles = (int)((P + 15) / 16);
  const int grid = cdiv(ntiles, IG_GROUPS) < 512 ? cdiv(ntiles, IG_GROUPS) : 512;   // 2 workgroups per CU (50 KB of LDS each)
  hipLaunchKernelGGL(k_input_grad, dim3(grid), dim3(IG_TPB), 0, as_stream(stream), (const bf16_t*)draw, (const bf16_t*)wpe,
                     (const bf16_t*)dcb_depth, (const bf16_t*)dcb_seg, (int)dcb_ld, (int)col0, (int)B, (int)H, (int)W, (int)Cin, dx, ntiles);
  CRD_LAUNCH_CHECK("crd_input_grad");
  return CRD_OK;
}
