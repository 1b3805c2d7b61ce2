// Encoder-side kernels for gfx950: the depthwise 3x3 convolution of the Simplified Transformer's Mlp, its data gradient (FLIP) and its
// weight gradient.  (The max-pool attention of the same Blocks: attention.hip.)
#include <stdlib.h>
#include "common.h"

namespace {

constexpr int TPB = 256;

// ------------------------------------------------------------------------------------------------
// Depthwise 3x3, stride 1, pad 1, pixel-major bf16 [B][H][W][C] (ld = C).
// A workgroup owns an 8 x TW pixel tile of a 64-channel window.  The (8+2) x (TW+2) halo of the window is loaded ONCE
// into LDS with coalesced 16-byte loads, all in flight together (the register sliding-window kernel this replaces read
// every input three times with ~190 VGPRs and one dependent load batch at a time: 1.5 TB/s); thread (column x, granule g)
// then walks down the tile's rows keeping the 3x3 neighbourhood of its 8 channels in registers: three ds_read_b128 per
// output, lanes g-fastest so a wave reads 1 KB contiguous.  Weights stay in registers; GroupNorm statistics are folded
// with shuffles + LDS and leave the workgroup as one atomic per slab and moment.
// TW = 32 (256 threads = 32 columns x 8 granules) or 16 (two row halves) for narrow images.
// ------------------------------------------------------------------------------------------------
constexpr int DTH = 8;    // tile rows
constexpr int DCW = 64;   // channel window (8 granules: 128-byte pixel rows in LDS)

// Optional GroupNorm of the INPUT applied while the halo is staged (Mlp.norm1 between fc1 and the depthwise conv,
// simplified_attention.py:37-38): xn = bf16((x - mean) * rstd * gamma + beta), exactly what crd_gn_apply would have
// written, so the normalised hidden tensor is never materialised.  A thread stages the same granule for every piece.
struct InNorm {
  const crd_sum_t* stats;   // g16 sums of x [B][C/16][2], or nullptr: no normalisation
  const float* gamma; const float* beta; int gmul;
};
__device__ __forceinline__ void innorm_coeffs(const InNorm& n, int b, int C, long long P, int c0, bool ok, float (&a)[8], float (&s)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) { a[j] = 1.f; s[j] = 0.f; }
  if (n.stats == nullptr || !ok) return;
  float mean, rstd;
  const int grp = (c0 >> 4) / n.gmul;
  gn_mean_rstd(n.stats + (long long)b * (C >> 4) * 2, grp * n.gmul, n.gmul, (float)P * 16.f * n.gmul, mean, rstd);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = n.gamma[c0 + j] * rstd;
    s[j] = n.beta[c0 + j] - mean * a[j];
  }
}
__device__ __forceinline__ uint4 innorm_apply(const uint4& u, const float (&a)[8], const float (&s)[8]) {
  uint4 r;
  r.x = pack_bf2(bf_lo(u.x) * a[0] + s[0], bf_hi(u.x) * a[1] + s[1]);
  r.y = pack_bf2(bf_lo(u.y) * a[2] + s[2], bf_hi(u.y) * a[3] + s[3]);
  r.z = pack_bf2(bf_lo(u.z) * a[4] + s[4], bf_hi(u.z) * a[5] + s[5]);
  r.w = pack_bf2(bf_lo(u.w) * a[6] + s[6], bf_hi(u.w) * a[7] + s[7]);
  return r;
}

// Optional first phase of the backward of a GroupNorm (gmul = 1, no activation) that FOLLOWS in the backward chain,
// fused into the producer of its dy: with y = this kernel's (rounded) output as dy and xr the GroupNorm's raw input,
// r[b][c] += (sum y, sum y*xhat) and rg[b][c/16] += sum_c gamma_c * r (crd_gn_bwd_reduce's outputs), so that only
// crd_gn_bwd_apply remains.  Mlp.norm1's backward receives d(H1N) from the depthwise data gradient: this saves one pass
// over (H1, d(H1N)) per block.
struct RedOut {
  const bf16_t* xr;       // raw input of the GroupNorm [B][H][W][C], or nullptr: no reduce
  const crd_sum_t* stats; // its g16 sums
  const float* gamma;
  crd_sum_t* r;           // [B][C][2] then [B][C/16][2]
};

template <bool FLIP, bool STATS, int TW>
__global__ __launch_bounds__(TPB) void k_dwconv(const bf16_t* x, int H, int W, int C, const float* w9, const float* bias,
                                                bf16_t* y, crd_sum_t* stats, int tiles_x, InNorm inn, RedOut red) {
  constexpr int HWD = TW + 2;                       // halo width
  constexpr int HPX = (DTH + 2) * HWD;              // halo pixels
  constexpr int RSPLIT = 32 / TW;                   // row groups of the thread mapping (TW = 16: rows 0-3 / 4-7)
  constexpr int ROWS = DTH / RSPLIT;                // rows a thread walks
  __shared__ __attribute__((aligned(16))) uint4 sh[HPX * 8];
  __shared__ float sred[4][16];
  const int b = blockIdx.z;
  const int c_win = blockIdx.y * DCW;
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int ty0 = tyi * DTH, tx0 = txi * TW;
  const bf16_t* xb = x + (long long)b * H * W * C;
  bf16_t* yb = y + (long long)b * H * W * C;
  const int t = threadIdx.x;
  const int nG = (C - c_win) >= DCW ? 8 : (C - c_win) >> 3;     // granules of this window that exist
  const int g = t & 7, xc = (t >> 3) % TW, rg = (t >> 3) / TW;
  const int c0 = c_win + g * 8;
  const bool gok = g < nG;
  // taps, bias, window and accumulators as PAIRS of channels: the kernel is bound by its vector instruction count (3200 per thread
  // for 64 outputs; the launch at stage 1 takes 41 us where its 109 MB need 20), and v_pk_fma_f32 multiplies two channels at once
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  f32x2 wv[9][4], bv[4];
  // ---- halo -> LDS: piece i = (halo pixel i >> 3, granule i & 7)
  {
    uint4 r[(HPX * 8 + TPB - 1) / TPB];
    bool inimg[(HPX * 8 + TPB - 1) / TPB];
#pragma unroll
    for (int k = 0; k < (HPX * 8 + TPB - 1) / TPB; ++k) {
      const int i = t + k * TPB;
      const int hp = i >> 3, g = i & 7;
      const int hy = hp / HWD, hx = hp - hy * HWD;
      const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
      inimg[k] = i < HPX * 8 && g < nG && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      // unconditional loads from a clamped address, zeroed by a select: under `if (inimg) load` the compiler put a
      // s_waitcnt vmcnt(0) right behind the FIRST piece's load (one memory latency before the other ten were requested)
      const int cy = iy < 0 ? 0 : (iy < H ? iy : H - 1), cx = ix < 0 ? 0 : (ix < W ? ix : W - 1), cgr = g < nG ? g : 0;
      const uint4 u = *reinterpret_cast<const uint4*>(xb + ((long long)cy * W + cx) * C + c_win + cgr * 8);
      r[k] = inimg[k] ? u : make_uint4(0, 0, 0, 0);
    }
    // weights, bias and the input-norm coefficients are requested while the halo is in flight (after the LDS stores they
    // were a second dependent round trip on the small grids)
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) {
      float w8[8];
      if (gok) load8t<1>(w9, (long long)(FLIP ? 8 - tp : tp) * C + c0, w8);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) w8[j] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) wv[tp][q] = f32x2{w8[2 * q], w8[2 * q + 1]};
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[q] = f32x2{(bias && gok) ? bias[c0 + 2 * q] : 0.f, (bias && gok) ? bias[c0 + 2 * q + 1] : 0.f};
    float na[8], ns[8];
    innorm_coeffs(inn, b, C, (long long)H * W, c_win + (t & 7) * 8, (t & 7) < nG, na, ns);
#pragma unroll
    for (int k = 0; k < (HPX * 8 + TPB - 1) / TPB; ++k) {
      const int i = t + k * TPB;
      if (i < HPX * 8) sh[i] = (inn.stats && inimg[k]) ? innorm_apply(r[k], na, ns) : r[k];   // the zero padding stays zero
    }
  }
  // the fused reduce reads the GroupNorm's raw input at every output position: all ROWS requests NOW (clamped addresses, like the
  // halo).  Inside the row loop each one was a load followed by its own wait -- eight memory latencies per thread: the data gradient
  // with the reduce took 50.5 us at stage 1 against 32.5 without
  uint4 xrv[ROWS];
  if (red.xr) {
    const int cgr = gok ? c0 : c_win;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int oy = ty0 + rg * ROWS + i, ox = tx0 + xc;
      const int cy = oy < H ? oy : H - 1, cx = ox < W ? ox : W - 1;
      xrv[i] = *reinterpret_cast<const uint4*>(red.xr + (((long long)b * H + cy) * W + cx) * C + cgr);
    }
  }
  __syncthreads();
  auto lds8 = [&](int hy, int hx, f32x2 (&v)[4]) {
    const uint4 u = sh[(hy * HWD + hx) * 8 + g];
    v[0] = f32x2{bf_lo(u.x), bf_hi(u.x)}; v[1] = f32x2{bf_lo(u.y), bf_hi(u.y)};
    v[2] = f32x2{bf_lo(u.z), bf_hi(u.z)}; v[3] = f32x2{bf_lo(u.w), bf_hi(u.w)};
  };
  // win[row slot][kx][channel pair]: rows rotate while the thread walks down
  f32x2 win[3][3][4];
  const int r0 = rg * ROWS;                 // first output row (tile-local); halo row of output row r, tap ky: r + ky
#pragma unroll
  for (int ky = 0; ky < 2; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) lds8(r0 + ky, xc + kx, win[ky][kx]);
  float s = 0.f, ss = 0.f;
  float rs0[8], rs1[8], rmean = 0.f, rrstd = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) rs0[j] = rs1[j] = 0.f;
  if (red.xr && gok) gn_mean_rstd(red.stats + (long long)b * (C >> 4) * 2, c0 >> 4, 1, (float)H * W * 16.f, rmean, rrstd);
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) lds8(r0 + i + 2, xc + kx, win[(i + 2) % 3][kx]);
    const int oy = ty0 + r0 + i, ox = tx0 + xc;
    f32x2 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = bv[q];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_elementwise_fma(win[(i + ky) % 3][kx][q], wv[ky * 3 + kx][q], acc[q]);
      }
    if (gok && oy < H && ox < W) {
      uint4 u;
      u.x = pack_bf2(acc[0][0], acc[0][1]); u.y = pack_bf2(acc[1][0], acc[1][1]); u.z = pack_bf2(acc[2][0], acc[2][1]); u.w = pack_bf2(acc[3][0], acc[3][1]);
      *reinterpret_cast<uint4*>(yb + ((long long)oy * W + ox) * C + c0) = u;
      if (red.xr) {
        const uint4 xv = xrv[i];
        const float gq[8] = {bf_lo(u.x), bf_hi(u.x), bf_lo(u.y), bf_hi(u.y), bf_lo(u.z), bf_hi(u.z), bf_lo(u.w), bf_hi(u.w)};
        const float xq[8] = {bf_lo(xv.x), bf_hi(xv.x), bf_lo(xv.y), bf_hi(xv.y), bf_lo(xv.z), bf_hi(xv.z), bf_lo(xv.w), bf_hi(xv.w)};
#pragma unroll
        for (int j = 0; j < 8; ++j) { rs0[j] += gq[j]; rs1[j] += gq[j] * ((xq[j] - rmean) * rrstd); }
      }
      if (STATS) {
        s += bf_lo(u.x) + bf_hi(u.x) + bf_lo(u.y) + bf_hi(u.y) + bf_lo(u.z) + bf_hi(u.z) + bf_lo(u.w) + bf_hi(u.w);
        ss += bf_lo(u.x) * bf_lo(u.x) + bf_hi(u.x) * bf_hi(u.x) + bf_lo(u.y) * bf_lo(u.y) + bf_hi(u.y) * bf_hi(u.y) +
              bf_lo(u.z) * bf_lo(u.z) + bf_hi(u.z) * bf_hi(u.z) + bf_lo(u.w) * bf_lo(u.w) + bf_hi(u.w) * bf_hi(u.w);
      }
    }
  }
  if (STATS) {
    // lanes of a wave: granule = lane & 7 -> slab = (lane & 7) >> 1; fold the two granules of a slab and the 8 columns
    s += __shfl_xor(s, 1); ss += __shfl_xor(ss, 1);
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
    const int wave = t >> 6, l = t & 63;
    if (l < 8 && (l & 1) == 0) { sred[wave][(l >> 1) * 2] = s; sred[wave][(l >> 1) * 2 + 1] = ss; }
    __syncthreads();
    if (t < 8) {                              // (slab, moment) of this 64-channel window
      const float v = sred[0][t] + sred[1][t] + sred[2][t] + sred[3][t];
      const int slab = (c_win >> 4) + (t >> 1);
      if (slab < (C >> 4)) stat_add(&stats[((long long)b * (C >> 4) + slab) * 2 + (t & 1)], v);
    }
  }
  if (red.xr) {
    // fold the 8 columns of the wave, then the 4 waves through LDS (the halo image is no longer needed): [wave][128]
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { rs0[j] += __shfl_xor(rs0[j], o); rs1[j] += __shfl_xor(rs1[j], o); }
    }
    __syncthreads();
    float* fr = reinterpret_cast<float*>(sh);
    const int wave = t >> 6, l = t & 63;
    if (l < 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { fr[wave * 128 + (l * 8 + j) * 2] = rs0[j]; fr[wave * 128 + (l * 8 + j) * 2 + 1] = rs1[j]; }
    }
    __syncthreads();
    const int nch = nG * 8;
    if (t < 2 * nch) {                         // (channel, moment) of this window
      const float v = fr[t] + fr[128 + t] + fr[256 + t] + fr[384 + t];
      const int c = c_win + (t >> 1);
      grad_add(&red.r[((long long)b * C + c) * 2 + (t & 1)], v);
      fr[512 + t] = v * red.gamma[c];
    }
    __syncthreads();
    if (t < 2 * (nch >> 4)) {                  // gamma-weighted sums of the 16-channel groups
      const int grp = t >> 1, which = t & 1;
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) a += fr[512 + (grp * 16 + j) * 2 + which];
      grad_add(&red.r[(long long)gridDim.z * C * 2 + ((long long)b * (C >> 4) + (c_win >> 4) + grp) * 2 + which], a);
    }
  }
}

// dw10[tap][c] += sum_{b,p} dy[p][c]*x[p+tap][c] for tap < 9; dw10[9][c] += sum dy (the bias gradient).
// Same tiling as k_dwconv: per 8 x TW tile the x halo and the dy tile of a 64-channel window go to LDS with coalesced
// loads, thread (column, granule) walks down the rows with the 3x3 x-neighbourhood in registers and accumulates its 80
// sums; a workgroup runs over `tiles_per_wg` vertically adjacent tiles before it folds them (shuffles over the columns of
// a wave, LDS over the waves) and adds them into ONE of `replicas` copies of the accumulator: an fp32 global atomic
// costs ~2.6 ns per 128-byte line, serialised device-wide, so all workgroups on one copy would be the whole kernel time.
// The caller sums the copies (crd_wgrad_unpack).
// Two workgroups per CU (76 KB of LDS each): needs <= 256 registers.  The SLP vectoriser's build used 354 (one workgroup per CU, 196
// moves to and from accumulation registers); without it (build.py: -fno-slp-vectorize for this file) 255 + 28 bytes of scratch:
// 66 -> 39 us on stage 1, 38 -> 26 on stage 2.  (Bounded WITH the vectoriser: 456 bytes of scratch, 100 us.)
#ifndef CRD_DWW_WGS
#define CRD_DWW_WGS 2
#endif
template <int TW>
__global__ __launch_bounds__(TPB, CRD_DWW_WGS) void k_dwconv_wgrad(const bf16_t* x, const bf16_t* dy, int H, int W, int C, crd_sum_t* dw10,
                                                      int replicas, int tiles_x, int tiles_y, int tiles_per_wg, InNorm inn) {
  constexpr int HWD = TW + 2;
  constexpr int HPX = (DTH + 2) * HWD;
  constexpr int RSPLIT = 32 / TW;
  constexpr int ROWS = DTH / RSPLIT;
  extern __shared__ __attribute__((aligned(16))) uint4 dsm[];   // x halo [HPX][8] | dy tile [8*TW][8]
  uint4* sx = dsm;
  uint4* sdy = dsm + HPX * 8;
  const int b = blockIdx.z;
  const int c_win = blockIdx.y * DCW;
  const int txi = blockIdx.x % tiles_x, ygrp = blockIdx.x / tiles_x;
  const int tx0 = txi * TW;
  const bf16_t* xb = x + (long long)b * H * W * C;
  const bf16_t* db = dy + (long long)b * H * W * C;
  const int t = threadIdx.x;
  const int nG = (C - c_win) >= DCW ? 8 : (C - c_win) >> 3;
  const int g = t & 7, xc = (t >> 3) % TW, rg = (t >> 3) / TW;
  float acc[10][8];
#pragma unroll
  for (int tp = 0; tp < 10; ++tp)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[tp][j] = 0.f;
  float na[8], ns[8];
  for (int it = 0; it < tiles_per_wg; ++it) {
    const int tyi = ygrp * tiles_per_wg + it;
    if (tyi >= tiles_y) break;                     // uniform
    const int ty0 = tyi * DTH;
    {
      constexpr int NX = (HPX * 8 + TPB - 1) / TPB, ND = (DTH * TW * 8) / TPB;
      uint4 rx[NX], rd[ND];
      bool inimg[NX];
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const int i = t + k * TPB;
        const int hp = i >> 3, gg = i & 7;
        const int hy = hp / HWD, hx = hp - hy * HWD;
        const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
        inimg[k] = i < HPX * 8 && gg < nG && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        // (unconditional loads from a clamped address + select, as in k_dwconv)
        const int cy = iy < 0 ? 0 : (iy < H ? iy : H - 1), cx = ix < 0 ? 0 : (ix < W ? ix : W - 1), cgr = gg < nG ? gg : 0;
        const uint4 u = *reinterpret_cast<const uint4*>(xb + ((long long)cy * W + cx) * C + c_win + cgr * 8);
        rx[k] = inimg[k] ? u : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        const int i = t + k * TPB;
        const int pp = i >> 3, gg = i & 7;
        const int py = pp / TW, px = pp - py * TW;
        const int iy = ty0 + py, ix = tx0 + px;
        const int cy = iy < H ? iy : H - 1, cx = ix < W ? ix : W - 1, cgr = gg < nG ? gg : 0;
        const uint4 u = *reinterpret_cast<const uint4*>(db + ((long long)cy * W + cx) * C + c_win + cgr * 8);
        rd[k] = (gg < nG && iy < H && ix < W) ? u : make_uint4(0, 0, 0, 0);
      }
      if (it == 0) innorm_coeffs(inn, b, C, (long long)H * W, c_win + (t & 7) * 8, (t & 7) < nG, na, ns);   // under the first tile's loads
      if (it > 0) __syncthreads();                 // everyone is done with the previous tile's LDS image
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const int i = t + k * TPB;
        if (i < HPX * 8) sx[i] = (inn.stats && inimg[k]) ? innorm_apply(rx[k], na, ns) : rx[k];
      }
#pragma unroll
      for (int k = 0; k < ND; ++k) sdy[t + k * TPB] = rd[k];
    }
    __syncthreads();
    float win[3][3][8];
    const int r0 = rg * ROWS;
#pragma unroll
    for (int ky = 0; ky < 2; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) unpack8(sx[((r0 + ky) * HWD + xc + kx) * 8 + g], win[ky][kx]);
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) unpack8(sx[((r0 + i + 2) * HWD + xc + kx) * 8 + g], win[(i + 2) % 3][kx]);
      float d[8];
      unpack8(sdy[((r0 + i) * TW + xc) * 8 + g], d);      // zero outside the image / window
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[9][j] += d[j];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[ky * 3 + kx][j] += d[j] * win[(i + ky) % 3][kx][j];
        }
    }
  }
  // columns of the wave (lane bits 3..5), then the waves one after the other through LDS
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
    for (int tp = 0; tp < 10; ++tp)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[tp][j] += __shfl_xor(acc[tp][j], o);
  }
  __syncthreads();
  float* sm = reinterpret_cast<float*>(dsm);      // [10][64]
  const int wave = t >> 6, l = t & 63;
  for (int w = 0; w < 4; ++w) {
    if (wave == w && l < 8) {
#pragma unroll
      for (int tp = 0; tp < 10; ++tp)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float* p = &sm[tp * 64 + l * 8 + j];
          *p = w == 0 ? acc[tp][j] : *p + acc[tp][j];
        }
    }
    __syncthreads();
  }
  crd_sum_t* dst = dw10 + (long long)((blockIdx.z * gridDim.x + blockIdx.x) % replicas) * 10 * C;
  const int nch = nG * 8;
  for (int i = t; i < 10 * nch; i += TPB) {
    const int tp = i / nch, cl = i - tp * nch;
    const float v = sm[tp * 64 + cl];
    if (v != 0.f) grad_add(&dst[(long long)tp * C + c_win + cl], v);
  }
}

}  // namespace

// tile width: 32; 16 for images at most 16 pixels wide (W = 13).  (Round 2 chose 16 whenever it wasted fewer columns -- W = 104:
// 112 instead of 128 -- but the 32-wide tiles are faster there: 19.56 -> 19.48 ms per step.)  CRD_DW_TW (developer switch) forces one.
static int dw_tile_width(int W) {
  static int forced = -1;
  if (forced < 0) forced = crd_dev_int("CRD_DW_TW", 0);
  if (forced == 16 || forced == 32) return forced;
  return W <= 16 ? 16 : 32;
}

extern "C" int crd_dwconv3x3(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* w9, const float* bias,
                             int32_t flip, void* y, crd_sum_t* stats, const crd_sum_t* in_stats, int32_t in_gmul,
                             const float* in_gamma, const float* in_beta, const void* red_x, const crd_sum_t* red_stats,
                             const float* red_gamma, crd_sum_t* red_r, crd_stream_t stream) {
  CRD_CHECK_ARG(x && w9 && y, "crd_dwconv3x3: null pointer");
  CRD_CHECK_ARG(!red_x || (red_stats && red_gamma && red_r), "crd_dwconv3x3: incomplete fused-reduce arguments");
  const RedOut red{reinterpret_cast<const bf16_t*>(red_x), red_stats, red_gamma, red_r};
  CRD_CHECK_ARG(!in_stats || (in_gamma && in_beta && in_gmul >= 1 && (C / 16) % in_gmul == 0), "crd_dwconv3x3: bad input-norm arguments");
  const InNorm inn{in_stats, in_gamma, in_beta, in_gmul};
  CRD_CHECK_ARG(C % 16 == 0, "crd_dwconv3x3: C must be a multiple of 16");
  const bf16_t* xp = reinterpret_cast<const bf16_t*>(x);
  bf16_t* yp = reinterpret_cast<bf16_t*>(y);
  hipStream_t st = as_stream(stream);
  // tile width: 32, or 16 when that wastes fewer columns (W = 13: 16 instead of 32)
  const int tw = dw_tile_width(W);
  const int tiles_x = cdiv(W, tw), tiles_y = cdiv(H, DTH);
  dim3 grid(tiles_x * tiles_y, cdiv(C, DCW), B);
#define CRD_DW(FL, STT, TWV) hipLaunchKernelGGL((k_dwconv<FL, STT, TWV>), grid, dim3(TPB), 0, st, xp, H, W, C, w9, bias, yp, stats, tiles_x, inn, red)
  if (tw == 32) {
    if (flip) { if (stats) CRD_DW(true, true, 32); else CRD_DW(true, false, 32); }
    else { if (stats) CRD_DW(false, true, 32); else CRD_DW(false, false, 32); }
  } else {
    if (flip) { if (stats) CRD_DW(true, true, 16); else CRD_DW(true, false, 16); }
    else { if (stats) CRD_DW(false, true, 16); else CRD_DW(false, false, 16); }
  }
#undef CRD_DW
  CRD_LAUNCH_CHECK("crd_dwconv3x3");
  return CRD_OK;
}

extern "C" int crd_dwconv3x3_wgrad(const void* x, const void* dy, int32_t B, int32_t H, int32_t W, int32_t C, crd_sum_t* dw10,
                                   int32_t replicas, const crd_sum_t* in_stats, int32_t in_gmul, const float* in_gamma,
                                   const float* in_beta, crd_stream_t stream) {
  CRD_CHECK_ARG(x && dy && dw10 && replicas >= 1, "crd_dwconv3x3_wgrad: null pointer / replicas < 1");
  CRD_CHECK_ARG(!in_stats || (in_gamma && in_beta && in_gmul >= 1 && (C / 16) % in_gmul == 0), "crd_dwconv3x3_wgrad: bad input-norm arguments");
  const InNorm inn{in_stats, in_gamma, in_beta, in_gmul};
  CRD_CHECK_ARG(C % 16 == 0 && C <= 4096, "crd_dwconv3x3_wgrad: C must be a multiple of 16, <= 4096");
  const int tw = dw_tile_width(W);
  const int tiles_x = cdiv(W, tw), tiles_y = cdiv(H, DTH), wins = cdiv(C, DCW);
  // vertical runs of tiles per workgroup: as long as possible (one fold + one set of atomics per run) while ~512
  // workgroups (two per CU: 76 KB of LDS each) remain
  int ysplit = cdiv(512, (long long)tiles_x * wins * B);
  if (ysplit > tiles_y) ysplit = tiles_y;
  if (ysplit < 1) ysplit = 1;
  const int per = cdiv(tiles_y, ysplit);
  ysplit = cdiv(tiles_y, per);
  dim3 grid(tiles_x * ysplit, wins, B);
  const bf16_t* xp = reinterpret_cast<const bf16_t*>(x);
  const bf16_t* dp = reinterpret_cast<const bf16_t*>(dy);
  hipStream_t st = as_stream(stream);
  if (tw == 32) {
    const size_t lds = (size_t)((DTH + 2) * 34 * 8 + DTH * 32 * 8) * sizeof(uint4);
    crd_reserve_lds_once<&k_dwconv_wgrad<32>>((int)lds, "k_dwconv_wgrad");
    hipLaunchKernelGGL(k_dwconv_wgrad<32>, grid, dim3(TPB), lds, st, xp, dp, H, W, C, dw10, replicas, tiles_x, tiles_y, per, inn);
  } else {
    const size_t lds = (size_t)((DTH + 2) * 18 * 8 + DTH * 16 * 8) * sizeof(uint4);
    crd_reserve_lds_once<&k_dwconv_wgrad<16>>((int)lds, "k_dwconv_wgrad");
    hipLaunchKernelGGL(k_dwconv_wgrad<16>, grid, dim3(TPB), lds, st, xp, dp, H, W, C, dw10, replicas, tiles_x, tiles_y, per, inn);
  }
  CRD_LAUNCH_CHECK("crd_dwconv3x3_wgrad");
  return CRD_OK;
}
