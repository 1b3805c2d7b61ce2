// Encoder-side kernels for gfx950: depthwise 3x3 (+wgrad) and the max-pool attention of the
// Simplified Transformer (fused QK^T + scale + row-max on MFMA, rank-1 output, backward).
// The head of the attention backward exists in two forms: k_attn_out_bwd + k_attn_scores_bwd + k_sum_partials_bf16 (three launches,
// dS through memory, the rank-one vector path riding in the second; also the fallback for shapes whose masks do not fit in LDS), and
// k_attn_bwd_fused + k_attn_dk_fold (two launches: output and score backward as one workgroup-local pass per pixel chunk, dS through
// LDS, the vector path riding in the fold).  dx1, dS, dq and the dK partials are the same bits in both.
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
  auto unpack8 = [&](const uint4& u, float (&v)[8]) {
    v[0] = bf_lo(u.x); v[1] = bf_hi(u.x); v[2] = bf_lo(u.y); v[3] = bf_hi(u.y);
    v[4] = bf_lo(u.z); v[5] = bf_hi(u.z); v[6] = bf_lo(u.w); v[7] = bf_hi(u.w);
  };
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

// Rank-one value path of the attention forward (documented at k_attn_xbar_proj below); also run by one extra workgroup
// per sample of k_attn_scores (crd_attn_fwd), hence blockDim-strided.
// y[r] = sum_c W[r][c] * sx[c] for the rows [r_lo, r_hi) of a bf16 matrix with `ld` elements per row: a wave takes four rows at
// a time, its lanes run along the columns (coalesced 16-byte loads, 512 columns per pass), the products are folded with the wave
// butterfly.  (One thread per row walking its 1 KB row 16 bytes at a time was a chain of 64 uncoalesced loads: the [C x C] vector
// products of the attention's rank-one path.)  The sums are taken in fp64: these per-sample vectors are broadcast over every pixel
// of the sample (x1 = x + bf16(u * S + bp)), so their rounding error is COHERENT across the image instead of averaging out, and the
// value should not depend on how the sum is grouped -- with the golden weights, the fp32 sum in this order instead of row-sequential
// (a 1e-7 relative difference in u) moved the 928 x 1600 comparison with the reference from 0.048 to 0.121.
template <class PRE, class F>
__device__ __forceinline__ void matvec_rows(const bf16_t* w, int ld, int r_lo, int r_hi, int ncols, const float* sx, PRE&& pre, F&& out) {
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  auto load_rows = [&](int r0, int c0, float (&wv)[4][8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k < r_hi ? r0 + k : r_hi - 1;                // (clamped: unconditional loads; the extra rows are not stored)
      load8(w + (long long)r * ld, c0 < ncols ? c0 : 0, 0, wv[k]);
    }
  };
  // the first batch of weight rows does not depend on the vector: it is requested before `pre` builds the vector in LDS
  // (pre() ends with the workgroup barrier; every thread calls it exactly once)
  float w0[4][8];
  const int r_first = r_lo + wave * 4;
  load_rows(r_first < r_hi ? r_first : r_lo, l * 8, w0);
  pre();
  for (int r0 = r_first; r0 < r_hi; r0 += nw * 4) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};             // fp64: see above
    for (int c0 = l * 8; c0 < ncols; c0 += 512) {
      float wv[4][8];
      if (r0 == r_first && c0 == l * 8) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int j = 0; j < 8; ++j) wv[k][j] = w0[k][j];
      } else {
        load_rows(r0, c0, wv);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k] += (double)wv[k][j] * (double)sx[c0 + j];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    if (l == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (r0 + k < r_hi) out(r0 + k, (float)acc[k]);
    }
  }
}
constexpr int VEC_ROWS = 64;       // rows of the [C x C] vector products per extra workgroup

struct XbarProj { const crd_sum_t* chan; const crd_sum_t* stats; const float* gamma; const float* beta; const bf16_t* w; int N, C; bf16_t* xbar; float* u; };
// part e of cdiv(C, VEC_ROWS): every part rebuilds xbar (C values from the sums) and owns VEC_ROWS rows of u; part 0 stores xbar
__device__ __forceinline__ void attn_xbar_proj_body(const XbarProj& x, int b, int e) {
  __shared__ float sx[1024];
  const int C = x.C, N = x.N, nt = blockDim.x;
  const int r_lo = e * VEC_ROWS, r_hi = r_lo + VEC_ROWS < C ? r_lo + VEC_ROWS : C;
  float* ub = x.u + (long long)b * C;
  matvec_rows(x.w, C, r_lo, r_hi, C, sx,
              [&]() {
                for (int c = threadIdx.x; c < C; c += nt) {
                  float mean, rstd;
                  gn_mean_rstd(x.stats + (long long)b * (C >> 4) * 2, c >> 4, 1, (float)N * 16.f, mean, rstd);
                  const float mc = stat_get(&x.chan[((long long)b * C + c) * 2]) / (float)N;
                  const bf16_t q = f2bf(x.gamma[c] * (mc - mean) * rstd + x.beta[c]);
                  if (e == 0) x.xbar[(long long)b * C + c] = q;
                  sx[c] = bf2f(q);
                }
                __syncthreads();
              },
              [&](int r, float v) { ub[r] = v; });
}

// ------------------------------------------------------------------------------------------------
// Attention scores: per head h,  s[n] = max_m bf16(bf16(q_n . k_m) * scale)  (the reference's
// autocast rounding points), S[n] = sum_h s_h[n].  MFMA operands are swapped -- A = K tile (rows =
// keys), B = Q tile (cols = queries) -- so each lane owns ONE query column and the 16 accumulator
// registers hold 16 keys: the max over keys is in-register plus one cross-half shuffle.
// One wave = 32 queries; K/Q fragments are read straight from L2-resident global memory.
// ------------------------------------------------------------------------------------------------
// One wave = 32 queries x ONE head (blockDim = 64 * heads * qg: wave w -> head w % heads, query group w / heads), so the
// per-head chain of dependent loads runs in parallel across the waves instead of serially inside one (stage 4: 8 heads);
// the heads' maxima of a query group meet in LDS.
__global__ __launch_bounds__(1024) void k_attn_scores(const bf16_t* q, const bf16_t* k, int N, int M, int heads, int d,
                                                      float scale, float* S, short* idx, int qg, XbarProj xp) {
  __shared__ float smax[16][32];
  const int b = blockIdx.y;
  // crd_attn_fwd: the value path, in the FIRST workgroups of the sample (a dependent chain of ~6 us: dispatched last, behind the
  // score tiles, it ended the launch 1.6 us late at stage 1)
  const int nvec = xp.chan ? (xp.C + VEC_ROWS - 1) / VEC_ROWS : 0;
  if ((int)blockIdx.x < nvec) { attn_xbar_proj_body(xp, b, blockIdx.x); return; }
  const int tile_x = blockIdx.x - nvec;
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = wave % heads, g = wave / heads;
  const int n0 = (tile_x * qg + g) * 32;
  const int C = heads * d;
  const int n = n0 + (l & 31);
  const bool nok = n < N;
  const bf16_t* qb = q + ((long long)b * N + (nok ? n : 0)) * C;
  const bf16_t* kb = k + (long long)b * M * C;
  const int half = l >> 5;
  // query fragments for this head (B operand: col = lane&31, k = 8*half + j within each 16-chunk)
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int kk = ks * 16 + half * 8;
    uint4 u = *reinterpret_cast<const uint4*>(qb + h * d + (kk < d ? kk : 0));       // (qb is row 0 for queries past N)
    if (kk >= d) u = make_uint4(0, 0, 0, 0);
    qf[ks] = *reinterpret_cast<bf16x8*>(&u);
  }
  float best = -INFINITY;
  int besti = 0;
  // key fragments (A operand: row = lane&31 -> key, k = 8*half + j) go through a ring of four 32-key tiles: a tile is requested
  // four tiles before the MFMAs that consume it.  Every load is UNCONDITIONAL (clamped row, columns past d zeroed by a select) and
  // the tile loop has no branch in its body: with `if (row < M) load` the compiler's wait insertion gave up and put
  // s_waitcnt vmcnt(0) in front of every use (29 of them), i.e. one full memory latency per tile whatever was prefetched --
  // 1.2 us per 32 keys, 16-19 us for the 325 keys of a 416 x 800 frame at every stage.
  const bool kcol_ok[4] = {half * 8 < d, 16 + half * 8 < d, 32 + half * 8 < d, 48 + half * 8 < d};
  auto load_keys = [&](int m0, uint4 (&dst)[4]) {
    int mrow = m0 + (l & 31);
    mrow = mrow < M ? mrow : M - 1;
    const bf16_t* rowp = kb + (long long)mrow * C + h * d;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) dst[ks] = *reinterpret_cast<const uint4*>(rowp + (kcol_ok[ks] ? ks * 16 + half * 8 : 0));
  };
  auto score_tile = [&](int m0, const uint4 (&kt)[4]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      uint4 kf = kt[ks];
      if (!kcol_ok[ks]) kf = make_uint4(0, 0, 0, 0);                  // (v_cndmask, no branch)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&kf), qf[ks], acc, 0, 0, 0);
    }
    // The kernel is bound by THIS: the two bf16 roundings, the scale, compare and two selects per score are vector instructions
    // (4 clocks each per wave), the MFMAs a quarter of that.  Roundings in pairs through v_cvt_pk_bf16_f32 (one instruction per
    // two values + one shift / mask each to widen again, instead of three integer operations per value); selects only -- as
    // `if (m < M && v > best)` this compiled to two exec-mask branches per key; the `m < M` select only in a tile that crosses M.
    const bool edge = m0 + 32 > M;                                    // wave-uniform
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const int ma = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;          // r even: the pair is keys ma, ma + 1
      const uint32_t p1 = pack_bf2(acc[r], acc[r + 1]);
      const uint32_t p2 = pack_bf2(bf_lo(p1) * scale, bf_hi(p1) * scale);
      float va = bf_lo(p2), vb = bf_hi(p2);
      if (edge) { va = ma < M ? va : -INFINITY; vb = ma + 1 < M ? vb : -INFINITY; }      // rows past M (clamped re-reads) never win
      const bool ta = va > best;
      best = ta ? va : best;
      besti = ta ? ma : besti;
      const bool tb = vb > best;
      best = tb ? vb : best;
      besti = tb ? ma + 1 : besti;
    }
  };
  uint4 ring[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) load_keys(j * 32, ring[j]);
  for (int m0 = 0; m0 < M; m0 += 128) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      score_tile(m0 + j * 32, ring[j]);
      __builtin_amdgcn_sched_barrier(0);               // keep the refill HERE: the scheduler otherwise sinks the ring's loads next
      load_keys(m0 + j * 32 + 128, ring[j]);           // to their uses (one latency per pass again)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // combine the two half-waves (same query column, other 16 rows of every tile)
  float ob = __shfl_xor(best, 32);
  int oi = __shfl_xor(besti, 32);
  if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  if (nok && half == 0) idx[((long long)b * N + n) * heads + h] = (short)besti;
  if (half == 0) smax[wave][l] = best;
  __syncthreads();
  if (h == 0 && half == 0 && nok) {       // S = sum over heads, in head order (as the serial loop did)
    float Ssum = 0.f;
    for (int hh = 0; hh < heads; ++hh) Ssum += smax[g * heads + hh][l];
    S[(long long)b * N + n] = Ssum;
  }
}

// ------------------------------------------------------------------------------------------------
// Config 5 experiment (round 6, BASELINE.json configs[4] "fp8 MFMA attention"): the same scores with e4m3 operands --
// s[n] = max_m bf16(bf16(qs ks (q8_n . k8_m)) * scale) -- on v_mfma_scale_f32_32x32x64_f8f6f4 (block scales 2^0): ONE K = 64 MFMA per
// 32-key tile instead of four bf16 ones, half the operand bytes.  q8 / k8: per-tensor-scaled e4m3 copies, rows [heads][64] bytes (the
// head dimension zero-padded to 64: two 16-byte granules per lane and no masking).  Everything behind the MFMA -- roundings, compare,
// arg-max selects, the head sum -- is the bf16 kernel's.  Measured and NOT wired into the plan: see DESIGN.md "Round 6".
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_attn_scores_fp8(const unsigned char* q8, const unsigned char* k8, int N, int M, int heads,
                                                          float qk_scale, float scale, float* S, short* idx, int qg) {
  typedef __attribute__((ext_vector_type(8))) int i32x8;
  typedef __attribute__((ext_vector_type(4))) int i32x4;
  __shared__ float smax[16][32];
  const int b = blockIdx.y;
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = wave % heads, g = wave / heads;
  const int n0 = (blockIdx.x * qg + g) * 32;
  const int n = n0 + (l & 31);
  const bool nok = n < N;
  const int half = l >> 5;
  const int RS = heads * 64;                                          // bytes per row
  const unsigned char* qrow = q8 + ((long long)b * N + (nok ? n : 0)) * RS + h * 64;
  const unsigned char* kb = k8 + (long long)b * M * RS + h * 64;
  // a lane's operand: 32 of the row's 64 bytes -- granules `half` and 2 + `half`, the same choice for keys and queries
  const i32x4 q_lo = *reinterpret_cast<const i32x4*>(qrow + half * 16), q_hi = *reinterpret_cast<const i32x4*>(qrow + (2 + half) * 16);
  const i32x8 qf = __builtin_shufflevector(q_lo, q_hi, 0, 1, 2, 3, 4, 5, 6, 7);
  const int SC = 0x7f7f7f7f;
  float best = -INFINITY;
  int besti = 0;
  auto load_keys = [&](int m0, i32x4 (&dst)[2]) {
    int mrow = m0 + (l & 31);
    mrow = mrow < M ? mrow : M - 1;
    const unsigned char* rowp = kb + (long long)mrow * RS;
    dst[0] = *reinterpret_cast<const i32x4*>(rowp + half * 16);
    dst[1] = *reinterpret_cast<const i32x4*>(rowp + (2 + half) * 16);
  };
  auto score_tile = [&](int m0, const i32x4 (&kt)[2]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const i32x8 kf = __builtin_shufflevector(kt[0], kt[1], 0, 1, 2, 3, 4, 5, 6, 7);
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf, qf, acc, 0, 0, 0, SC, 0, SC);
    const bool edge = m0 + 32 > M;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const int ma = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const uint32_t p1 = pack_bf2(acc[r] * qk_scale, acc[r + 1] * qk_scale);
      const uint32_t p2 = pack_bf2(bf_lo(p1) * scale, bf_hi(p1) * scale);
      float va = bf_lo(p2), vb = bf_hi(p2);
      if (edge) { va = ma < M ? va : -INFINITY; vb = ma + 1 < M ? vb : -INFINITY; }
      const bool ta = va > best;
      best = ta ? va : best;
      besti = ta ? ma : besti;
      const bool tb = vb > best;
      best = tb ? vb : best;
      besti = tb ? ma + 1 : besti;
    }
  };
  i32x4 ring[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) load_keys(j * 32, ring[j]);
  for (int m0 = 0; m0 < M; m0 += 128) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      score_tile(m0 + j * 32, ring[j]);
      __builtin_amdgcn_sched_barrier(0);
      load_keys(m0 + j * 32 + 128, ring[j]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  float ob = __shfl_xor(best, 32);
  int oi = __shfl_xor(besti, 32);
  if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  if (nok && half == 0) idx[((long long)b * N + n) * heads + h] = (short)besti;
  if (half == 0) smax[wave][l] = best;
  __syncthreads();
  if (h == 0 && half == 0 && nok) {
    float Ssum = 0.f;
    for (int hh = 0; hh < heads; ++hh) Ssum += smax[g * heads + hh][l];
    S[(long long)b * N + n] = Ssum;
  }
}

// xbar[b][c] = mean_n GN(x)[b][n][c] = gamma_c*(mean_n x_c - mu_g)*rstd_g + beta_c   (bf16 out)
__global__ void k_attn_xbar(const crd_sum_t* chan, const crd_sum_t* stats, const float* gamma, const float* beta, int N, int C,
                            bf16_t* xbar) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float mean, rstd;
    gn_mean_rstd(stats + (long long)b * (C >> 4) * 2, c >> 4, 1, (float)N * 16.f, mean, rstd);
    float mc = stat_get(&chan[((long long)b * C + c) * 2]) / (float)N;
    xbar[(long long)b * C + c] = f2bf(gamma[c] * (mc - mean) * rstd + beta[c]);
  }
}

// Rank-one value path of the attention in one launch per direction (they were xbar + a [B,1,C] 1x1 "conv", and a
// conversion + [B,1,C] data-gradient "conv" + a scale: three to four dependent dispatches of a few hundred threads).
// Forward: xbar[b][c] = bf16(mean_n GroupNorm(x)[b][n][c]) (as k_attn_xbar), u[b][co] = sum_ci W[co][ci] * xbar[b][ci]
// with W the proj weight in its packed bf16 forward form [C][C] (bf16 products, fp32 accumulation, as the MFMA path).
__global__ __launch_bounds__(TPB) void k_attn_xbar_proj(XbarProj x) { attn_xbar_proj_body(x, blockIdx.y, blockIdx.x); }

// Backward: tb = bf16(t); es[b][ci] = inv_n * sum_co W[co][ci] * tb[b][co], with wt the proj weight in its packed bf16
// data-gradient form [C][Cpad] (row ci, contiguous over co).
struct VecBwd { const crd_sum_t* t; const bf16_t* wt; int C, Cpad; float inv_n; bf16_t* tb; float* es; };
// (part e owns `rows` rows of es; a row's sum does not depend on the split)
__device__ __forceinline__ void attn_vec_bwd_body(const VecBwd& v, int b, int e, int rows = VEC_ROWS) {
  __shared__ float st[1024];
  const int C = v.C;
  const int r_lo = e * rows, r_hi = r_lo + rows < C ? r_lo + rows : C;
  float* eb = v.es + (long long)b * C;
  const float inv_n = v.inv_n;
  matvec_rows(v.wt, v.Cpad, r_lo, r_hi, C, st,
              [&]() {
                for (int c = threadIdx.x; c < C; c += TPB) {
                  const bf16_t q = f2bf(grad_get(&v.t[(long long)b * C + c]));
                  if (e == 0) v.tb[(long long)b * C + c] = q;
                  st[c] = bf2f(q);
                }
                __syncthreads();
              },
              [&](int r, float a) { eb[r] = a * inv_n; });
}
__global__ __launch_bounds__(TPB) void k_attn_vec_bwd(VecBwd v) { attn_vec_bwd_body(v, blockIdx.y, blockIdx.x); }

// x1 = x + dp[b]*bf16(u[b][c]*S[b][n] + bp[c])
__global__ __launch_bounds__(TPB) void k_attn_out_residual(const float* x, const float* u, const float* S, const float* bp,
                                                           const float* dp, long long N, int C, float* x1) {
  const int b = blockIdx.y;
  const int CG = C >> 3;
  const long long total = N * CG;
  const float dps = dp ? dp[b] : 1.f;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int cg = (int)(i % CG);
    const long long n = i / CG;
    const float s = S[(long long)b * N + n];
    float v[8], uu[8], bb[8];
    const long long off = ((long long)b * N + n) * C + cg * 8;
    load8(x, off, 1, v);
    load8(u, (long long)b * C + cg * 8, 1, uu);
    load8(bp, cg * 8, 1, bb);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += dps * bf_round(uu[j] * s + bb[j]);
    store8_f32(x1, off, v);
  }
}

// dy = dp[b]*dx1:  t[b][c] += sum_n dy*S ; dbp_rows[b][c] += sum_n dy ; dS[b][n] = sum_c dy*u[b][c]
// Four pixel groups are loaded per iteration (one load in flight per thread left the kernel latency-bound); the sums are
// folded over the wave's pixel lanes with shuffles and over the waves through LDS, then added with one atomic per value
// and workgroup into PER-SAMPLE rows (chain depth = workgroups of the sample; crd_wgrad_unpack sums the rows of dbp).
// PRE: the apply phase of Block.norm2's backward runs first, in the same threads -- dx1 += (gamma * dxn - S1 - xhat * S2) * rstd with
// xhat from the fp32 residual stream x, (S1, S2) the group sums crd_gn_bwd_reduce / the fc1 data-gradient epilogue left in r --
// crd_gn_bwd_apply's arithmetic for an fp32 accumulating output without activation or mask, written back to dx1 (the residual
// gradient the rest of the block's backward continues with).  The parameter gradients of that GroupNorm come from r as there.
struct GnPre {
  const float* x; const bf16_t* dxn; const crd_sum_t* stats; const float* gamma; const crd_sum_t* r; float* dgamma; float* dbeta; int B;
};
template <bool PRE>
__global__ __launch_bounds__(TPB) void k_attn_out_bwd(float* dx1, const float* u, const float* S, const float* dp,
                                                      long long N, int C, int chunk, crd_sum_t* t, crd_sum_t* dbp_rows, float* dS, GnPre pre) {
  extern __shared__ float sm[];  // [2][C]
  const int b = blockIdx.y;
  const int CG = C >> 3;
  int W2 = 1;
  while (W2 < CG) W2 <<= 1;           // lanes per pixel (power of two, <= 64 since C <= 512)
  const int PPW = 64 / W2;            // pixels per wave-iteration
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = l / W2, cg = l % W2;
  const bool cok = cg < CG;
  const float dps = dp ? dp[b] : 1.f;
  float uu[8], ta[8], ba[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { uu[j] = cok ? u[(long long)b * C + cg * 8 + j] : 0.f; ta[j] = ba[j] = 0.f; }
  long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk;
  if (p1 > N) p1 = N;
  float ga[8], mean = 0.f, rstd = 0.f, S1 = 0.f, S2 = 0.f;
  if (PRE) {
    if (b == 0 && pre.dgamma) {       // parameter gradients: the workgroups of sample 0 share the channels (as k_gn_bwd_apply)
      for (int c = blockIdx.x * TPB + threadIdx.x; c < C; c += gridDim.x * TPB) {
        const float ob = pre.dbeta[c], og = pre.dgamma[c];
        long long g0, g1;
        sum_samples(pre.r, pre.B, C, c, g0, g1);
        pre.dbeta[c] = ob + (float)g0 * (1.f / GRAD_ONE);
        pre.dgamma[c] = og + (float)g1 * (1.f / GRAD_ONE);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) ga[j] = cok ? pre.gamma[cg * 8 + j] : 0.f;
    if (cok) {
      const int grp = cg >> 1;                                    // 16-channel groups (gmul = 1)
      const float inv_m = 1.f / ((float)N * 16.f);
      const crd_sum_t* rg = pre.r + (long long)pre.B * C * 2 + ((long long)b * (C >> 4) + grp) * 2;
      S1 = grad_get(rg) * inv_m; S2 = grad_get(rg + 1) * inv_m;
      gn_mean_rstd(pre.stats + (long long)b * (C >> 4) * 2, grp, 1, (float)N * 16.f, mean, rstd);
    }
  }
  constexpr int UN = 4;
  for (long long nb = p0 + wave * PPW; nb < p1; nb += (long long)UN * 4 * PPW) {
    float v[UN][8], s[UN];
    float xv[PRE ? UN : 1][8], dv[PRE ? UN : 1][8];
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const long long n = nb + (long long)k * 4 * PPW + sub;
      const bool ok = cok && n < p1;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
      s[k] = 0.f;
      if (ok) {
        const long long off = ((long long)b * N + n) * C + cg * 8;
        load8(dx1, off, 1, v[k]); s[k] = S[(long long)b * N + n];
        if (PRE) { load8(pre.x, off, 1, xv[PRE ? k : 0]); load8(pre.dxn, off, 0, dv[PRE ? k : 0]); }
      }
    }
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const long long n = nb + (long long)k * 4 * PPW + sub;
      if (PRE && cok && n < p1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (xv[PRE ? k : 0][j] - mean) * rstd;
          float o = (ga[j] * dv[PRE ? k : 0][j] - S1 - xh * S2) * rstd;
          o += v[k][j];
          v[k][j] = o;
        }
        store8_f32(dx1, ((long long)b * N + n) * C + cg * 8, v[k]);
      }
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[k][j] *= dps; dot += v[k][j] * uu[j]; ta[j] += v[k][j] * s[k]; ba[j] += v[k][j]; }
      for (int o = W2 >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
      if (cok && n < p1 && cg == 0) dS[(long long)b * N + n] = dot;
    }
  }
  for (int o = W2; o < 64; o <<= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { ta[j] += __shfl_xor(ta[j], o); ba[j] += __shfl_xor(ba[j], o); }
  }
  for (int w = 0; w < 4; ++w) {
    if (wave == w && sub == 0 && cok) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float* p0_ = &sm[cg * 8 + j];
        float* p1_ = &sm[C + cg * 8 + j];
        *p0_ = w == 0 ? ta[j] : *p0_ + ta[j];
        *p1_ = w == 0 ? ba[j] : *p1_ + ba[j];
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < C; i += TPB) {
    grad_add(&t[(long long)b * C + i], sm[i]);
    grad_add(&dbp_rows[(long long)b * C + i], sm[C + i]);
  }
}

// dq[b][n][c] = scale*dS[b][n]*k[b][idx[b][n][h(c)]][c] ; dk[b][m][c] += scale*dS[b][n]*q[b][n][c]
__global__ __launch_bounds__(TPB) void k_attn_scores_bwd(const bf16_t* q, const bf16_t* k, const float* dS, const short* idx,
                                                         long long N, int M, int heads, int d, float scale, int chunk,
                                                         bf16_t* dq, crd_sum_t* dk, int use_lds, float* dk_part, VecBwd vec) {
  // LDS (use_lds): the workgroup's pixel chunk -- q rows [chunk][CG] (16-byte granules), g = scale*dS [chunk], and per
  // (head, key) a BITMASK over the chunk's pixels: bit n set <=> pixel n's arg-max for that head is this key
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.y;
  // cdiv(C, 64) extra workgroups per sample run the rank-one vector path of the same backward step (crd_attn_bwd: it depends on
  // the same producer, crd_attn_out_bwd, and a launch of its own cost more than its work)
  const int nvec = vec.t ? (vec.C + VEC_ROWS - 1) / VEC_ROWS : 0;
  if ((int)blockIdx.x < nvec) { attn_vec_bwd_body(vec, b, blockIdx.x); return; }
  const int chunk_x = blockIdx.x - nvec;
  const int C = heads * d, CG = C >> 3;
  long long p0 = (long long)chunk_x * chunk, p1 = p0 + chunk;
  if (p1 > N) p1 = N;
  const int npx = (int)(p1 - p0);
  const int HM = heads * M, WPC = (chunk + 31) >> 5;                           // mask words per (head, key)
  uint4* sq = reinterpret_cast<uint4*>(smem);                                  // [chunk][CG]
  float* sg = reinterpret_cast<float*>(smem + (size_t)chunk * C * 2);          // [chunk]
  unsigned* mask = reinterpret_cast<unsigned*>(sg + chunk);                    // [HM][WPC]
  if (use_lds) {
    for (int i = threadIdx.x; i < HM * WPC; i += TPB) mask[i] = 0u;
    __syncthreads();
  }
  const long long total = (long long)npx * CG;
  // UB items per thread and pass: first the index / gradient scalars of all of them, then the dependent row gathers, so
  // that a pass costs two memory latencies instead of two per item
  constexpr int UB = 4;
  for (long long i0 = threadIdx.x; i0 < total; i0 += (long long)UB * TPB) {
    int cgv[UB], mv[UB];
    long long nv[UB];
    float gv[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const long long i = i0 + (long long)u * TPB;
      const bool ok = i < total;
      cgv[u] = ok ? (int)(i % CG) : 0;
      nv[u] = ok ? p0 + i / CG : p0;
      const int h = (cgv[u] * 8) / d;
      mv[u] = idx[((long long)b * N + nv[u]) * heads + h];
      gv[u] = ok ? scale * dS[(long long)b * N + nv[u]] : 0.f;
    }
    uint4 kraw[UB], qraw[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      kraw[u] = *reinterpret_cast<const uint4*>(k + ((long long)b * M + mv[u]) * C + cgv[u] * 8);
      qraw[u] = *reinterpret_cast<const uint4*>(q + ((long long)b * N + nv[u]) * C + cgv[u] * 8);
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if (i0 + (long long)u * TPB >= total) continue;
      float kv[8];
      kv[0] = bf_lo(kraw[u].x); kv[1] = bf_hi(kraw[u].x); kv[2] = bf_lo(kraw[u].y); kv[3] = bf_hi(kraw[u].y);
      kv[4] = bf_lo(kraw[u].z); kv[5] = bf_hi(kraw[u].z); kv[6] = bf_lo(kraw[u].w); kv[7] = bf_hi(kraw[u].w);
#pragma unroll
      for (int j = 0; j < 8; ++j) kv[j] *= gv[u];
      store8_bf16(dq, ((long long)b * N + nv[u]) * C + cgv[u] * 8, kv);
      if (use_lds) {
        const int nl = (int)(nv[u] - p0);
        sq[nl * CG + cgv[u]] = qraw[u];
        const int h = (cgv[u] * 8) / d;
        // one bit per (pixel, head): integer LDS atomic, the result does not depend on the order
        if (cgv[u] * 8 == h * d) atomicOr(&mask[(h * M + mv[u]) * WPC + (nl >> 5)], 1u << (nl & 31));
        if (cgv[u] == 0) sg[nl] = gv[u];
      } else {
        float qv[8];
        qv[0] = bf_lo(qraw[u].x); qv[1] = bf_hi(qraw[u].x); qv[2] = bf_lo(qraw[u].y); qv[3] = bf_hi(qraw[u].y);
        qv[4] = bf_lo(qraw[u].z); qv[5] = bf_hi(qraw[u].z); qv[6] = bf_lo(qraw[u].w); qv[7] = bf_hi(qraw[u].w);
        crd_sum_t* dst = &dk[((long long)b * M + mv[u]) * C + cgv[u] * 8];
#pragma unroll
        for (int j = 0; j < 8; ++j) grad_add(dst + j, gv[u] * qv[j]);
      }
    }
  }
  if (!use_lds) return;
  // dK of the chunk without float atomics (32 ds_add_f32 per thread were 20 of this kernel's 28 us: LDS fp32 atomics
  // retire about one lane every few cycles) and in a FIXED order: the thread that owns (key m, granule cg) walks the set
  // bits of the key's mask -- the pixels routed to m, in ascending order -- and adds up their q rows.  (Round 2 built
  // per-key pixel lists with an LDS cursor atomic: a count pass, a scan and a fill pass more, and a summation order that
  // changed from run to run.)
  __syncthreads();
  float* outp = dk_part ? dk_part + ((long long)chunk_x * gridDim.y + b) * M * C : nullptr;
  for (int pr = threadIdx.x; pr < M * CG; pr += TPB) {
    const int m = pr / CG, cg = pr - m * CG;
    const int h = (cg * 8) / d;
    const unsigned* mk = mask + (h * M + m) * WPC;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int w = 0; w < WPC; ++w) {
      unsigned bits = mk[w];
      while (bits) {
        const int n = (w << 5) + __builtin_ctz(bits);
        bits &= bits - 1;
        const uint4 u = sq[n * CG + cg];
        const float g = sg[n];
        acc[0] += g * bf_lo(u.x); acc[1] += g * bf_hi(u.x); acc[2] += g * bf_lo(u.y); acc[3] += g * bf_hi(u.y);
        acc[4] += g * bf_lo(u.z); acc[5] += g * bf_hi(u.z); acc[6] += g * bf_lo(u.w); acc[7] += g * bf_hi(u.w);
      }
    }
    if (outp) {
      store8_f32(outp, (long long)m * C + cg * 8, acc);
    } else {
      crd_sum_t* dst = &dk[((long long)b * M + m) * C + cg * 8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (acc[j] != 0.f) grad_add(dst + j, acc[j]);
    }
  }
}

// k_attn_out_bwd<PRE> and the LDS path of k_attn_scores_bwd as ONE workgroup-local pass over the scores kernel's pixel chunks (grid
// (parts, B), parts = crd_attn_scores_bwd_partials): the score backward needs from the output backward only dS of its own pixels, a dot
// product over one pixel's channels, so g = scale * dS goes from phase 1 to phase 2 through LDS instead of a launch boundary and a
// round trip through memory.  The only grid-wide dependency of the pair, the rank-one vector path's need for the complete t, rides
// in the launch that folds the dK partials instead (k_attn_dk_fold).  No workgroup waits for another.
//   Phase 1 is k_attn_out_bwd's body on [p0, p1): the same lanes per pixel, per-element arithmetic and shuffle order, so dx1 and dS
// are the same bits; t and dbp_rows are summed over other chunks than there (fixed-point adds: still reproducible).  Loads are
// unconditional from clamped addresses, zeroed by selects.
//   Phase 2 is k_attn_scores_bwd's: dq from gathered k rows, q rows and mask bits into LDS, the owner-computes dK walk, plain stores
// of this chunk's partial copy.  The index and row loads of its first pass (the only one at chunks of <= 1024 granules) are
// requested BEFORE phase 1: they depend on nothing phase 1 computes, and the launch is two memory latencies deep instead of four.
struct ScoreBwd { const bf16_t* q; const bf16_t* k; const short* idx; int M, heads, d; float scale; bf16_t* dq; float* dk_part; };
template <int UB>
__device__ __forceinline__ void fused_load_index(const ScoreBwd& sb, int b, long long N, long long p0, int total, int i0,
                                                 int (&cgv)[UB], int (&mv)[UB], long long (&nv)[UB]) {
  const int CG = (sb.heads * sb.d) >> 3;
#pragma unroll
  for (int v = 0; v < UB; ++v) {
    const int i = i0 + v * TPB;                     // (int: a chunk has at most 32767 pixels of 64 granules)
    const int ic = i < total ? i : 0;               // (past the end: item 0, loaded and not used; no branch around the divisions)
    cgv[v] = ic % CG;
    nv[v] = p0 + ic / CG;
    mv[v] = sb.idx[((long long)b * N + nv[v]) * sb.heads + (cgv[v] * 8) / sb.d];
  }
}
template <int UB>
__device__ __forceinline__ void fused_load_rows(const ScoreBwd& sb, int b, long long N, const int (&cgv)[UB], const int (&mv)[UB],
                                                const long long (&nv)[UB], uint4 (&kraw)[UB], uint4 (&qraw)[UB]) {
  const int C = sb.heads * sb.d;
#pragma unroll
  for (int v = 0; v < UB; ++v) {
    kraw[v] = *reinterpret_cast<const uint4*>(sb.k + ((long long)b * sb.M + mv[v]) * C + cgv[v] * 8);
    qraw[v] = *reinterpret_cast<const uint4*>(sb.q + ((long long)b * N + nv[v]) * C + cgv[v] * 8);
  }
}
// dq = g * the gathered k rows; the q rows and one mask bit per (pixel, head) into LDS (k_attn_scores_bwd's pass with g from LDS)
template <int UB>
__device__ __forceinline__ void fused_scatter(const ScoreBwd& sb, int b, long long N, long long p0, int total, int i0,
                                              const int (&cgv)[UB], const int (&mv)[UB], const long long (&nv)[UB], const uint4 (&kraw)[UB],
                                              const uint4 (&qraw)[UB], uint4* sq, const float* sg, unsigned* mask, int WPC) {
  const int C = sb.heads * sb.d, CG = C >> 3;
#pragma unroll
  for (int v = 0; v < UB; ++v) {
    if (i0 + v * TPB >= total) continue;
    const int nl = (int)(nv[v] - p0);
    const float gv = sg[nl];
    float kv[8];
    kv[0] = bf_lo(kraw[v].x); kv[1] = bf_hi(kraw[v].x); kv[2] = bf_lo(kraw[v].y); kv[3] = bf_hi(kraw[v].y);
    kv[4] = bf_lo(kraw[v].z); kv[5] = bf_hi(kraw[v].z); kv[6] = bf_lo(kraw[v].w); kv[7] = bf_hi(kraw[v].w);
#pragma unroll
    for (int j = 0; j < 8; ++j) kv[j] *= gv;
    store8_bf16(sb.dq, ((long long)b * N + nv[v]) * C + cgv[v] * 8, kv);
    sq[nl * CG + cgv[v]] = make_uint4(qraw[v].x, qraw[v].y, qraw[v].z, qraw[v].w);      // (by element: the struct copy kept qraw in scratch)
    const int h = (cgv[v] * 8) / sb.d;
    // one bit per (pixel, head): integer LDS atomic, the result does not depend on the order
    if (cgv[v] * 8 == h * sb.d) atomicOr(&mask[(h * sb.M + mv[v]) * WPC + (nl >> 5)], 1u << (nl & 31));
  }
}
template <bool PRE>
__global__ __launch_bounds__(TPB) void k_attn_bwd_fused(float* dx1, const float* u, const float* S, const float* dp, long long N, int chunk,
                                                        crd_sum_t* t, crd_sum_t* dbp_rows, float* dS, GnPre pre, ScoreBwd sb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.y;
  const int M = sb.M, heads = sb.heads, d = sb.d;
  const int C = heads * d, CG = C >> 3;
  long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk;
  if (p1 > N) p1 = N;
  const int npx = (int)(p1 - p0);
  const int HM = heads * M, WPC = (chunk + 31) >> 5;                           // mask words per (head, key)
  uint4* sq = reinterpret_cast<uint4*>(smem);                                  // [chunk][CG]
  float* sg = reinterpret_cast<float*>(smem + (size_t)chunk * C * 2);          // [chunk]: g = scale * dS
  unsigned* mask = reinterpret_cast<unsigned*>(sg + chunk);                    // [HM][WPC]
  float* sm = reinterpret_cast<float*>(mask + HM * WPC);                       // [2][C]: the waves' t / dbp sums
  for (int i = threadIdx.x; i < HM * WPC; i += TPB) mask[i] = 0u;              // (published by the barriers of the wave fold below)
  // ---- phase 2, loads: UB items per thread and pass, the index scalars of all of them, then the dependent row gathers
  const int total = npx * CG;
  constexpr int UB = 4;
  int cgv[UB], mv[UB];
  long long nv[UB];
  uint4 kraw[UB], qraw[UB];
  fused_load_index<UB>(sb, b, N, p0, total, threadIdx.x, cgv, mv, nv);
  // ---- phase 1: k_attn_out_bwd on the chunk
  int W2 = 1;
  while (W2 < CG) W2 <<= 1;           // lanes per pixel (power of two, <= 64 since C <= 512)
  const int PPW = 64 / W2;            // pixels per wave-iteration
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = l / W2, cg = l % W2;
  const bool cok = cg < CG;
  const int cgc = cok ? cg : 0;
  const float dps = dp ? dp[b] : 1.f;
  float uu[8], ta[8], ba[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { uu[j] = u[(long long)b * C + cgc * 8 + j]; uu[j] = cok ? uu[j] : 0.f; ta[j] = ba[j] = 0.f; }
  float ga[8], mean = 0.f, rstd = 0.f, S1 = 0.f, S2 = 0.f;
  if (PRE) {
    if (b == 0 && pre.dgamma) {       // parameter gradients: the workgroups of sample 0 share the channels (as k_gn_bwd_apply)
      for (int c = blockIdx.x * TPB + threadIdx.x; c < C; c += gridDim.x * TPB) {
        const float ob = pre.dbeta[c], og = pre.dgamma[c];
        long long g0, g1;
        sum_samples(pre.r, pre.B, C, c, g0, g1);
        pre.dbeta[c] = ob + (float)g0 * (1.f / GRAD_ONE);
        pre.dgamma[c] = og + (float)g1 * (1.f / GRAD_ONE);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { ga[j] = pre.gamma[cgc * 8 + j]; ga[j] = cok ? ga[j] : 0.f; }
    if (cok) {
      const int grp = cg >> 1;                                    // 16-channel groups (gmul = 1)
      const float inv_m = 1.f / ((float)N * 16.f);
      const crd_sum_t* rg = pre.r + (long long)pre.B * C * 2 + ((long long)b * (C >> 4) + grp) * 2;
      S1 = grad_get(rg) * inv_m; S2 = grad_get(rg + 1) * inv_m;
      gn_mean_rstd(pre.stats + (long long)b * (C >> 4) * 2, grp, 1, (float)N * 16.f, mean, rstd);
    }
  }
  fused_load_rows<UB>(sb, b, N, cgv, mv, nv, kraw, qraw);
  constexpr int UN = 4;
  for (long long nb = p0 + wave * PPW; nb < p1; nb += (long long)UN * 4 * PPW) {
    float v[UN][8], s[UN];
    float xv[PRE ? UN : 1][8], dv[PRE ? UN : 1][8];
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const long long n = nb + (long long)k * 4 * PPW + sub;
      const bool ok = cok && n < p1;
      const long long nc = n < p1 ? n : p1 - 1;
      const long long off = ((long long)b * N + nc) * C + cgc * 8;
      load8(dx1, off, 1, v[k]);
      s[k] = S[(long long)b * N + nc];
      if (PRE) { load8(pre.x, off, 1, xv[PRE ? k : 0]); load8(pre.dxn, off, 0, dv[PRE ? k : 0]); }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = ok ? v[k][j] : 0.f;
      s[k] = ok ? s[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const long long n = nb + (long long)k * 4 * PPW + sub;
      if (PRE && cok && n < p1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (xv[PRE ? k : 0][j] - mean) * rstd;
          float o = (ga[j] * dv[PRE ? k : 0][j] - S1 - xh * S2) * rstd;
          o += v[k][j];
          v[k][j] = o;
        }
        store8_f32(dx1, ((long long)b * N + n) * C + cg * 8, v[k]);
      }
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[k][j] *= dps; dot += v[k][j] * uu[j]; ta[j] += v[k][j] * s[k]; ba[j] += v[k][j]; }
      for (int o = W2 >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
      if (cok && n < p1 && cg == 0) {
        sg[n - p0] = sb.scale * dot;
        if (dS) dS[(long long)b * N + n] = dot;
      }
    }
  }
  for (int o = W2; o < 64; o <<= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { ta[j] += __shfl_xor(ta[j], o); ba[j] += __shfl_xor(ba[j], o); }
  }
  for (int w = 0; w < 4; ++w) {
    if (wave == w && sub == 0 && cok) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float* p0_ = &sm[cg * 8 + j];
        float* p1_ = &sm[C + cg * 8 + j];
        *p0_ = w == 0 ? ta[j] : *p0_ + ta[j];
        *p1_ = w == 0 ? ba[j] : *p1_ + ba[j];
      }
    }
    __syncthreads();                  // (the last one also publishes sg and the zeroed masks to phase 2)
  }
  for (int i = threadIdx.x; i < C; i += TPB) {
    grad_add(&t[(long long)b * C + i], sm[i]);
    grad_add(&dbp_rows[(long long)b * C + i], sm[C + i]);
  }
  // ---- phase 2: k_attn_scores_bwd's LDS path with g from LDS; the first pass consumes the rows requested at the top
  fused_scatter<UB>(sb, b, N, p0, total, threadIdx.x, cgv, mv, nv, kraw, qraw, sq, sg, mask, WPC);
  for (int i0 = threadIdx.x + UB * TPB; i0 < total; i0 += UB * TPB) {      // chunks of more than 1024 granules
    int cg2[UB], m2[UB];
    long long n2[UB];
    uint4 k2[UB], q2[UB];
    fused_load_index<UB>(sb, b, N, p0, total, i0, cg2, m2, n2);
    fused_load_rows<UB>(sb, b, N, cg2, m2, n2, k2, q2);
    fused_scatter<UB>(sb, b, N, p0, total, i0, cg2, m2, n2, k2, q2, sq, sg, mask, WPC);
  }
  __syncthreads();
  // the owner of (key m, granule cg) walks the set bits of the key's mask in ascending pixel order (as k_attn_scores_bwd)
  float* outp = sb.dk_part + ((long long)blockIdx.x * gridDim.y + b) * M * C;
  for (int pr = threadIdx.x; pr < M * CG; pr += TPB) {
    const int m = pr / CG, cgo = pr - m * CG;
    const int h = (cgo * 8) / d;
    const unsigned* mk = mask + (h * M + m) * WPC;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int w = 0; w < WPC; ++w) {
      unsigned bits = mk[w];
      while (bits) {
        const int n = (w << 5) + __builtin_ctz(bits);
        bits &= bits - 1;
        const uint4 q8 = sq[n * CG + cgo];
        const float g = sg[n];
        acc[0] += g * bf_lo(q8.x); acc[1] += g * bf_hi(q8.x); acc[2] += g * bf_lo(q8.y); acc[3] += g * bf_hi(q8.y);
        acc[4] += g * bf_lo(q8.z); acc[5] += g * bf_hi(q8.z); acc[6] += g * bf_lo(q8.w); acc[7] += g * bf_hi(q8.w);
      }
    }
    store8_f32(outp, (long long)m * C + cgo * 8, acc);
  }
}

// dst[i] = bf16(sum_r part[r*stride + i]), 8 elements per thread
// (workgroup blk of nblk: k_attn_dk_fold runs the same fold behind its rider workgroups)
__device__ __forceinline__ void sum_partials_body(const float* part, int replicas, long long stride, bf16_t* dst, long long n8, int blk,
                                                  int nblk) {
  for (long long i = (long long)blk * TPB + threadIdx.x; i < n8; i += (long long)nblk * TPB) {
    // the copies four at a time, all loads of a pass in flight (clamped index, select past the end; still added in index
    // order): one copy per iteration was one dependent memory latency per copy -- 52 of them at stage 1
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    for (int r0 = 0; r0 < replicas; r0 += 4) {
      float w[4][8];
#pragma unroll
      for (int k = 0; k < 4; ++k) load8(part, (long long)(r0 + k < replicas ? r0 + k : replicas - 1) * stride + i * 8, 1, w[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = r0 + k < replicas;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += ok ? w[k][j] : 0.f;
      }
    }
    store8_bf16(dst, i * 8, v);
  }
}
__global__ __launch_bounds__(TPB) void k_sum_partials_bf16(const float* part, int replicas, long long stride, bf16_t* dst, long long n8) {
  sum_partials_body(part, replicas, stride, dst, n8, blockIdx.x, gridDim.x);
}
// The fold of k_attn_bwd_fused's dK partials with the rank-one vector path as riders: the first B * cdiv(C, FOLD_VEC_ROWS) workgroups
// run attn_vec_bwd_body (sample-major), the rest are k_sum_partials_bf16's.  t is complete when this launch starts (it sits behind the
// launch that adds it up), and tb / es are first read behind it.  A rider owns 16 rows, one batch of four per wave, requested before t
// is read: with VEC_ROWS rows (four dependent batches) the riders ended the launch 3 us behind the fold workgroups.
constexpr int FOLD_VEC_ROWS = 16;
__global__ __launch_bounds__(TPB) void k_attn_dk_fold(const float* part, int replicas, long long stride, bf16_t* dst, long long n8, int B,
                                                      VecBwd vec) {
  const int nv = (vec.C + FOLD_VEC_ROWS - 1) / FOLD_VEC_ROWS, nrider = B * nv;
  if ((int)blockIdx.x < nrider) { attn_vec_bwd_body(vec, blockIdx.x / nv, blockIdx.x % nv, FOLD_VEC_ROWS); return; }
  sum_partials_body(part, replicas, stride, dst, n8, blockIdx.x - nrider, gridDim.x - nrider);
}

// dst[i] = bf16(value of the fixed-point gradient sum src[i]), 8 elements per thread
__global__ __launch_bounds__(TPB) void k_gsum_to_bf16(const crd_sum_t* src, bf16_t* dst, long long n8) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n8; i += (long long)gridDim.x * TPB) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = grad_get(src + i * 8 + j);
    store8_bf16(dst, i * 8, v);
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

static int attn_scores_launch(const void* q, const void* k, int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d, float scale,
                              float* S, int16_t* idx, const XbarProj& xp, const char* who, crd_stream_t stream) {
  CRD_CHECK_ARG(q && k && S && idx, "%s: null pointer", who);
  CRD_UNSUPPORTED(d % 8 == 0 && d <= 64 && M < 32768, "%s: head dim must be a multiple of 8, <= 64 (got %d)", who, d);
  CRD_UNSUPPORTED(heads >= 1 && heads <= 16, "%s: at most 16 heads (got %d)", who, heads);
  int qg = 8 / heads;                      // query groups per workgroup: ~8 waves, at most 16
  if (qg < 1) qg = 1;
  if (qg > 4) qg = 4;
  dim3 grid(cdiv(N, 32 * qg) + (xp.chan ? cdiv(xp.C, VEC_ROWS) : 0), B);
  hipLaunchKernelGGL(k_attn_scores, grid, dim3(64 * heads * qg), 0, as_stream(stream), reinterpret_cast<const bf16_t*>(q),
                     reinterpret_cast<const bf16_t*>(k), N, M, heads, d, scale, S, idx, qg, xp);
  CRD_LAUNCH_CHECK(who);
  return CRD_OK;
}

extern "C" int crd_attn_scores(const void* q, const void* k, int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d,
                               float scale, float* S, int16_t* idx, crd_stream_t stream) {
  return attn_scores_launch(q, k, B, N, M, heads, d, scale, S, idx, XbarProj{}, "crd_attn_scores", stream);
}

extern "C" int crd_attn_scores_fp8(const void* q8, const void* k8, int32_t B, int32_t N, int32_t M, int32_t heads, float qk_scale,
                                   float scale, float* ssum, int16_t* idx, crd_stream_t stream) {
  CRD_CHECK_ARG(q8 && k8 && ssum && idx && B > 0 && N > 0 && M > 0 && qk_scale > 0.f, "crd_attn_scores_fp8: bad argument");
  CRD_UNSUPPORTED(heads >= 1 && heads <= 16, "crd_attn_scores_fp8: at most 16 heads");
  CRD_CHECK_ARG((reinterpret_cast<uintptr_t>(q8) & 15) == 0 && (reinterpret_cast<uintptr_t>(k8) & 15) == 0, "crd_attn_scores_fp8: 16-byte aligned operands");
  int qg = 8 / heads;                                    // query groups per workgroup: the bf16 kernel's rule (the comparison is like for like)
  if (qg < 1) qg = 1;
  if (qg > 4) qg = 4;
  hipLaunchKernelGGL(k_attn_scores_fp8, dim3(cdiv(N, 32 * qg), B), dim3(64 * heads * qg), 0, as_stream(stream),
                     reinterpret_cast<const unsigned char*>(q8), reinterpret_cast<const unsigned char*>(k8), N, M, heads, qk_scale, scale, ssum,
                     reinterpret_cast<short*>(idx), qg);
  CRD_LAUNCH_CHECK("crd_attn_scores_fp8");
  return CRD_OK;
}

extern "C" int crd_attn_fwd(const void* q, const void* k, int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d, float scale,
                            float* S, int16_t* idx, const crd_sum_t* chan_sums, const crd_sum_t* stats, const float* gamma,
                            const float* beta, const void* w_fwd, void* xbar, float* u, crd_stream_t stream) {
  CRD_CHECK_ARG(chan_sums && stats && gamma && beta && w_fwd && xbar && u, "crd_attn_fwd: null pointer");
  const int C = heads * d;
  CRD_UNSUPPORTED(C % 16 == 0 && C <= 1024, "crd_attn_fwd: C must be a multiple of 16, <= 1024");
  return attn_scores_launch(q, k, B, N, M, heads, d, scale, S, idx,
                            XbarProj{chan_sums, stats, gamma, beta, reinterpret_cast<const bf16_t*>(w_fwd), N, C,
                                     reinterpret_cast<bf16_t*>(xbar), u}, "crd_attn_fwd", stream);
}

extern "C" int crd_attn_xbar(const crd_sum_t* chan_sums, const crd_sum_t* stats, const float* gamma, const float* beta, int32_t B,
                             int32_t N, int32_t C, void* xbar, crd_stream_t stream) {
  CRD_CHECK_ARG(chan_sums && stats && gamma && beta && xbar, "crd_attn_xbar: null pointer");
  hipLaunchKernelGGL(k_attn_xbar, dim3(B), dim3(256), 0, as_stream(stream), chan_sums, stats, gamma, beta, N, C,
                     reinterpret_cast<bf16_t*>(xbar));
  CRD_LAUNCH_CHECK("crd_attn_xbar");
  return CRD_OK;
}

extern "C" int crd_attn_xbar_proj(const crd_sum_t* chan_sums, const crd_sum_t* stats, const float* gamma, const float* beta, const void* w_fwd,
                                  int32_t B, int32_t N, int32_t C, void* xbar, float* u, crd_stream_t stream) {
  CRD_CHECK_ARG(chan_sums && stats && gamma && beta && w_fwd && xbar && u, "crd_attn_xbar_proj: null pointer");
  CRD_UNSUPPORTED(C % 16 == 0 && C <= 1024, "crd_attn_xbar_proj: C must be a multiple of 16, <= 1024");
  hipLaunchKernelGGL(k_attn_xbar_proj, dim3(cdiv(C, VEC_ROWS), B), dim3(TPB), 0, as_stream(stream),
                     XbarProj{chan_sums, stats, gamma, beta, reinterpret_cast<const bf16_t*>(w_fwd), N, C, reinterpret_cast<bf16_t*>(xbar), u});
  CRD_LAUNCH_CHECK("crd_attn_xbar_proj");
  return CRD_OK;
}

extern "C" int crd_attn_vec_bwd(const crd_sum_t* t, const void* w_dgrad, int32_t B, int32_t C, int32_t Cpad, float inv_n, void* tb, float* es,
                                crd_stream_t stream) {
  CRD_CHECK_ARG(t && w_dgrad && tb && es, "crd_attn_vec_bwd: null pointer");
  CRD_UNSUPPORTED(C % 8 == 0 && C <= 1024 && Cpad >= C && Cpad % 8 == 0, "crd_attn_vec_bwd: C must be a multiple of 8, <= 1024");
  hipLaunchKernelGGL(k_attn_vec_bwd, dim3(cdiv(C, VEC_ROWS), B), dim3(TPB), 0, as_stream(stream),
                     VecBwd{t, reinterpret_cast<const bf16_t*>(w_dgrad), C, Cpad, inv_n, reinterpret_cast<bf16_t*>(tb), es});
  CRD_LAUNCH_CHECK("crd_attn_vec_bwd");
  return CRD_OK;
}

extern "C" int crd_attn_out_residual(const float* x, const float* u, const float* S, const float* bp, const float* dp,
                                     int32_t B, int32_t N, int32_t C, float* x1, crd_stream_t stream) {
  CRD_CHECK_ARG(x && u && S && bp && x1, "crd_attn_out_residual: null pointer");
  CRD_CHECK_ARG(C % 8 == 0, "crd_attn_out_residual: C %% 8");
  const long long total = (long long)N * (C / 8);
  int nblk = cdiv(total, TPB);
  if (nblk > 2048) nblk = 2048;
  hipLaunchKernelGGL(k_attn_out_residual, dim3(nblk, B), dim3(TPB), 0, as_stream(stream), x, u, S, bp, dp, (long long)N, C, x1);
  CRD_LAUNCH_CHECK("crd_attn_out_residual");
  return CRD_OK;
}

// workgroups per sample of k_attn_out_bwd: 256 pixels each, fewer on small grids, at most 1024 workgroups per launch
static int attn_out_bwd_blocks(int B, int N) {
  static int small = -1;
  if (small < 0) small = crd_dev_int("CRD_ATTN_OUT_BWD_CHUNK", 32);
  int nblk = cdiv(N, (long long)B * cdiv(N, 256) < 128 ? small : 256);     // fewer pixels per workgroup on small grids
  int cap = 1024 / (B > 0 ? B : 1); if (cap < 1) cap = 1;
  if (nblk > cap) nblk = cap;
  const int chunk = cdiv(N, nblk);
  return cdiv(N, chunk);
}

extern "C" int crd_attn_out_bwd_blocks(int32_t B, int32_t N, int32_t C) {
  (void)C;                                 // the rule does not depend on the channel count (the lanes per pixel do, inside the kernel)
  return B > 0 && N > 0 ? attn_out_bwd_blocks(B, N) : 0;
}

static int attn_out_bwd_launch(float* dx1, const float* u, const float* S, const float* dp, int32_t B, int32_t N, int32_t C, crd_sum_t* t,
                               crd_sum_t* dbp_rows, float* dS, const GnPre* pre, const char* who, crd_stream_t stream) {
  CRD_CHECK_ARG(dx1 && u && S && t && dbp_rows && dS, "%s: null pointer", who);
  CRD_UNSUPPORTED(C % 8 == 0 && C <= 512, "%s: C must be a multiple of 8 and <= 512", who);
  const int nblk = attn_out_bwd_blocks(B, N);
  const int chunk = cdiv(N, nblk);
  if (pre) hipLaunchKernelGGL(k_attn_out_bwd<true>, dim3(nblk, B), dim3(TPB), 2 * C * sizeof(float), as_stream(stream), dx1, u, S, dp,
                              (long long)N, C, chunk, t, dbp_rows, dS, *pre);
  else hipLaunchKernelGGL(k_attn_out_bwd<false>, dim3(nblk, B), dim3(TPB), 2 * C * sizeof(float), as_stream(stream), dx1, u, S, dp,
                          (long long)N, C, chunk, t, dbp_rows, dS, GnPre{});
  CRD_LAUNCH_CHECK(who);
  return CRD_OK;
}

extern "C" int crd_attn_out_bwd(const float* dx1, const float* u, const float* S, const float* dp, int32_t B, int32_t N,
                                int32_t C, crd_sum_t* t, crd_sum_t* dbp_rows, float* dS, crd_stream_t stream) {
  return attn_out_bwd_launch(const_cast<float*>(dx1), u, S, dp, B, N, C, t, dbp_rows, dS, nullptr, "crd_attn_out_bwd", stream);
}

extern "C" int crd_attn_out_bwd_gn(float* dx1, const float* u, const float* S, const float* dp, int32_t B, int32_t N, int32_t C,
                                   crd_sum_t* t, crd_sum_t* dbp_rows, float* dS, const float* x, const void* dxn, const crd_sum_t* stats,
                                   const float* gamma, const crd_sum_t* r, float* dgamma, float* dbeta, crd_stream_t stream) {
  CRD_CHECK_ARG(x && dxn && stats && gamma && r, "crd_attn_out_bwd_gn: null pointer");
  CRD_CHECK_ARG(C % 16 == 0 && (dgamma == nullptr) == (dbeta == nullptr), "crd_attn_out_bwd_gn: C %% 16, dgamma / dbeta both or neither");
  const GnPre pre{x, reinterpret_cast<const bf16_t*>(dxn), stats, gamma, r, dgamma, dbeta, B};
  return attn_out_bwd_launch(dx1, u, S, dp, B, N, C, t, dbp_rows, dS, &pre, "crd_attn_out_bwd_gn", stream);
}

// LDS of the chunked path: q rows + g + one pixel bitmask per (head, key) of a `chunk`-pixel chunk
static size_t attn_bwd_lds(int chunk, int M, int heads, int C) {
  return (size_t)chunk * C * 2 + (size_t)chunk * 4 + (size_t)heads * M * ((chunk + 31) / 32) * 4 + 16;
}
// workgroups per sample of the chunked (LDS) path; 0: a chunk does not fit in LDS, the global-atomics path runs
static int attn_bwd_blocks(int B, int N, int M, int heads, int C) {
  // pixels per workgroup: 128; 32 (N <= 512) or 64 on grids that would leave most CUs without a workgroup (N = 104 / 416 /
  // 1664 per sample gave 8 / 32 / 104 workgroups): 24.87 -> 24.53 ms per step, the extra partial copies included
  static int small = -1, mid = -1;
  if (small < 0) {
    small = crd_dev_int("CRD_ATTN_BWD_CHUNK", 32);
    mid = crd_dev_int("CRD_ATTN_BWD_CHUNK2", 64);
  }
  int target = 128;
  if ((long long)B * cdiv(N, 128) < 128) target = N <= 512 ? small : mid;
  int nblk = cdiv(N, target);
  int cap = 2048 / (B > 0 ? B : 1); if (cap < 1) cap = 1;
  if (nblk > cap) nblk = cap;
  const int chunk = cdiv(N, nblk);
  if (attn_bwd_lds(chunk, M, heads, C) > 128 * 1024 || chunk > 32767) return 0;
  return cdiv(N, chunk);
}

extern "C" int crd_attn_scores_bwd_partials(int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d) {
  return attn_bwd_blocks(B, N, M, heads, heads * d);
}

static int attn_scores_bwd_launch(const void* q, const void* k, const float* dS, const int16_t* idx, int32_t B, int32_t N,
                                  int32_t M, int32_t heads, int32_t d, float scale, void* dq, crd_sum_t* dk, float* dk_partials,
                                  const VecBwd& vec, const char* who, crd_stream_t stream) {
  CRD_CHECK_ARG(q && k && dS && idx && dq && (dk || dk_partials), "%s: null pointer", who);
  CRD_CHECK_ARG(d % 8 == 0, "%s: head dim must be a multiple of 8", who);
  const int C = heads * d;
  // the chunked path (q rows of <= 128 pixels staged in LDS, counting sort by key, owner-computes dK) runs whenever the
  // chunk fits; the fallback adds every contribution to global memory with an atomic of its own
  int nblk = attn_bwd_blocks(B, N, M, heads, C);
  const int use_lds = nblk > 0;
  CRD_CHECK_ARG(use_lds ? (dk_partials || dk) : dk != nullptr, "%s: this shape needs the dk accumulator", who);
  crd_reserve_lds_once<&k_attn_scores_bwd>(128 * 1024, "k_attn_scores_bwd");
  if (!use_lds) {
    nblk = cdiv(N, 64);
    int cap = 2048 / (B > 0 ? B : 1); if (cap < 1) cap = 1;
    if (nblk > cap) nblk = cap;
  }
  int chunk = cdiv(N, nblk);
  nblk = cdiv(N, chunk);
  const size_t lds = attn_bwd_lds(chunk, M, heads, C);
  hipLaunchKernelGGL(k_attn_scores_bwd, dim3(nblk + (vec.t ? cdiv(vec.C, VEC_ROWS) : 0), B), dim3(TPB), use_lds ? lds : 0, as_stream(stream),
                     reinterpret_cast<const bf16_t*>(q), reinterpret_cast<const bf16_t*>(k), dS, reinterpret_cast<const short*>(idx),
                     (long long)N, M, heads, d, scale, chunk, reinterpret_cast<bf16_t*>(dq), dk, use_lds,
                     use_lds ? dk_partials : nullptr, vec);
  CRD_LAUNCH_CHECK(who);
  return CRD_OK;
}

extern "C" int crd_attn_scores_bwd(const void* q, const void* k, const float* dS, const int16_t* idx, int32_t B, int32_t N,
                                   int32_t M, int32_t heads, int32_t d, float scale, void* dq, crd_sum_t* dk, float* dk_partials,
                                   crd_stream_t stream) {
  return attn_scores_bwd_launch(q, k, dS, idx, B, N, M, heads, d, scale, dq, dk, dk_partials, VecBwd{}, "crd_attn_scores_bwd", stream);
}

extern "C" int crd_attn_bwd(const void* q, const void* k, const float* dS, const int16_t* idx, int32_t B, int32_t N, int32_t M,
                            int32_t heads, int32_t d, float scale, void* dq, crd_sum_t* dk, float* dk_partials, const crd_sum_t* t,
                            const void* w_dgrad, int32_t Cpad, float inv_n, void* tb, float* es, crd_stream_t stream) {
  CRD_CHECK_ARG(t && w_dgrad && tb && es, "crd_attn_bwd: null pointer");
  const int C = heads * d;
  CRD_UNSUPPORTED(C <= 1024 && Cpad >= C && Cpad % 8 == 0, "crd_attn_bwd: C must be <= 1024");
  return attn_scores_bwd_launch(q, k, dS, idx, B, N, M, heads, d, scale, dq, dk, dk_partials,
                                VecBwd{t, reinterpret_cast<const bf16_t*>(w_dgrad), C, Cpad, inv_n, reinterpret_cast<bf16_t*>(tb), es},
                                "crd_attn_bwd", stream);
}

extern "C" int crd_sum_partials_bf16(const float* part, int32_t replicas, int64_t replica_stride, void* dst, int64_t n,
                                     crd_stream_t stream) {
  CRD_CHECK_ARG(part && dst && replicas >= 1 && n > 0 && n % 8 == 0 && replica_stride % 8 == 0, "crd_sum_partials_bf16: bad argument");
  long long nb = (n / 8 + TPB - 1) / TPB;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_sum_partials_bf16, dim3((unsigned)nb), dim3(TPB), 0, as_stream(stream), part, replicas, (long long)replica_stride,
                     reinterpret_cast<bf16_t*>(dst), (long long)(n / 8));
  CRD_LAUNCH_CHECK("crd_sum_partials_bf16");
  return CRD_OK;
}

// LDS of k_attn_bwd_fused: the chunked score path's plus the [2][C] sums of the output backward
static size_t attn_bwd_fused_lds(int chunk, int M, int heads, int C) { return attn_bwd_lds(chunk, M, heads, C) + 2 * (size_t)C * sizeof(float); }
// workgroups per sample of k_attn_bwd_fused = the score backward's chunk rule; 0: this shape stays on the separate launches
static int attn_bwd_fused_blocks(int B, int N, int M, int heads, int C) {
  if (B < 1 || N < 1 || M < 1 || heads < 1 || C < 8 || C % 8 || C > 512) return 0;
  const int nblk = attn_bwd_blocks(B, N, M, heads, C);
  if (nblk == 0 || attn_bwd_fused_lds(cdiv(N, nblk), M, heads, C) > 128 * 1024) return 0;
  return nblk;
}

extern "C" int crd_attn_bwd_fused_supported(int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d) {
  return d > 0 && d % 8 == 0 && heads > 0 ? attn_bwd_fused_blocks(B, N, M, heads, heads * d) : 0;
}

extern "C" int crd_attn_bwd_fused(float* dx1, const float* u, const float* S, const float* dp, const void* q, const void* k, const int16_t* idx,
                                  int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d, float scale, crd_sum_t* t, crd_sum_t* dbp_rows,
                                  float* dS, void* dq, float* dk_partials, const float* x, const void* dxn, const crd_sum_t* stats,
                                  const float* gamma, const crd_sum_t* r, float* dgamma, float* dbeta, crd_stream_t stream) {
  CRD_CHECK_ARG(dx1 && u && S && q && k && idx && t && dbp_rows && dq && dk_partials, "crd_attn_bwd_fused: null pointer");
  CRD_CHECK_ARG(B > 0 && N > 0 && M > 0 && heads > 0, "crd_attn_bwd_fused: B, N, M and heads must be positive");
  CRD_CHECK_ARG(d > 0 && d % 8 == 0, "crd_attn_bwd_fused: head dim must be a multiple of 8");
  const bool pre = x || dxn || stats || gamma || r || dgamma || dbeta;
  const int C = heads * d;
  CRD_UNSUPPORTED(C <= 512, "crd_attn_bwd_fused: C = %d must be <= 512", C);
  if (pre) {
    CRD_CHECK_ARG(x && dxn && stats && gamma && r, "crd_attn_bwd_fused: null pointer (GroupNorm backward)");
    CRD_CHECK_ARG(C % 16 == 0 && (dgamma == nullptr) == (dbeta == nullptr), "crd_attn_bwd_fused: C %% 16, dgamma / dbeta both or neither");
  }
  const int nblk = attn_bwd_fused_blocks(B, N, M, heads, C);
  CRD_UNSUPPORTED(nblk > 0, "crd_attn_bwd_fused: a pixel chunk (q rows, g, masks, 2 * C channel sums) does not fit in LDS "
                            "(crd_attn_bwd_fused_supported = 0)");
  const int chunk = cdiv(N, nblk);
  const size_t lds = attn_bwd_fused_lds(chunk, M, heads, C);
  const ScoreBwd sb{reinterpret_cast<const bf16_t*>(q), reinterpret_cast<const bf16_t*>(k), reinterpret_cast<const short*>(idx), M, heads, d,
                    scale, reinterpret_cast<bf16_t*>(dq), dk_partials};
  if (pre) {
    crd_reserve_lds_once<&k_attn_bwd_fused<true>>(128 * 1024, "k_attn_bwd_fused<true>");
    hipLaunchKernelGGL(k_attn_bwd_fused<true>, dim3(nblk, B), dim3(TPB), lds, as_stream(stream), dx1, u, S, dp, (long long)N, chunk, t,
                       dbp_rows, dS, GnPre{x, reinterpret_cast<const bf16_t*>(dxn), stats, gamma, r, dgamma, dbeta, B}, sb);
  } else {
    crd_reserve_lds_once<&k_attn_bwd_fused<false>>(128 * 1024, "k_attn_bwd_fused<false>");
    hipLaunchKernelGGL(k_attn_bwd_fused<false>, dim3(nblk, B), dim3(TPB), lds, as_stream(stream), dx1, u, S, dp, (long long)N, chunk, t,
                       dbp_rows, dS, GnPre{}, sb);
  }
  CRD_LAUNCH_CHECK("crd_attn_bwd_fused");
  return CRD_OK;
}

extern "C" int crd_attn_dk_fold(const float* part, int32_t replicas, int64_t replica_stride, void* dst, int64_t n, const crd_sum_t* t,
                                const void* w_dgrad, int32_t B, int32_t C, int32_t Cpad, float inv_n, void* tb, float* es, crd_stream_t stream) {
  CRD_CHECK_ARG(part && dst && replicas >= 1 && n > 0 && n % 8 == 0 && replica_stride % 8 == 0, "crd_attn_dk_fold: bad argument");
  CRD_CHECK_ARG(t && w_dgrad && tb && es && B > 0, "crd_attn_dk_fold: null pointer");
  CRD_UNSUPPORTED(C > 0 && C % 8 == 0 && C <= 1024 && Cpad >= C && Cpad % 8 == 0, "crd_attn_dk_fold: C must be a multiple of 8, <= 1024");
  long long nb = (n / 8 + TPB - 1) / TPB;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_attn_dk_fold, dim3((unsigned)(nb + (long long)B * cdiv(C, FOLD_VEC_ROWS))), dim3(TPB), 0, as_stream(stream), part, replicas,
                     (long long)replica_stride, reinterpret_cast<bf16_t*>(dst), (long long)(n / 8), B,
                     VecBwd{t, reinterpret_cast<const bf16_t*>(w_dgrad), C, Cpad, inv_n, reinterpret_cast<bf16_t*>(tb), es});
  CRD_LAUNCH_CHECK("crd_attn_dk_fold");
  return CRD_OK;
}

extern "C" int crd_gsum_to_bf16(const crd_sum_t* src, void* dst, int64_t n, crd_stream_t stream) {
  CRD_CHECK_ARG(src && dst && n > 0 && n % 8 == 0, "crd_gsum_to_bf16: bad argument");
  long long nb = (n / 8 + TPB - 1) / TPB;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_gsum_to_bf16, dim3((unsigned)nb), dim3(TPB), 0, as_stream(stream), src, reinterpret_cast<bf16_t*>(dst),
                     (long long)(n / 8));
  CRD_LAUNCH_CHECK("crd_gsum_to_bf16");
  return CRD_OK;
}
