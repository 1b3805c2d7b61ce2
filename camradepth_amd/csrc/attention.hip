// The max-pool attention of the Simplified Transformer's encoder Blocks for gfx950: fused QK^T + scale + row-max on MFMA, rank-1
// output, backward.
// The head of the attention backward exists in two forms: k_attn_out_bwd + k_attn_scores_bwd + k_sum_partials_bf16 (three launches,
// dS through memory, the rank-one vector path riding in the second; also the fallback for shapes whose masks do not fit in LDS), and
// k_attn_bwd_fused + k_attn_dk_fold (two launches: output and score backward as one workgroup-local pass per pixel chunk, dS through
// LDS, the vector path riding in the fold).  dx1, dS, dq and the dK partials are the same bits in both.  The index / row / scatter
// pass of the score backward is one set of functions (load_index, load_rows, scatter) for both forms; the output backward and the
// owner-computes dK walk are written out in k_attn_bwd_fused as well as in the separate kernels, on purpose: behind any function
// boundary the compiler scheduled the fused kernel differently, and the step was 0.04 ms slower ("One file for the attention").
#include <stdlib.h>
#include "common.h"

namespace {

constexpr int TPB = 256;

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
  auto load4 = [&](int r0, int c0, float (&wv)[4][8]) {
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
  load4(r_first < r_hi ? r_first : r_lo, l * 8, w0);
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
        load4(r0, c0, wv);
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
// What follows the MFMAs of a 32-key tile, in both score kernels: acc[r] is this lane's query against key m0 + (r & 3) + 8 * (r >> 2) +
// 4 * half; the running maximum and its key are updated with bf16(bf16(acc * pre) * scale).  pre is the fp8 kernel's operand scale (the
// bf16 kernel passes none: the multiply by the constant 1 folds away).
// The kernels are bound by THIS: the two bf16 roundings, the scale, compare and two selects per score are vector instructions
// (4 clocks each per wave), the MFMAs a quarter of that.  Roundings in pairs through v_cvt_pk_bf16_f32 (one instruction per
// two values + one shift / mask each to widen again, instead of three integer operations per value); selects only -- as
// `if (m < M && v > best)` this compiled to two exec-mask branches per key; the `m < M` select only in a tile that crosses M.
__device__ __forceinline__ void argmax_tile(const f32x16& acc, int m0, int half, int M, float scale, float& best, int& besti, float pre = 1.f) {
  const bool edge = m0 + 32 > M;                                    // wave-uniform
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int ma = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;          // r even: the pair is keys ma, ma + 1
    const uint32_t p1 = pack_bf2(acc[r] * pre, acc[r + 1] * pre);
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
}
// The end of both score kernels (wave w -> head w % heads, query group w / heads; lane -> query n, half-wave `half` of its keys): the
// two half-waves meet, idx is stored, and the heads' maxima of a query group meet in the kernel's smax.  (The lane's coordinates by
// reference to the kernel's own: passed by value k_attn_scores no longer compiled to the instruction stream it was tuned as.  After
// a change to this signature or its call sites, regenerate profiles/resources_attention_split.txt and compare.)
__device__ __forceinline__ void scores_finish(float best, int besti, const int& b, const int& N, const int& n, const bool& nok, const int& heads,
                                              const int& h, const int& g, const int& half, const int& wave, const int& l, float* S, short* idx) {
  __shared__ float smax[16][32];
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

// One wave = 32 queries x ONE head (blockDim = 64 * heads * qg: wave w -> head w % heads, query group w / heads), so the
// per-head chain of dependent loads runs in parallel across the waves instead of serially inside one (stage 4: 8 heads);
// the heads' maxima of a query group meet in LDS.
__global__ __launch_bounds__(1024) void k_attn_scores(const bf16_t* q, const bf16_t* k, int N, int M, int heads, int d,
                                                      float scale, float* S, short* idx, int qg, XbarProj xp) {
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
    argmax_tile(acc, m0, half, M, scale, best, besti);
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
  scores_finish(best, besti, b, N, n, nok, heads, h, g, half, wave, l, S, idx);
}

// ------------------------------------------------------------------------------------------------
// Config 5 experiment (round 6, BASELINE.json configs[4] "fp8 MFMA attention"): the same scores with e4m3 operands --
// s[n] = max_m bf16(bf16(qs ks (q8_n . k8_m)) * scale) -- on v_mfma_scale_f32_32x32x64_f8f6f4 (block scales 2^0): ONE K = 64 MFMA per
// 32-key tile instead of four bf16 ones, half the operand bytes.  q8 / k8: per-tensor-scaled e4m3 copies, rows [heads][64] bytes (the
// head dimension zero-padded to 64: two 16-byte granules per lane and no masking).  Everything behind the MFMA -- roundings, compare,
// arg-max selects, the head sum -- is the bf16 kernel's (argmax_tile, scores_finish).  Measured and NOT wired into the plan: see DESIGN.md "Round 6".
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_attn_scores_fp8(const unsigned char* q8, const unsigned char* k8, int N, int M, int heads,
                                                          float qk_scale, float scale, float* S, short* idx, int qg) {
  typedef __attribute__((ext_vector_type(8))) int i32x8;
  typedef __attribute__((ext_vector_type(4))) int i32x4;
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
    argmax_tile(acc, m0, half, M, scale, best, besti, qk_scale);
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
  scores_finish(best, besti, b, N, n, nok, heads, h, g, half, wave, l, S, idx);
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
// The chunked form works on one workgroup's pixel chunk [p0, p0 + npx) in LDS: the q rows sq [chunk][CG] (16-byte granules),
// g = scale * dS in sg [chunk], and per (head, key) a BITMASK over the chunk's pixels, mask [heads * M][WPC]: bit n set <=> pixel n's
// arg-max for that head is this key.  An item is (pixel, granule); a thread takes UB items per pass: first the index scalars of all
// of them (load_index), then the dependent row gathers (load_rows), so that a pass costs two memory latencies instead of two per
// item; scatter consumes them.  k_attn_scores_bwd fills sg from dS, k_attn_bwd_fused from its first phase.
struct ScoreBwd { const bf16_t* q; const bf16_t* k; const short* idx; int M, heads, d; float scale; bf16_t* dq; float* dk_part; };
template <int UB>
__device__ __forceinline__ void load_index(const ScoreBwd& sb, int b, long long N, long long p0, int total, int i0,
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
__device__ __forceinline__ void load_rows(const ScoreBwd& sb, int b, long long N, const int (&cgv)[UB], const int (&mv)[UB],
                                          const long long (&nv)[UB], uint4 (&kraw)[UB], uint4 (&qraw)[UB]) {
  const int C = sb.heads * sb.d;
#pragma unroll
  for (int v = 0; v < UB; ++v) {
    kraw[v] = *reinterpret_cast<const uint4*>(sb.k + ((long long)b * sb.M + mv[v]) * C + cgv[v] * 8);
    qraw[v] = *reinterpret_cast<const uint4*>(sb.q + ((long long)b * N + nv[v]) * C + cgv[v] * 8);
  }
}
// dq = g * the gathered k rows; the q rows and one mask bit per (pixel, head) into LDS
template <int UB>
__device__ __forceinline__ void scatter(const ScoreBwd& sb, int b, long long N, long long p0, int total, int i0,
                                        const int (&cgv)[UB], const int (&mv)[UB], const long long (&nv)[UB], const uint4 (&kraw)[UB],
                                        const uint4 (&qraw)[UB], uint4* sq, const float* sg, unsigned* mask, int WPC) {
  const int C = sb.heads * sb.d, CG = C >> 3;
#pragma unroll
  for (int v = 0; v < UB; ++v) {
    if (i0 + v * TPB >= total) continue;
    const int nl = (int)(nv[v] - p0);
    const float gv = sg[nl];
    float kv[8];
    unpack8(kraw[v], kv);
#pragma unroll
    for (int j = 0; j < 8; ++j) kv[j] *= gv;
    store8_bf16(sb.dq, ((long long)b * N + nv[v]) * C + cgv[v] * 8, kv);
    sq[nl * CG + cgv[v]] = make_uint4(qraw[v].x, qraw[v].y, qraw[v].z, qraw[v].w);      // (by element: the struct copy kept qraw in scratch)
    const int h = (cgv[v] * 8) / sb.d;
    // one bit per (pixel, head): integer LDS atomic, the result does not depend on the order
    if (cgv[v] * 8 == h * sb.d) atomicOr(&mask[(h * sb.M + mv[v]) * WPC + (nl >> 5)], 1u << (nl & 31));
  }
}

__global__ __launch_bounds__(TPB) void k_attn_scores_bwd(const bf16_t* q, const bf16_t* k, const float* dS, const short* idx,
                                                         long long N, int M, int heads, int d, float scale, int chunk,
                                                         bf16_t* dq, crd_sum_t* dk, int use_lds, float* dk_part, VecBwd vec) {
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
  const ScoreBwd sb{q, k, idx, M, heads, d, scale, dq, dk_part};
  constexpr int UB = 4;
  if (!use_lds) {
    // no chunk of this shape fits in LDS: every product goes to the dk accumulator with an atomic of its own.  A loop of its own (the
    // chunk is not bounded by LDS here, so the items are counted in 64 bits, and g comes from memory with the indices)
    const long long total = (p1 - p0) * CG;
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
        mv[u] = idx[((long long)b * N + nv[u]) * heads + (cgv[u] * 8) / d];
        gv[u] = ok ? scale * dS[(long long)b * N + nv[u]] : 0.f;
      }
      uint4 kraw[UB], qraw[UB];
      load_rows<UB>(sb, b, N, cgv, mv, nv, kraw, qraw);
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        if (i0 + (long long)u * TPB >= total) continue;
        float kv[8], qv[8];
        unpack8(kraw[u], kv);
        unpack8(qraw[u], qv);
#pragma unroll
        for (int j = 0; j < 8; ++j) kv[j] *= gv[u];
        store8_bf16(dq, ((long long)b * N + nv[u]) * C + cgv[u] * 8, kv);
        crd_sum_t* dst = &dk[((long long)b * M + mv[u]) * C + cgv[u] * 8];
#pragma unroll
        for (int j = 0; j < 8; ++j) grad_add(dst + j, gv[u] * qv[j]);
      }
    }
    return;
  }
  const int npx = (int)(p1 - p0), total = npx * CG;
  const int HM = heads * M, WPC = (chunk + 31) >> 5;                           // mask words per (head, key)
  uint4* sq = reinterpret_cast<uint4*>(smem);                                  // [chunk][CG]
  float* sg = reinterpret_cast<float*>(smem + (size_t)chunk * C * 2);          // [chunk]
  unsigned* mask = reinterpret_cast<unsigned*>(sg + chunk);                    // [HM][WPC]
  int cgv[UB], mv[UB];
  long long nv[UB];
  uint4 kraw[UB], qraw[UB];
  load_index<UB>(sb, b, N, p0, total, threadIdx.x, cgv, mv, nv);
  for (int i = threadIdx.x; i < npx; i += TPB) sg[i] = scale * dS[(long long)b * N + p0 + i];      // (in flight with the indices)
  for (int i = threadIdx.x; i < HM * WPC; i += TPB) mask[i] = 0u;
  load_rows<UB>(sb, b, N, cgv, mv, nv, kraw, qraw);
  __syncthreads();
  scatter<UB>(sb, b, N, p0, total, threadIdx.x, cgv, mv, nv, kraw, qraw, sq, sg, mask, WPC);
  for (int i0 = threadIdx.x + UB * TPB; i0 < total; i0 += UB * TPB) {      // chunks of more than 1024 granules
    int cg2[UB], m2[UB];
    long long n2[UB];
    uint4 k2[UB], q2[UB];
    load_index<UB>(sb, b, N, p0, total, i0, cg2, m2, n2);
    load_rows<UB>(sb, b, N, cg2, m2, n2, k2, q2);
    scatter<UB>(sb, b, N, p0, total, i0, cg2, m2, n2, k2, q2, sq, sg, mask, WPC);
  }
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
        float qv[8];
        unpack8(sq[n * CG + cg], qv);
        const float g = sg[n];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += g * qv[j];
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
  load_index<UB>(sb, b, N, p0, total, threadIdx.x, cgv, mv, nv);
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
  load_rows<UB>(sb, b, N, cgv, mv, nv, kraw, qraw);
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
  scatter<UB>(sb, b, N, p0, total, threadIdx.x, cgv, mv, nv, kraw, qraw, sq, sg, mask, WPC);
  for (int i0 = threadIdx.x + UB * TPB; i0 < total; i0 += UB * TPB) {      // chunks of more than 1024 granules
    int cg2[UB], m2[UB];
    long long n2[UB];
    uint4 k2[UB], q2[UB];
    load_index<UB>(sb, b, N, p0, total, i0, cg2, m2, n2);
    load_rows<UB>(sb, b, N, cg2, m2, n2, k2, q2);
    scatter<UB>(sb, b, N, p0, total, i0, cg2, m2, n2, k2, q2, sq, sg, mask, WPC);
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

// workgroups of the flat 8-elements-per-thread kernels: one thread per granule, at most 2048 workgroups (they stride over the rest)
static unsigned flat_grid(long long n8) {
  const long long nb = (n8 + TPB - 1) / TPB;
  return (unsigned)(nb > 2048 ? 2048 : nb);
}

extern "C" int crd_sum_partials_bf16(const float* part, int32_t replicas, int64_t replica_stride, void* dst, int64_t n,
                                     crd_stream_t stream) {
  CRD_CHECK_ARG(part && dst && replicas >= 1 && n > 0 && n % 8 == 0 && replica_stride % 8 == 0, "crd_sum_partials_bf16: bad argument");
  hipLaunchKernelGGL(k_sum_partials_bf16, dim3(flat_grid(n / 8)), dim3(TPB), 0, as_stream(stream), part, replicas, (long long)replica_stride,
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
  hipLaunchKernelGGL(k_attn_dk_fold, dim3(flat_grid(n / 8) + (unsigned)B * cdiv(C, FOLD_VEC_ROWS)), dim3(TPB), 0, as_stream(stream), part, replicas,
                     (long long)replica_stride, reinterpret_cast<bf16_t*>(dst), (long long)(n / 8), B,
                     VecBwd{t, reinterpret_cast<const bf16_t*>(w_dgrad), C, Cpad, inv_n, reinterpret_cast<bf16_t*>(tb), es});
  CRD_LAUNCH_CHECK("crd_attn_dk_fold");
  return CRD_OK;
}

extern "C" int crd_gsum_to_bf16(const crd_sum_t* src, void* dst, int64_t n, crd_stream_t stream) {
  CRD_CHECK_ARG(src && dst && n > 0 && n % 8 == 0, "crd_gsum_to_bf16: bad argument");
  hipLaunchKernelGGL(k_gsum_to_bf16, dim3(flat_grid(n / 8)), dim3(TPB), 0, as_stream(stream), src, reinterpret_cast<bf16_t*>(dst),
                     (long long)(n / 8));
  CRD_LAUNCH_CHECK("crd_gsum_to_bf16");
  return CRD_OK;
}
