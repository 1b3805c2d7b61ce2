// GroupNorm family for gfx950: statistics, apply(+GELU,+dropout mask), backward.
// All kernels are HBM-bound streaming passes: one thread owns 8 consecutive channels (16-byte bf16
// / 32-byte fp32 accesses) of a pixel and keeps its channel group fixed while striding over pixels,
// so per-channel partial sums stay in registers; workgroup partials are merged in LDS and flushed
// with one global atomic per value.
//
// The three stand-alone passes of the training step -- k_gn_apply, k_gn_bwd_reduce, k_gn_bwd_apply -- share one software-pipelined
// loop (stream_first / stream_pixels below): granules stay packed as loaded, slot u of the next batch is requested as soon as slot u
// of this one is unpacked, addresses are a scalar base plus one 32-bit offset per tensor.  Every instantiation needs at most 128
// registers (4 waves per SIMD) and no scratch; the common ones need fewer.  Bytes requested ahead per CU in the steady state =
// waves per SIMD x 4 SIMDs x 64 lanes x slots x bytes per slot:
//   k_gn_apply      bf16 x: 68 registers, 7 waves x 256 lanes x 4 slots x 16 B = 112 KB    (fp32 x: 5 x 256 x 4 x 32 B = 160 KB)
//   k_gn_bwd_reduce bf16 x, dy, GELU:  93 registers, 5 x 256 x 2 x 32 B =  80 KB          (without GELU 6 waves:  96 KB)
//   k_gn_bwd_apply  bf16 dx written once, GELU: 83 registers, 5 x 256 x 2 x 32 B = 80 KB  (without GELU 7 waves: 112 KB)
//   forms with fp32 tensors or a dx they add to take fewer slots (gn_form_slots): 96..128 B per lane, 4..5 waves: 96..160 KB
// Twice the slots (128..256 KB ahead) measured SLOWER on the plan's launches (profiles/gn_stream_sweep.txt), so the constants are
// the smaller ones: what the passes gained came from registers, addressing and issuing loads in front of arithmetic.
// Measured on MI355X, warm, the 171 launches of the 8 x 256 x 416 training step (profiles/gn_stream_ab.txt; 6.3 TB/s = what a
// streaming kernel sustains): crd_gn_apply 0.39 ms = 3.9 TB/s (was 0.41), crd_gn_bwd_reduce 0.68 ms = 3.3 TB/s (was 0.73),
// crd_gn_bwd_apply 0.96 ms = 4.3 TB/s (was 1.23); the large decoder tensors run at 5.0-5.9 TB/s, launches under ~1 MB per
// CU-round are bound by the ~3-5 us a launch of this shape takes.
#include <stdlib.h>
#include <utility>
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int U = 4;   // independent 16-byte loads in flight per thread in k_gn_stats / k_attn_out_residual_stats

// thread -> (channel granule cg, pixel lane pl); CG = C/8 granules; PL = TPB/CG pixel lanes
struct Map {
  int cg, pl, PL; bool active;
  __device__ Map(int C) {
    int CG = C >> 3;
    PL = TPB / CG;
    if (PL < 1) PL = 1;
    active = threadIdx.x < PL * CG;
    cg = threadIdx.x % CG;
    pl = threadIdx.x / CG;
  }
};

// sm holds `rows` rows of n floats (one per pixel lane); leaves their sum in row 0.  LDS float atomics for this merge
// cost 18 us of a 40 us kernel (ablation in tools/bench_gn.py): every lane of a wave hits one of four banks.
__device__ __forceinline__ void fold_rows(float* sm, int n, int rows) {
  for (int i = threadIdx.x; i < n; i += TPB) {
    float a = sm[i];
    for (int r = 1; r < rows; ++r) a += sm[(long long)r * n + i];
    sm[i] = a;
  }
  __syncthreads();
}

template <int XF>
__global__ __launch_bounds__(TPB) void k_gn_stats(const void* x, int x_f32, int x_ld, long long P, int C, int chunk,
                                                  crd_sum_t* stats, crd_sum_t* chan) {
  extern __shared__ float sm[];  // [PL][C][2]: one row of channel sums per pixel lane, folded after the barrier
  const int b = blockIdx.y;
  Map m(C);
  float s[8], ss[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = ss[j] = 0.f;
  if (m.active) {
    long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk;
    if (p1 > P) p1 = P;
    for (long long p = p0 + m.pl; p < p1; p += (long long)U * m.PL) {   // U independent loads in flight per thread
      float v[U][8];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        long long pp = p + (long long)u * m.PL;
        if (pp >= p1) pp = p1 - 1;
        load8t<XF>(x, ((long long)b * P + pp) * x_ld + m.cg * 8, v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (p + (long long)u * m.PL < p1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { s[j] += v[u][j]; ss[j] += v[u][j] * v[u][j]; }
        }
    }
    float4* row = reinterpret_cast<float4*>(sm + (long long)m.pl * 2 * C + m.cg * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) row[j] = make_float4(s[2 * j], ss[2 * j], s[2 * j + 1], ss[2 * j + 1]);
  }
  __syncthreads();
  fold_rows(sm, 2 * C, m.PL);
  if (chan)
    for (int i = threadIdx.x; i < 2 * C; i += TPB) stat_add(&chan[(long long)b * C * 2 + i], sm[i]);
  if (stats)
    for (int g = threadIdx.x; g < (C >> 4) * 2; g += TPB) {
      int slab = g >> 1, which = g & 1;
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) a += sm[(slab * 16 + j) * 2 + which];
      stat_add(&stats[((long long)b * (C >> 4) + slab) * 2 + which], a);
    }
}

// crd_attn_out_residual with the GroupNorm statistics of its output (the block's norm2 input) folded in:
// x1 = x + dp[b]*bf16(u[b][c]*S[b][n] + bp[c]);  stats[b][c/16] += (sum, sumsq) of x1.  Thread mapping and fold as in
// k_gn_stats.
__global__ __launch_bounds__(TPB) void k_attn_out_residual_stats(const float* x, const float* u, const float* S, const float* bp,
                                                                 const float* dp, long long P, int C, int chunk, float* x1,
                                                                 crd_sum_t* stats) {
  extern __shared__ float sm[];  // [PL][C][2]
  const int b = blockIdx.y;
  Map m(C);
  if (m.active) {
    float s[8], ss[8], uu[8], bb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = ss[j] = 0.f;
    const float dps = dp ? dp[b] : 1.f;
    load8(u, (long long)b * C + m.cg * 8, 1, uu);
    load8(bp, m.cg * 8, 1, bb);
    long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk;
    if (p1 > P) p1 = P;
    for (long long p = p0 + m.pl; p < p1; p += (long long)U * m.PL) {
      float v[U][8], sv[U];
#pragma unroll
      for (int q = 0; q < U; ++q) {
        long long pp = p + (long long)q * m.PL;
        if (pp >= p1) pp = p1 - 1;
        load8(x, ((long long)b * P + pp) * C + m.cg * 8, 1, v[q]);
        sv[q] = S[(long long)b * P + pp];
      }
#pragma unroll
      for (int q = 0; q < U; ++q)
        if (p + (long long)q * m.PL < p1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            v[q][j] += dps * bf_round(uu[j] * sv[q] + bb[j]);
            s[j] += v[q][j]; ss[j] += v[q][j] * v[q][j];
          }
          store8_f32(x1, ((long long)b * P + p + (long long)q * m.PL) * C + m.cg * 8, v[q]);
        }
    }
    float4* row = reinterpret_cast<float4*>(sm + (long long)m.pl * 2 * C + m.cg * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) row[j] = make_float4(s[2 * j], ss[2 * j], s[2 * j + 1], ss[2 * j + 1]);
  }
  __syncthreads();
  fold_rows(sm, 2 * C, m.PL);
  for (int g = threadIdx.x; g < (C >> 4) * 2; g += TPB) {
    int slab = g >> 1, which = g & 1;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) a += sm[(slab * 16 + j) * 2 + which];
    stat_add(&stats[((long long)b * (C >> 4) + slab) * 2 + which], a);
  }
}

// ---- the streaming loop shared by k_gn_apply, k_gn_bwd_reduce and k_gn_bwd_apply ----------------------------------------------
// One granule as it was loaded: the 8 channels of one pixel, 16 B of bf16 or 32 B of fp32, kept PACKED until the point of use (a batch
// held as floats was v[4][8] + d[4][8] = 64 registers; packed bf16 it is 32).
template <int F32> struct Gran;
template <> struct Gran<0> {
  uint4 q;
  __device__ __forceinline__ void load(const char* p) { q = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void get(float (&v)[8]) const { unpack8(q, v); }
};
template <> struct Gran<1> {
  float4 a, b;
  __device__ __forceinline__ void load(const char* p) {
    a = reinterpret_cast<const float4*>(p)[0]; b = reinterpret_cast<const float4*>(p)[1];
  }
  __device__ __forceinline__ void get(float (&v)[8]) const {
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
};
// A tensor as one thread walks it: the address of the first pixel of the workgroup's chunk (the same for every thread: scalar
// registers), the thread's byte offset from there to its granule in its next pixel, and the bytes from one of its pixels to the
// next (PL rows).  One 32-bit add per access and one register per tensor; as ((b * P + pixel) * ld + c0) per access the loop spent a
// 64-bit multiply on each and kept a 64-bit address per slot and tensor in registers.  The launchers refuse a chunk whose rows
// span 2^31 bytes or more (gn_chunk_fits).
struct Walk {
  char* base; unsigned off, step;
  __device__ Walk(const void* tensor, int elem_bytes, long long first_row, int ld, int c0, int pl, int PL)
      : base(reinterpret_cast<char*>(const_cast<void*>(tensor)) + first_row * ld * elem_bytes),
        off((unsigned)(pl * ld + c0) * elem_bytes), step((unsigned)(PL * ld) * elem_bytes) {}
  __device__ __forceinline__ char* next() { char* r = base + off; off += step; return r; }
};

// A thread walks its pixels q, q + PL, q + 2 PL, ... < n (counted from the start of its workgroup's chunk) in that order, NU of them
// ("slots") per batch.  request(u) loads the thread's next unrequested pixel into slot u (packed), take(u) unpacks slot u into the
// caller's floats, work() does the arithmetic and the stores of what was taken; each advances the Walks it uses, so pixels are
// requested, and worked on, in ascending order whatever NU is.
// stream_first requests the first batch: the caller does that before it loads its parameters, so that everything a workgroup needs
// first is in flight together.  stream_pixels then requests slot u of batch k + 1 as soon as slot u of batch k has been unpacked,
// IN FRONT of that slot's arithmetic and stores: but for the slot being worked on, a whole batch of loads stays in flight per thread
// throughout (with the loads of batch k + 1 issued only after the stores of batch k, nothing was in flight during the arithmetic).
// Which phase a batch runs in is decided for the whole workgroup (scalar branches: a per-thread test would send the lanes of one
// wave through the steady state AND the tail one after the other).  A slot past the end of the chunk is neither requested nor read.
template <int NU, class Req>
__device__ __forceinline__ void stream_first(int q, int n, int PL, Req&& request) {
  if (NU * PL <= n) {           // a whole batch for every lane
#pragma unroll
    for (int u = 0; u < NU; ++u) request(u);
  } else {
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (q + u * PL < n) request(u);
  }
}
template <int NU, class Req, class Take, class Work>
__device__ __forceinline__ void stream_pixels(int q, int n, int PL, Req&& request, Take&& take, Work&& work) {
  const int step = NU * PL;
  int done = 0;                 // pixels of the chunk in finished batches (the same for every thread)
  // steady state: this batch and the next are whole for every lane, so nothing in the body is conditional (around a conditional
  // request the compiler waits for EVERY outstanding load where the branches join, and the pipeline is gone)
#pragma nounroll
  for (; done + 2 * step <= n; done += step) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      take(u);
      request(u);
      work();
      __builtin_amdgcn_sched_barrier(0);        // one slot at a time: interleaved, the slots' temporaries do not fit 128 registers
    }
  }
  q += done;
  if (done + step <= n) {       // the last whole batch: what follows it is ragged, or nothing
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      take(u);
      if (q + u * PL + step < n) request(u);
      work();
    }
    q += step;
    done += step;
  }
  if (done < n) {               // the ragged rest
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (q + u * PL < n) {
        take(u);
        work();
      }
  }
}

// What one output element computes, the same operations in the same order in every kernel that needs them.
// forward: ga = gamma * rstd and be = beta - mean * ga are folded per channel by the caller
template <int ACT>
__device__ __forceinline__ float gn_fwd_elem(float v, float ga, float be, float mk) {
  float w = v * ga + be;
  if (ACT == 1) w = gelu_exact(w);
  return w * mk;
}
// backward: xh = the normalised input, g = dy * mask * act'(xh * gamma + beta), dx = (gamma * g - S1 - xh * S2) * rstd
__device__ __forceinline__ float gn_xhat(float v, float mean, float rstd) { return (v - mean) * rstd; }
template <int ACT>
__device__ __forceinline__ float gn_bwd_g(float xh, float d, float ga, float be, float mk) {
  float g = d * mk;
  if (ACT == 1) g *= gelu_grad(xh * ga + be);
  return g;
}
__device__ __forceinline__ float gn_bwd_dx(float xh, float g, float ga, float S1, float S2, float rstd) {
  return (ga * g - S1 - xh * S2) * rstd;
}
// dx += : the finished gradient is rounded before it is added, as it always was (the old dx used to be loaded behind a run-time
// branch, where the compiler could not fuse the add into the multiply by rstd; now it can, and must not)
__device__ __forceinline__ float add_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// slots per batch (CRD_EXTRA_FLAGS=-DCRD_GN_U_...=n for an A/B build; the sweep is in DESIGN 4, "GroupNorm streaming passes")
#ifndef CRD_GN_U_APPLY
#define CRD_GN_U_APPLY 4
#endif
#ifndef CRD_GN_U_BWD
#define CRD_GN_U_BWD 2
#endif
#ifndef CRD_GN_U_RED
#define CRD_GN_U_RED 2
#endif
constexpr int U_APPLY = CRD_GN_U_APPLY, U_BWD = CRD_GN_U_BWD, U_RED = CRD_GN_U_RED;
// ... of the bf16 forms.  A form that loads more bytes per pixel (fp32 x or dy, the dx it adds to) takes half or a quarter of the
// slots, so that every form requests GN_AHEAD_BYTES or a little more per thread and none needs more registers than GN_WAVES waves per
// SIMD leave it (512 / 4 = 128).  A batch of the partition (U * PL pixels) is then two or four whole batches of such a form.
#ifndef CRD_GN_WAVES
#define CRD_GN_WAVES 4
#endif
constexpr int GN_WAVES = CRD_GN_WAVES, GN_AHEAD_BYTES = 96;
constexpr int gn_form_slots(int slots, int bytes_per_slot) {
  while (slots > 1 && (slots / 2) * bytes_per_slot >= GN_AHEAD_BYTES) slots /= 2;
  return slots;
}

template <int XF, int YF, int ACT>
__global__ __launch_bounds__(TPB, GN_WAVES) void k_gn_apply(const void* x, int x_f32, int x_ld, long long P, int C, int chunk,
                                                  const crd_sum_t* stats, int gmul, const float* gamma, const float* beta,
                                                  int act, const float* mask, void* y, int y_ld, int y_f32, float y_inv_scale,
                                                  void* y2, int y2_ld) {
  const int b = blockIdx.y;
  Map m(C);
  if (!m.active) return;
  const int c0 = m.cg * 8;
  long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk;
  if (p1 > P) p1 = P;
  const long long row0 = (long long)b * P + p0;             // the chunk's first pixel, as a row of the tensors
  const int q = m.pl, n = (int)(p1 - p0);
  // Every load the first batch needs is issued before anything is waited for -- the pixels, then the parameters, then
  // the statistics: four dependent round trips (kernel arguments, statistics, parameters, data) were most of the ~5 us
  // a launch on a small grid takes.
  constexpr int NU = gn_form_slots(U_APPLY, XF ? 32 : 16);
  Gran<XF> xq[NU];
  Walk xw(x, XF ? 4 : 2, row0, x_ld, c0, m.pl, m.PL);
  auto request = [&](int u) __attribute__((always_inline)) { xq[u].load(xw.next()); };
  stream_first<NU>(q, n, m.PL, request);
  float ga[8], be[8], mk[8];
  load8(gamma, c0, 1, ga);
  load8(beta, c0, 1, be);
  if (mask) load8(mask, (long long)b * C + c0, 1, mk);
  else {
#pragma unroll
    for (int j = 0; j < 8; ++j) mk[j] = 1.f;
  }
  float mean, rstd;
  const int grp = (c0 >> 4) / gmul;
  gn_mean_rstd(stats + (long long)b * (C >> 4) * 2, grp * gmul, gmul, (float)P * 16.f * gmul, mean, rstd);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ga[j] *= rstd;
    be[j] -= mean * ga[j];
  }
  float v[8];
  Walk yw(y, YF >= 2 ? 1 : YF ? 4 : 2, row0, y_ld, c0, m.pl, m.PL);      // YF: 0 bf16, 1 fp32, 2 e4m3, 3 e4m3 (y) and bf16 (y2)
  Walk y2w(y2, 2, row0, YF == 3 ? y2_ld : 0, c0, m.pl, m.PL);
  stream_pixels<NU>(
      q, n, m.PL, request, [&](int u) __attribute__((always_inline)) { xq[u].get(v); },
      [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gn_fwd_elem<ACT>(v[j], ga[j], be[j], mk[j]);
        if (YF >= 2) store8_fp8(yw.next(), 0, v, y_inv_scale);
        else if (YF) store8_f32(reinterpret_cast<float*>(yw.next()), 0, v);
        else store8_bf16(yw.next(), 0, v);
        if (YF == 3) store8_bf16(y2w.next(), 0, v);
      });
}

// r[b][c] = (sum_p g, sum_p g*xhat), g = dy*mask*act'(u)
// gridDim.z = channel slices of Cs channels each (a multiple of the group width): a workgroup then covers Cs channels of
// gridDim.z times the pixels instead of all C channels -- the same number of workgroups, 2 Cs instead of 2 C atomics each
// (Mlp.norm2 of stages 1-2: 1-1.7 M 64-bit atomics per launch were ~10 of its 32-36 us).
template <int XF, int DF, int ACT>
__global__ __launch_bounds__(TPB, GN_WAVES) void k_gn_bwd_reduce(const void* x, int x_f32, int x_ld, const void* dy, int dy_f32,
                                                       int dy_ld, long long P, int C, int Cs, int chunk, const crd_sum_t* stats,
                                                       int gmul, const float* gamma, const float* beta, int act,
                                                       const float* mask, crd_sum_t* r, float* partial) {
  extern __shared__ float sm[];  // [PL][Cs][2]
  const int b = blockIdx.y, cs = blockIdx.z * Cs;
  Map m(Cs);
  if (m.active) {
    const int c0 = cs + m.cg * 8;
    long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk;
    if (p1 > P) p1 = P;
    const long long row0 = (long long)b * P + p0;
    const int q = m.pl, n = (int)(p1 - p0);
    // first batch, parameters and statistics all in flight before the first wait (see k_gn_apply)
    // (all-fp32 with GELU: one slot of 64 B -- with two it spills 116 bytes per lane at 128 registers)
    constexpr int NU = (XF && DF && ACT) ? 1 : gn_form_slots(U_RED, (XF ? 32 : 16) + (DF ? 32 : 16));
    Gran<XF> xq[NU];
    Gran<DF> dq[NU];
    Walk xw(x, XF ? 4 : 2, row0, x_ld, c0, m.pl, m.PL), dw(dy, DF ? 4 : 2, row0, dy_ld, c0, m.pl, m.PL);
    auto request = [&](int u) __attribute__((always_inline)) {
      xq[u].load(xw.next());
      dq[u].load(dw.next());
    };
    stream_first<NU>(q, n, m.PL, request);
    float ga[8], be[8], mk[8], s0[8], s1[8];
    load8(gamma, c0, 1, ga);
    load8(beta, c0, 1, be);
    if (mask) load8(mask, (long long)b * C + c0, 1, mk);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!mask) mk[j] = 1.f;
      s0[j] = s1[j] = 0.f;
    }
    float mean, rstd;
    const int grp = (c0 >> 4) / gmul;
    gn_mean_rstd(stats + (long long)b * (C >> 4) * 2, grp * gmul, gmul, (float)P * 16.f * gmul, mean, rstd);
    float v[8], d[8];
    stream_pixels<NU>(
        q, n, m.PL, request, [&](int u) __attribute__((always_inline)) { xq[u].get(v); dq[u].get(d); },
        [&]() __attribute__((always_inline)) {                // (a thread's pixels in ascending order, whatever the batch size)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xh = gn_xhat(v[j], mean, rstd);
            const float g = gn_bwd_g<ACT>(xh, d[j], ga[j], be[j], mk[j]);
            s0[j] += g; s1[j] += g * xh;
            if (ACT == 1 && j == 3) __builtin_amdgcn_sched_barrier(0);
          }
          // the sums are opaque between pixels: otherwise the SLP vectoriser pairs the contributions of two SLOTS to one sum, keeps both
          // slots unpacked to do so and the kernel spills (92-388 bytes of scratch per lane at 128 registers)
#pragma unroll
          for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(s0[j]), "+v"(s1[j]));
        });
    float4* row = reinterpret_cast<float4*>(sm + (long long)m.pl * 2 * Cs + m.cg * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) row[j] = make_float4(s0[2 * j], s1[2 * j], s0[2 * j + 1], s1[2 * j + 1]);
  }
  __syncthreads();
  fold_rows(sm, 2 * Cs, m.PL);
  if (partial) {   // plain stores of this workgroup's sums; k_gn_bwd_finalize folds them (no contended atomics)
    float* dst = partial + ((long long)b * gridDim.x + blockIdx.x) * 2 * C + cs * 2;
    for (int i = threadIdx.x; i < 2 * Cs; i += TPB) dst[i] = sm[i];
    return;
  }
  // per-channel sums out; in the same pass weight them with gamma in place (all threads, coalesced gamma loads) for the
  // group sums below -- a serial walk of one thread over the 64..128 channels of a group, with a dependent gamma load
  // per channel, was 5 us of this kernel's 13 us floor
  for (int i = threadIdx.x; i < 2 * Cs; i += TPB) {
    const float v = sm[i];
    grad_add(&r[((long long)b * C + cs) * 2 + i], v);
    sm[i] = v * gamma[cs + (i >> 1)];
  }
  __syncthreads();
  // per-group sums S1 = sum_c gamma_c r0, S2 = sum_c gamma_c r1 (stored after the [B][C][2] block of r)
  const int cpg = 16 * gmul, G = C / cpg, Gs = Cs / cpg;
  crd_sum_t* rg = r + (long long)gridDim.y * C * 2 + ((long long)b * G + cs / cpg) * 2;
  for (int gi = threadIdx.x; gi < 2 * Gs; gi += TPB) {
    const int grp = gi >> 1, which = gi & 1;
    float acc = 0.f;
    for (int c = grp * cpg; c < (grp + 1) * cpg; ++c) acc += sm[c * 2 + which];
    grad_add(&rg[grp * 2 + which], acc);
  }
}

// r[b][c][0..1] = sum over workgroup partials; rg[b][grp] += sum_c gamma_c r[b][c]  (64 channels per workgroup)
__global__ __launch_bounds__(TPB) void k_gn_bwd_finalize(const float* partial, int nblk, int C, int gmul, const float* gamma,
                                                         crd_sum_t* r, int B) {
  __shared__ float sm[4][64][2];
  const int b = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), lane = threadIdx.x >> 6;
  float s0 = 0.f, s1 = 0.f;
  if (c < C)
    for (int k = lane; k < nblk; k += 4) {
      const float* p = partial + ((long long)b * nblk + k) * 2 * C + c * 2;
      s0 += p[0]; s1 += p[1];
    }
  sm[lane][threadIdx.x & 63][0] = s0; sm[lane][threadIdx.x & 63][1] = s1;
  __syncthreads();
  if (lane == 0 && c < C) {
    s0 = sm[0][threadIdx.x][0] + sm[1][threadIdx.x][0] + sm[2][threadIdx.x][0] + sm[3][threadIdx.x][0];
    s1 = sm[0][threadIdx.x][1] + sm[1][threadIdx.x][1] + sm[2][threadIdx.x][1] + sm[3][threadIdx.x][1];
    r[((long long)b * C + c) * 2] = to_fx(s0, GRAD_ONE);          // fixed summation order above: reproducible
    r[((long long)b * C + c) * 2 + 1] = to_fx(s1, GRAD_ONE);
    const float g = gamma[c];
    sm[0][threadIdx.x][0] = g * s0; sm[0][threadIdx.x][1] = g * s1;
  }
  __syncthreads();
  // group sums: 16-channel slabs of this 64-channel window, added into the group's accumulator
  if (threadIdx.x < 8) {
    const int slab = threadIdx.x >> 1, which = threadIdx.x & 1, c0 = blockIdx.x * 64 + slab * 16;
    if (c0 < C) {
      float a = 0.f;
      for (int j = 0; j < 16; ++j) a += sm[0][slab * 16 + j][which];
      const int cpg = 16 * gmul;
      grad_add(r + (long long)B * C * 2 + ((long long)b * (C / cpg) + c0 / cpg) * 2 + which, a);
    }
  }
}

// Phase 2 of the backward.  What a launch writes is decided at compile time, so that the common form (bf16 dx written once) does not
// carry the registers of the others: DXF = dx is fp32, ACC = dx is added to, DX2 = the scaled bf16 copy, FP8 = the e4m3 copy with its
// amax (crd_gn_bwd_apply_fp8: bf16 dx written once, no copy).  Parameter gradients stay a run-time branch: it is taken AFTER the
// pixels, where none of its registers are live across the loop and its dependent loads (the old and new sums) do not stand between
// a workgroup's first loads and its first arithmetic.
struct BapArgs {
  const void *x, *dy;
  const crd_sum_t *stats, *r;
  const float *gamma, *beta, *mask, *scale2, *scale8;
  float *dgamma, *dbeta;
  void *dx, *dx2;
  unsigned char* dx8;
  unsigned* amax8;
  long long P;
  int x_ld, dy_ld, dx_ld, dx2_ld, dx8_ld, C, chunk, gmul, B;
};

template <int XF, int DF, int ACT, int DXF, int ACC, int DX2, int FP8>
__global__ __launch_bounds__(TPB, GN_WAVES) void k_gn_bwd_apply(const BapArgs a) {
  const int b = blockIdx.y, C = a.C;
  const long long P = a.P;
  Map m(C);
  float amax = 0.f;
  if (m.active) {
    const int c0 = m.cg * 8;
    long long p0 = (long long)blockIdx.x * a.chunk, p1 = p0 + a.chunk;
    if (p1 > P) p1 = P;
    const long long row0 = (long long)b * P + p0;
    const int q = m.pl, n = (int)(p1 - p0);
    // first batch, parameters, reduce sums and statistics all in flight before the first wait (see k_gn_apply); the dx a launch
    // adds to is streamed like x and dy (its owner is the only thread that reads or writes it, so requesting it ahead is safe,
    // also where dx is dy)
    constexpr int NU = gn_form_slots(U_BWD, (XF ? 32 : 16) + (DF ? 32 : 16) + (ACC ? (DXF ? 32 : 16) : 0));
    Gran<XF> xq[NU];
    Gran<DF> dq[NU];
    Gran<DXF> wq[ACC ? NU : 1];
    Walk xw(a.x, XF ? 4 : 2, row0, a.x_ld, c0, m.pl, m.PL), dw(a.dy, DF ? 4 : 2, row0, a.dy_ld, c0, m.pl, m.PL);
    Walk ow(a.dx, DXF ? 4 : 2, row0, a.dx_ld, c0, m.pl, m.PL), aw = ow;       // dx as it is written / as it is added to
    Walk o8w(a.dx8, 1, row0, FP8 ? a.dx8_ld : 0, c0, m.pl, m.PL), o2w(a.dx2, 2, row0, DX2 ? a.dx2_ld : 0, c0, m.pl, m.PL);
    auto request = [&](int u) __attribute__((always_inline)) {
      xq[u].load(xw.next());
      dq[u].load(dw.next());
      if (ACC) wq[u].load(aw.next());
    };
    stream_first<NU>(q, n, m.PL, request);
    float ga[8], be[8], mk[8];
    load8(a.gamma, c0, 1, ga);
    load8(a.beta, c0, 1, be);
    if (a.mask) load8(a.mask, (long long)b * C + c0, 1, mk);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) mk[j] = 1.f;
    }
    const int grp = (c0 >> 4) / a.gmul;
    const int cpg = 16 * a.gmul;
    const float inv_m = 1.f / ((float)P * cpg);
    const crd_sum_t* rg = a.r + (long long)a.B * C * 2 + ((long long)b * (C / cpg) + grp) * 2;
    const float S1 = grad_get(rg) * inv_m, S2 = grad_get(rg + 1) * inv_m;
    float mean, rstd;
    gn_mean_rstd(a.stats + (long long)b * (C >> 4) * 2, grp * a.gmul, a.gmul, (float)P * cpg, mean, rstd);
    const float sc2 = (DX2 && a.scale2) ? a.scale2[b] : 1.f;
    // dx8 (config 5, fp8 data gradients): an e4m3 copy of the bf16 gradient just stored, e4m3(bf16(dx) / *scale8), and the running
    // max |bf16(dx)| of the launch into one of CRD_FP8_AMAX_SLOTS slots (u32 max on the bit pattern of a non-negative float)
    const float inv8 = (FP8 && a.scale8) ? 1.f / fmaxf(*a.scale8, 1e-30f) : 0.f;
    float v[8], d[8], w[8];
    stream_pixels<NU>(
        q, n, m.PL, request,
        [&](int u) __attribute__((always_inline)) {
          xq[u].get(v); dq[u].get(d);
          if (ACC) wq[u].get(w);
        },
        [&]() __attribute__((always_inline)) {
          float o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xh = gn_xhat(v[j], mean, rstd);
            const float g = gn_bwd_g<ACT>(xh, d[j], ga[j], be[j], mk[j]);
            o[j] = gn_bwd_dx(xh, g, ga[j], S1, S2, rstd);
            if (ACT == 1 && j == 3) __builtin_amdgcn_sched_barrier(0);
          }
          if (ACC) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = add_rounded(o[j], w[j]);
          }
          if (DXF) store8_f32(reinterpret_cast<float*>(ow.next()), 0, o);
          else store8_bf16(ow.next(), 0, o);
          if (FP8) {          // e4m3 copy of the stored bf16 gradient + its running amax
            // The bf16 values come from the hardware converter (v_cvt_pk_bf16_f32, what store8_bf16 above wrote) and are unpacked once for
            // BOTH the amax and the e4m3 conversion: as software roundings per use (bf_round = ~5 integer operations, twice per element)
            // they were 80 of this path's ~110 vector operations per 8 elements and made crd_gn_bwd_apply_fp8 459 us where the plain apply takes
            // 318 (B = 16, 128 channels): three quarters of what the e4m3 data gradients gain (profiles/r06_c5_decoder_backward_chain_*).
            const uint32_t w0 = pack_bf2(o[0], o[1]), w1 = pack_bf2(o[2], o[3]), w2 = pack_bf2(o[4], o[5]), w3 = pack_bf2(o[6], o[7]);
            const float r[8] = {bf_lo(w0), bf_hi(w0), bf_lo(w1), bf_hi(w1), bf_lo(w2), bf_hi(w2), bf_lo(w3), bf_hi(w3)};
            // a NaN / infinite gradient would vanish here -- fmaxf drops NaN, the e4m3 conversion clamps to +-448 -- while the bf16 tensor next
            // to it carries it on: raise the sticky non-finite flag instead, so that the step reports NaN like the bf16 path.
            // (one test per 8 values: a sum is non-finite iff a term is, or the finite terms overflow -- 8 values near the bf16 maximum)
            const float chk = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            if (!(fabsf(chk) < 3.0e38f)) crd_tu_nonfinite = 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(r[j]));
            uint2 q8;
            q8.x = pack_fp8x4(r[0] * inv8, r[1] * inv8, r[2] * inv8, r[3] * inv8);
            q8.y = pack_fp8x4(r[4] * inv8, r[5] * inv8, r[6] * inv8, r[7] * inv8);
            *reinterpret_cast<uint2*>(o8w.next()) = q8;
          }
          if (DX2) {          // second copy of the finished gradient: bf16(scale2[b] * dx)
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] *= sc2;
            store8_bf16(o2w.next(), 0, o);
          }
        });
  }
  if (b == 0 && a.dgamma) {   // parameter gradients: the workgroups of sample 0 share the channels (one workgroup doing all
                              // of them put B x C dependent loads in front of its own pixels: +5 us on the small grids)
    for (int c = blockIdx.x * TPB + threadIdx.x; c < C; c += gridDim.x * TPB) {
      const float ob = a.dbeta[c], og = a.dgamma[c];        // (requested with the sums, not behind them)
      long long g0, g1;
      sum_samples(a.r, a.B, C, c, g0, g1);
      a.dbeta[c] = ob + (float)g0 * (1.f / GRAD_ONE);
      a.dgamma[c] = og + (float)g1 * (1.f / GRAD_ONE);
    }
  }
  if (FP8) {              // one u32 max per workgroup, spread over the slots (same-address atomics serialise chip-wide: ~13 ns each)
    __shared__ float s_amax[TPB / 64];
#pragma unroll
    for (int o_ = 32; o_ > 0; o_ >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o_));
    if ((threadIdx.x & 63) == 0) s_amax[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
      float a_ = s_amax[0];
      for (int w_ = 1; w_ < TPB / 64; ++w_) a_ = fmaxf(a_, s_amax[w_]);
      if (a_ > 0.f) atomicMax(a.amax8 + ((blockIdx.x + blockIdx.y * gridDim.x) % CRD_FP8_AMAX_SLOTS), __float_as_uint(a_));
    }
  }
}

struct GnKnobs { int minpix, small, cap_r, cap_e; };
inline const GnKnobs& gn_knobs() {
  static const GnKnobs k = {crd_dev_int("CRD_GN_MINPIX", 2), crd_dev_int("CRD_GN_SMALL", 256), crd_dev_int("CRD_GN_CAP_R", 768),
                            crd_dev_int("CRD_GN_CAP_E", 2048)};
  return k;
}

// Partition of the REDUCING kernels (crd_gn_stats, crd_attn_out_residual_stats, crd_gn_bwd_reduce).  It decides which float partial
// sums are formed, so it does not change: a step stays bit-reproducible against earlier builds only while it holds.
inline void grid_for(long long P, int C, int B, dim3& grid, int& chunk) {
  const GnKnobs& k = gn_knobs();
  int CG = C >> 3;
  int PL = TPB / CG; if (PL < 1) PL = 1;
  long long per_block = (long long)PL * 8;         // >= 8 pixels per pixel-lane (two batches of U loads)
  long long nblk = (P + per_block - 1) / per_block;
  if (nblk * B < k.small && k.minpix < 8) {          // small grids: fewer pixels per lane rather than idle CUs
    per_block = (long long)PL * k.minpix;
    nblk = (P + per_block - 1) / per_block;
  }
  long long cap = k.cap_r / (B > 0 ? B : 1); if (cap < 1) cap = 1;
  if (nblk > cap) nblk = cap;
  if (nblk < 1) nblk = 1;
  chunk = (int)((P + nblk - 1) / nblk);
  nblk = (P + chunk - 1) / chunk;
  grid = dim3((unsigned)nblk, (unsigned)B);
}

// Partition of the ELEMENTWISE kernels (crd_gn_apply[_fp8]: kind 0, crd_gn_bwd_apply[_fp8]: kind 1); their results do not depend on
// it.  A batch is U * PL pixels (what a workgroup's lanes request at once).  Grids that do not fill the chip keep the small-grid rule
// of grid_for (fewer pixels per lane rather than idle CUs).  Every other grid gets chunks of WHOLE batches, so that only the last
// workgroup of a sample can have a ragged batch (the predicated tail of the loop, where loads are waited for all at once), at least 8 pixels
// per lane, and at most cap_e workgroups in all: a few per CU that live long, not thousands that pay the four dependent round
// trips of a workgroup's head for two to four batches.
inline int gn_slots(int kind) { return kind == 0 ? U_APPLY : U_BWD; }
inline void gn_elem_shape(long long P, int C, int B, int kind, long long& nblk, long long& chunk, long long& batch) {
  const GnKnobs& k = gn_knobs();
  const int U_ = gn_slots(kind);
  int CG = C >> 3;
  int PL = TPB / CG; if (PL < 1) PL = 1;
  batch = (long long)U_ * PL;
  long long cap = k.cap_e / (B > 0 ? B : 1); if (cap < 1) cap = 1;
  const long long per_block = (long long)PL * 8;
  if ((P + per_block - 1) / per_block * B < k.small && k.minpix < 8) {
    const long long pb = (long long)PL * k.minpix;
    nblk = (P + pb - 1) / pb;
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    chunk = (P + nblk - 1) / nblk;
  } else {
    const long long nbatch = (P + batch - 1) / batch;
    long long per = (nbatch + cap - 1) / cap;                       // batches per workgroup
    const long long least = (8 + U_ - 1) / U_;
    if (per < least) per = least;
    chunk = per * batch;
    if (chunk > P) chunk = P;
  }
  if (chunk < 1) chunk = 1;
  nblk = (P + chunk - 1) / chunk;
  if (nblk < 1) nblk = 1;
}
// the Walks of the streaming kernels keep 32-bit byte offsets inside a workgroup's chunk (rows of at most 4-byte elements)
inline bool gn_chunk_fits(int chunk, int ld) { return ((long long)chunk + TPB) * ld * 4 < (1ll << 31); }
#define CRD_GN_CHUNK_FITS(name, chunk, ld) \
  CRD_UNSUPPORTED(gn_chunk_fits(chunk, ld), name ": a workgroup's %d rows of %d elements span 2 GiB or more", chunk, ld)

inline void grid_elem(long long P, int C, int B, int kind, dim3& grid, int& chunk) {
  long long nblk, ch, batch;
  gn_elem_shape(P, C, B, kind, nblk, ch, batch);
  chunk = (int)ch;
  grid = dim3((unsigned)nblk, (unsigned)B);
}

int check_common(const char* name, int x_ld, int x_coff, int C, int x_f32) {
  if (C % 16 != 0 || C > 2048) { crd_set_error("%s: C must be a multiple of 16 and <= 2048 (got %d)", name, C); return CRD_E_UNSUPPORTED; }
  if (x_ld % 8 || x_coff % 8) { crd_set_error("%s: ld/coff must be multiples of 8", name); return CRD_E_INVALID; }
  (void)x_f32;
  return CRD_OK;
}

// LDS of the reducing kernels: one row of 2*C sums per pixel lane
inline size_t lds_rows(int C) {
  int PL = TPB / (C >> 3); if (PL < 1) PL = 1;
  return (size_t)PL * 2 * C * sizeof(float);
}

inline const void* off_ptr(const void* p, int f32, int coff) {
  return f32 ? (const void*)(reinterpret_cast<const float*>(p) + coff) : (const void*)(reinterpret_cast<const bf16_t*>(p) + coff);
}

}  // namespace

extern "C" int crd_gn_stats(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t P, int32_t C,
                            crd_sum_t* stats, crd_sum_t* chan_sums, crd_stream_t stream) {
  CRD_CHECK_ARG(x && (stats || chan_sums), "crd_gn_stats: null pointer");
  int rc = check_common("crd_gn_stats", x_ld, x_coff, C, x_f32);
  if (rc) return rc;
  dim3 grid; int chunk;
  grid_for(P, C, B, grid, chunk);
  if (x_f32) hipLaunchKernelGGL(k_gn_stats<1>, grid, dim3(TPB), lds_rows(C), as_stream(stream), off_ptr(x, x_f32, x_coff),
                                x_f32, x_ld, (long long)P, C, chunk, stats, chan_sums);
  else hipLaunchKernelGGL(k_gn_stats<0>, grid, dim3(TPB), lds_rows(C), as_stream(stream), off_ptr(x, x_f32, x_coff),
                          x_f32, x_ld, (long long)P, C, chunk, stats, chan_sums);
  CRD_LAUNCH_CHECK("crd_gn_stats");
  return CRD_OK;
}

extern "C" int crd_attn_out_residual_stats(const float* x, const float* u, const float* S, const float* bp, const float* dp,
                                           int32_t B, int32_t N, int32_t C, float* x1, crd_sum_t* stats, crd_stream_t stream) {
  CRD_CHECK_ARG(x && u && S && bp && x1 && stats, "crd_attn_out_residual_stats: null pointer");
  int rc = check_common("crd_attn_out_residual_stats", C, 0, C, 1);
  if (rc) return rc;
  dim3 grid; int chunk;
  grid_for(N, C, B, grid, chunk);
  hipLaunchKernelGGL(k_attn_out_residual_stats, grid, dim3(TPB), lds_rows(C), as_stream(stream), x, u, S, bp, dp, (long long)N, C,
                     chunk, x1, stats);
  CRD_LAUNCH_CHECK("crd_attn_out_residual_stats");
  return CRD_OK;
}

extern "C" int crd_gn_apply(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t P, int32_t C,
                            const crd_sum_t* stats, int32_t gmul, const float* gamma, const float* beta, int32_t act,
                            const float* mask, void* y, int32_t y_f32, int32_t y_ld, int32_t y_coff, crd_stream_t stream) {
  CRD_CHECK_ARG(x && stats && gamma && beta && y, "crd_gn_apply: null pointer");
  CRD_CHECK_ARG(gmul >= 1 && (C / 16) % gmul == 0, "crd_gn_apply: bad gmul %d for C=%d", gmul, C);
  CRD_CHECK_ARG(y_ld % 8 == 0 && y_coff % 8 == 0, "crd_gn_apply: y_ld/y_coff must be multiples of 8");
  int rc = check_common("crd_gn_apply", x_ld, x_coff, C, x_f32);
  if (rc) return rc;
  dim3 grid; int chunk;
  grid_elem(P, C, B, 0, grid, chunk);
  CRD_GN_CHUNK_FITS("crd_gn_apply", chunk, x_ld > y_ld ? x_ld : y_ld);
  void* yp = y_f32 ? (void*)(reinterpret_cast<float*>(y) + y_coff) : (void*)(reinterpret_cast<bf16_t*>(y) + y_coff);
#define CRD_GN_APPLY(XF, YF, ACT)                                                                                        \
  hipLaunchKernelGGL((k_gn_apply<XF, YF, ACT>), grid, dim3(TPB), 0, as_stream(stream), off_ptr(x, x_f32, x_coff), x_f32, \
                     x_ld, (long long)P, C, chunk, stats, gmul, gamma, beta, act, mask, yp, y_ld, y_f32, 1.f, nullptr, 0)
  const int key = (x_f32 ? 4 : 0) | (y_f32 ? 2 : 0) | (act ? 1 : 0);
  switch (key) {
    case 0: CRD_GN_APPLY(0, 0, 0); break;  case 1: CRD_GN_APPLY(0, 0, 1); break;
    case 2: CRD_GN_APPLY(0, 1, 0); break;  case 3: CRD_GN_APPLY(0, 1, 1); break;
    case 4: CRD_GN_APPLY(1, 0, 0); break;  case 5: CRD_GN_APPLY(1, 0, 1); break;
    case 6: CRD_GN_APPLY(1, 1, 0); break;  default: CRD_GN_APPLY(1, 1, 1); break;
  }
#undef CRD_GN_APPLY
  CRD_LAUNCH_CHECK("crd_gn_apply");
  return CRD_OK;
}

extern "C" int crd_gn_apply_fp8(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t P, int32_t C,
                                const crd_sum_t* stats, int32_t gmul, const float* gamma, const float* beta, int32_t act,
                                const float* mask, void* y_fp8, int32_t y_ld, int32_t y_coff, float y_scale, void* y_bf16,
                                int32_t yb_ld, int32_t yb_coff, crd_stream_t stream) {
  CRD_CHECK_ARG(x && stats && gamma && beta && y_fp8 && y_scale > 0.f, "crd_gn_apply_fp8: null pointer / bad scale");
  CRD_CHECK_ARG(gmul >= 1 && (C / 16) % gmul == 0, "crd_gn_apply_fp8: bad gmul %d for C=%d", gmul, C);
  CRD_CHECK_ARG(y_ld % 8 == 0 && y_coff % 8 == 0 && yb_ld % 8 == 0 && yb_coff % 8 == 0, "crd_gn_apply_fp8: ld/coff must be multiples of 8");
  int rc = check_common("crd_gn_apply_fp8", x_ld, x_coff, C, x_f32);
  if (rc) return rc;
  dim3 grid; int chunk;
  grid_elem(P, C, B, 0, grid, chunk);
  CRD_GN_CHUNK_FITS("crd_gn_apply_fp8", chunk, (x_ld > y_ld ? x_ld : y_ld) > yb_ld ? (x_ld > y_ld ? x_ld : y_ld) : yb_ld);
  void* yp = reinterpret_cast<unsigned char*>(y_fp8) + y_coff;
  void* y2 = y_bf16 ? (void*)(reinterpret_cast<bf16_t*>(y_bf16) + yb_coff) : nullptr;
#define CRD_GN_APPLY8(XF, YF, ACT)                                                                                       \
  hipLaunchKernelGGL((k_gn_apply<XF, YF, ACT>), grid, dim3(TPB), 0, as_stream(stream), off_ptr(x, x_f32, x_coff), x_f32, \
                     x_ld, (long long)P, C, chunk, stats, gmul, gamma, beta, act, mask, yp, y_ld, 0, 1.f / y_scale, y2, yb_ld)
  switch ((x_f32 ? 4 : 0) | (y2 ? 2 : 0) | (act ? 1 : 0)) {
    case 0: CRD_GN_APPLY8(0, 2, 0); break;  case 1: CRD_GN_APPLY8(0, 2, 1); break;
    case 2: CRD_GN_APPLY8(0, 3, 0); break;  case 3: CRD_GN_APPLY8(0, 3, 1); break;
    case 4: CRD_GN_APPLY8(1, 2, 0); break;  case 5: CRD_GN_APPLY8(1, 2, 1); break;
    case 6: CRD_GN_APPLY8(1, 3, 0); break;  default: CRD_GN_APPLY8(1, 3, 1); break;
  }
#undef CRD_GN_APPLY8
  CRD_LAUNCH_CHECK("crd_gn_apply_fp8");
  return CRD_OK;
}

extern "C" int crd_gn_bwd_reduce(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, const void* dy, int32_t dy_f32,
                                 int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                                 int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask,
                                 crd_sum_t* r, float* scratch, int64_t scratch_capacity, crd_stream_t stream) {
  CRD_CHECK_ARG(x && dy && stats && gamma && beta && r, "crd_gn_bwd_reduce: null pointer");
  CRD_CHECK_ARG(gmul >= 1 && (C / 16) % gmul == 0, "crd_gn_bwd_reduce: bad gmul");
  CRD_CHECK_ARG(dy_ld % 8 == 0 && dy_coff % 8 == 0, "crd_gn_bwd_reduce: dy_ld/dy_coff must be multiples of 8");
  int rc = check_common("crd_gn_bwd_reduce", x_ld, x_coff, C, x_f32);
  if (rc) return rc;
  dim3 grid; int chunk;
  // channel slices (atomics path, C >= 256): the largest S in 8 / 4 / 2 whose slices are >= 64 channels and whole groups
  int S = 1;
  static int slicing = -1;
  if (slicing < 0) slicing = crd_dev_int("CRD_GN_RED_SLICES", 1);      // developer switch (A/B)
  if (slicing && !scratch && C >= 256) {
    const int cpg = 16 * gmul;
    for (int s_ = 8; s_ > 1; s_ >>= 1)
      if (C % s_ == 0 && (C / s_) % cpg == 0 && (C / s_) % 8 == 0 && C / s_ >= 64) { S = s_; break; }
  }
  const int Cs = C / S;
  grid_for(P, Cs, B * S, grid, chunk);            // the same number of workgroups: S times the pixels per workgroup
  grid = dim3(grid.x, (unsigned)B, (unsigned)S);
  CRD_GN_CHUNK_FITS("crd_gn_bwd_reduce", chunk, x_ld > dy_ld ? x_ld : dy_ld);
  float* part = (scratch && (long long)B * grid.x * 2 * C <= scratch_capacity && grid.x > 1) ? scratch : nullptr;
#define CRD_GN_RED(XF, DF, ACT)                                                                                              \
  hipLaunchKernelGGL((k_gn_bwd_reduce<XF, DF, ACT>), grid, dim3(TPB), lds_rows(Cs), as_stream(stream),                     \
                     off_ptr(x, x_f32, x_coff), x_f32, x_ld, off_ptr(dy, dy_f32, dy_coff), dy_f32, dy_ld, (long long)P, C, \
                     Cs, chunk, stats, gmul, gamma, beta, act, mask, r, part)
  switch ((x_f32 ? 4 : 0) | (dy_f32 ? 2 : 0) | (act ? 1 : 0)) {
    case 0: CRD_GN_RED(0, 0, 0); break;  case 1: CRD_GN_RED(0, 0, 1); break;
    case 2: CRD_GN_RED(0, 1, 0); break;  case 3: CRD_GN_RED(0, 1, 1); break;
    case 4: CRD_GN_RED(1, 0, 0); break;  case 5: CRD_GN_RED(1, 0, 1); break;
    case 6: CRD_GN_RED(1, 1, 0); break;  default: CRD_GN_RED(1, 1, 1); break;
  }
#undef CRD_GN_RED
  if (part)
    hipLaunchKernelGGL(k_gn_bwd_finalize, dim3(cdiv(C, 64), B), dim3(TPB), 0, as_stream(stream), scratch, (int)grid.x, C, gmul,
                       gamma, r, B);
  CRD_LAUNCH_CHECK("crd_gn_bwd_reduce");
  return CRD_OK;
}

// The forms crd_gn_bwd_apply[_fp8] can ask for: key = XF | DF << 1 | ACT << 2 | form << 3, form 0..7 = DXF | ACC << 1 | DX2 << 2 and
// form 8 = the e4m3 copy (bf16 dx written once).  One launcher per key, instantiated from the index sequence below.
constexpr int BAP_FORMS = 9, BAP_KEYS = 8 * BAP_FORMS;
typedef void (*bap_launch_t)(dim3, hipStream_t, const BapArgs&);
template <int K>
static void bap_launch(dim3 grid, hipStream_t stream, const BapArgs& a) {
  constexpr int F = K >> 3, F8 = F == 8;
  hipLaunchKernelGGL((k_gn_bwd_apply<K & 1, (K >> 1) & 1, (K >> 2) & 1, F8 ? 0 : (F & 1), F8 ? 0 : ((F >> 1) & 1),
                                     F8 ? 0 : ((F >> 2) & 1), F8>),
                     grid, dim3(TPB), 0, stream, a);
}
template <int... K>
static bap_launch_t bap_pick(int key, std::integer_sequence<int, K...>) {
  static const bap_launch_t tab[] = {bap_launch<K>...};
  return tab[key];
}

static int gn_bwd_apply_impl(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, const void* dy, int32_t dy_f32,
                             int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                             int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask,
                             const crd_sum_t* r, float* dgamma, float* dbeta, void* dx, int32_t dx_f32, int32_t dx_ld,
                             int32_t dx_coff, int32_t dx_accumulate, void* dx2, int32_t dx2_ld, const float* scale2,
                             void* dx8, int32_t dx8_ld, int32_t dx8_coff, const float* scale8, uint32_t* amax8, crd_stream_t stream) {
  unsigned char* dx8p = dx8 ? reinterpret_cast<unsigned char*>(dx8) + dx8_coff : nullptr;
  CRD_CHECK_ARG(x && dy && stats && gamma && beta && r && dx, "crd_gn_bwd_apply: null pointer");
  CRD_CHECK_ARG(!dx2 || dx2_ld % 8 == 0, "crd_gn_bwd_apply: dx2_ld must be a multiple of 8");
  CRD_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "crd_gn_bwd_apply: dgamma and dbeta go together");
  CRD_CHECK_ARG(gmul >= 1 && (C / 16) % gmul == 0, "crd_gn_bwd_apply: bad gmul");
  CRD_CHECK_ARG(dy_ld % 8 == 0 && dy_coff % 8 == 0 && dx_ld % 8 == 0 && dx_coff % 8 == 0,
                "crd_gn_bwd_apply: dy/dx ld/coff must be multiples of 8");
  int rc = check_common("crd_gn_bwd_apply", x_ld, x_coff, C, x_f32);
  if (rc) return rc;
  dim3 grid; int chunk;
  grid_elem(P, C, B, 1, grid, chunk);
  {
    int ld = x_ld > dy_ld ? x_ld : dy_ld;
    if (dx_ld > ld) ld = dx_ld;
    if (dx2 && dx2_ld > ld) ld = dx2_ld;
    if (dx8 && dx8_ld > ld) ld = dx8_ld;
    CRD_GN_CHUNK_FITS("crd_gn_bwd_apply", chunk, ld);
  }
  BapArgs a;
  a.x = off_ptr(x, x_f32, x_coff); a.dy = off_ptr(dy, dy_f32, dy_coff);
  a.stats = stats; a.r = r;
  a.gamma = gamma; a.beta = beta; a.mask = mask; a.scale2 = scale2; a.scale8 = scale8;
  a.dgamma = dgamma; a.dbeta = dbeta;
  a.dx = dx_f32 ? (void*)(reinterpret_cast<float*>(dx) + dx_coff) : (void*)(reinterpret_cast<bf16_t*>(dx) + dx_coff);
  a.dx2 = dx2; a.dx8 = dx8p; a.amax8 = amax8;
  a.P = P;
  a.x_ld = x_ld; a.dy_ld = dy_ld; a.dx_ld = dx_ld; a.dx2_ld = dx2_ld; a.dx8_ld = dx8_ld;
  a.C = C; a.chunk = chunk; a.gmul = gmul; a.B = B;
  const int form = dx8p ? 8 : ((dx_f32 ? 1 : 0) | (dx_accumulate ? 2 : 0) | (dx2 ? 4 : 0));
  const int key = (x_f32 ? 1 : 0) | (dy_f32 ? 2 : 0) | (act ? 4 : 0) | (form << 3);
  bap_pick(key, std::make_integer_sequence<int, BAP_KEYS>())(grid, as_stream(stream), a);
  CRD_LAUNCH_CHECK("crd_gn_bwd_apply");
  return CRD_OK;
}

// The partition crd_gn_apply[_fp8] (kind 0) and crd_gn_bwd_apply[_fp8] (kind 1) use for B samples of P pixels and C channels: nblk
// workgroups per sample of `chunk` pixels each (the last one what is left), batch_pixels = the pixels a workgroup requests at once.
extern "C" int crd_gn_launch_shape(int32_t P, int32_t C, int32_t B, int32_t kind, int32_t* nblk, int32_t* chunk,
                                   int32_t* batch_pixels) {
  CRD_CHECK_ARG(nblk && chunk && batch_pixels, "crd_gn_launch_shape: null pointer");
  CRD_CHECK_ARG(P >= 1 && B >= 1 && (kind == 0 || kind == 1), "crd_gn_launch_shape: P, B >= 1 and kind 0 (apply) or 1 (backward apply)");
  int rc = check_common("crd_gn_launch_shape", 0, 0, C, 0);
  if (rc) return rc;
  long long n, ch, bp;
  gn_elem_shape(P, C, B, kind, n, ch, bp);
  *nblk = (int32_t)n; *chunk = (int32_t)ch; *batch_pixels = (int32_t)bp;
  return CRD_OK;
}

extern "C" int crd_gn_bwd_apply(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, const void* dy, int32_t dy_f32,
                                int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                                int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask,
                                const crd_sum_t* r, float* dgamma, float* dbeta, void* dx, int32_t dx_f32, int32_t dx_ld,
                                int32_t dx_coff, int32_t dx_accumulate, void* dx2, int32_t dx2_ld, const float* scale2,
                                crd_stream_t stream) {
  return gn_bwd_apply_impl(x, x_f32, x_ld, x_coff, dy, dy_f32, dy_ld, dy_coff, B, P, C, stats, gmul, gamma, beta, act, mask, r, dgamma, dbeta,
                           dx, dx_f32, dx_ld, dx_coff, dx_accumulate, dx2, dx2_ld, scale2, nullptr, 0, 0, nullptr, nullptr, stream);
}

extern "C" int crd_gn_bwd_apply_fp8(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, const void* dy, int32_t dy_f32,
                                    int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                                    int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask,
                                    const crd_sum_t* r, float* dgamma, float* dbeta, void* dx, int32_t dx_ld, int32_t dx_coff,
                                    void* dx_fp8, int32_t dx8_ld, int32_t dx8_coff, const float* scale_dev, uint32_t* amax_slots,
                                    crd_stream_t stream) {
  CRD_CHECK_ARG(dx_fp8 && scale_dev && amax_slots && dx8_ld % 8 == 0 && dx8_coff % 8 == 0,
                "crd_gn_bwd_apply_fp8: the e4m3 copy needs its buffer, a device scale and the amax slots (ld / coff multiples of 8)");
  return gn_bwd_apply_impl(x, x_f32, x_ld, x_coff, dy, dy_f32, dy_ld, dy_coff, B, P, C, stats, gmul, gamma, beta, act, mask, r, dgamma, dbeta,
                           dx, 0, dx_ld, dx_coff, 0, nullptr, 0, nullptr, dx_fp8, dx8_ld, dx8_coff, scale_dev, amax_slots, stream);
}
