// Evaluation kernels for gfx950: the metrics of Trainer.test (crd_test_metrics, crd_seg_confusion) and the standard
// depth-evaluation sums, binned by true distance (include/camradepth_hip.h: crd_depth_eval), where one HBM-bound pass over
// prediction and ground truth serves every distance cap and every metric.
#include <math.h>
#include "common.h"

namespace {

constexpr int TPB = 256;

// The metrics of Trainer.test.  They stay ABOVE the fp contract(off) pragma below: they are compiled with the default contraction
// (sq += e * e is one FMA), as they always were, and crd_test_metrics' sums keep their bits that way.

// Trainer.test metrics (runner.py:443-465), per frame f: pred clipped to [0,1] and both scaled by max_depth, ground truth
// beyond max_distance dropped; acc[f] = (sum |e|, sum e^2, sum |e|/gt, count)
__global__ __launch_bounds__(TPB) void k_test_metrics(const float* pred, const float* gt, long long n, float max_depth,
                                                      float max_distance, crd_sum_t* acc) {
  const int f = blockIdx.y;
  const float* p = pred + (long long)f * n;
  const float* g = gt + (long long)f * n;
  float sa = 0.f, sq = 0.f, sr = 0.f, cnt = 0.f;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
    float t = g[i] * max_depth;
    if (t > max_distance) t = 0.f;
    if (t > 0.f) {
      const float e = fminf(fmaxf(p[i], 0.f), 1.f) * max_depth - t;
      sa += fabsf(e); sq += e * e; sr += fabsf(e) / t; cnt += 1.f;
    }
  }
  sa = wave_sum(sa); sq = wave_sum(sq); sr = wave_sum(sr); cnt = wave_sum(cnt);
  __shared__ float sm[TPB / 64][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[wave][0] = sa; sm[wave][1] = sq; sm[wave][2] = sr; sm[wave][3] = cnt; }
  __syncthreads();
  if (threadIdx.x < 4) {
    float v = 0.f;
    for (int w = 0; w < TPB / 64; ++w) v += sm[w][threadIdx.x];
    stat_add(&acc[f * 4 + threadIdx.x], v);
  }
}

// Confusion matrix of one frame for the Jaccard index of Trainer.test (runner.py:432-436): prediction = arg-max over the C
// logits of a pixel (NCHW fp32, first maximal class), confmat[f][target][pred] += 1; labels outside [0, C) are counted in
// oor[f] and skipped (torchmetrics 0.10.2 raises on them, which the reference catches: that frame's IoU stays NaN).
__global__ __launch_bounds__(TPB) void k_seg_confusion(const float* logits, const long long* labels, int C, long long HW,
                                                       unsigned long long* confmat, unsigned long long* oor) {
  extern __shared__ unsigned int hist[];      // C * C + 1
  const int f = blockIdx.y;
  for (int i = threadIdx.x; i <= C * C; i += TPB) hist[i] = 0;
  __syncthreads();
  const float* lg = logits + (long long)f * C * HW;
  const long long* lb = labels + (long long)f * HW;
  for (long long p = (long long)blockIdx.x * TPB + threadIdx.x; p < HW; p += (long long)gridDim.x * TPB) {
    const long long t = lb[p];
    if (t < 0 || t >= C) { atomicAdd(&hist[C * C], 1u); continue; }
    float best = lg[p];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = lg[(long long)c * HW + p];
      if (v > best) { best = v; arg = c; }
    }
    atomicAdd(&hist[(int)t * C + arg], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += TPB)
    if (hist[i]) atomicAdd(&confmat[(long long)f * C * C + i], (unsigned long long)hist[i]);
  if (threadIdx.x == 0 && hist[C * C]) atomicAdd(&oor[f], (unsigned long long)hist[C * C]);
}

}  // namespace

extern "C" int crd_test_metrics(const float* pred, const float* gt, int32_t frames, int64_t n, float max_depth, float max_distance,
                                crd_sum_t* acc, crd_stream_t stream) {
  CRD_CHECK_ARG(pred && gt && acc && frames > 0 && n > 0, "crd_test_metrics: bad argument");
  hipLaunchKernelGGL(k_test_metrics, dim3(blocks_for(n, TPB, 64), frames), dim3(TPB), 0, as_stream(stream), pred, gt, (long long)n,
                     max_depth, max_distance, acc);
  CRD_LAUNCH_CHECK("crd_test_metrics");
  return CRD_OK;
}

extern "C" int crd_seg_confusion(const float* logits, const int64_t* labels, int32_t frames, int32_t C, int64_t HW, int64_t* confmat,
                                 int64_t* out_of_range, crd_stream_t stream) {
  CRD_CHECK_ARG(logits && labels && confmat && out_of_range && frames > 0 && C > 0 && C <= 64 && HW > 0, "crd_seg_confusion: bad argument");
  hipLaunchKernelGGL(k_seg_confusion, dim3(blocks_for(HW, TPB, 128), frames), dim3(TPB), (C * C + 1) * sizeof(unsigned int), as_stream(stream),
                     logits, reinterpret_cast<const long long*>(labels), C, (long long)HW,
                     reinterpret_cast<unsigned long long*>(confmat), reinterpret_cast<unsigned long long*>(out_of_range));
  CRD_LAUNCH_CHECK("crd_seg_confusion");
  return CRD_OK;
}

// From here on the per-pixel arithmetic is part of the contract (every statement rounded on its own in fp32): no fused
// multiply-adds.
#pragma clang fp contract(off)

namespace {

constexpr int PIX_PER_THREAD = 8;                // two 16-byte loads of each input per thread
constexpr int CHUNK = TPB * PIX_PER_THREAD;      // pixels of one workgroup: a contiguous piece of one frame
constexpr int COLS = CRD_EVAL_COLUMNS;

template <int C> constexpr float eval_one() { return (float)(1ll << CRD_EVAL_FRAC_BITS[C]); }

// A thread's sums for the bin of the pixels it saw last.  Neighbouring pixels of a depth map mostly share a bin, so a thread adds
// in registers and goes to the workgroup's table only when the bin changes: with every pixel valid and in one bin the table would
// otherwise take 12 same-address LDS atomics per pixel.  Integer adds: the grouping does not change the total.
struct EvalAcc {
  int bin;
  unsigned cnt, d1, d2, d3;
  long long s[8];            // columns 1..8
};

__device__ __forceinline__ void lds_add(unsigned long long* t, unsigned long long v) {
  if (v) atomicAdd(t, v);
}

__device__ __forceinline__ void eval_flush(unsigned long long* tab, EvalAcc& a) {
  if (a.cnt == 0) return;
  unsigned long long* t = tab + a.bin * COLS;
  atomicAdd(t, (unsigned long long)a.cnt);
#pragma unroll
  for (int k = 0; k < 8; ++k) { lds_add(t + 1 + k, (unsigned long long)a.s[k]); a.s[k] = 0; }
  lds_add(t + 9, a.d1); lds_add(t + 10, a.d2); lds_add(t + 11, a.d3);
  a.cnt = a.d1 = a.d2 = a.d3 = 0;
}

// One pixel with a lidar hit (g > 0 was the caller's compare).
__device__ __forceinline__ void eval_pixel(float p, float g, float max_depth, float min_depth, float bin_width, int last_bin,
                                           EvalAcc& a, unsigned long long* tab) {
  const float dg = max_depth * (1.0f - g);
  if (!(dg >= min_depth)) return;
  // clamps as selects: a NaN prediction stays NaN (fminf / fmaxf would replace it by the bound) and ends in the sticky flag
  const float pc = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);
  const float dr = max_depth * (1.0f - pc);
  const float dp = dr < min_depth ? min_depth : (dr > max_depth ? max_depth : dr);
  int b = (int)floorf(dg / bin_width);
  b = b < last_bin ? b : last_bin;
  if (b != a.bin) { eval_flush(tab, a); a.bin = b; }
  const float e = dp - dg, ae = fabsf(e), e2 = e * e;
  const float r = logf(dp) - logf(dg);
  const float q = 1.0f / dp - 1.0f / dg;
  const float m = fmaxf(dp / dg, dg / dp);
  a.cnt += 1;
  a.s[0] += to_fx(ae, eval_one<1>());
  a.s[1] += to_fx(e2, eval_one<2>());
  a.s[2] += to_fx(ae / dg, eval_one<3>());
  a.s[3] += to_fx(e2 / dg, eval_one<4>());
  a.s[4] += to_fx(r, eval_one<5>());
  a.s[5] += to_fx(r * r, eval_one<6>());
  a.s[6] += to_fx(fabsf(q), eval_one<7>());
  a.s[7] += to_fx(q * q, eval_one<8>());
  a.d1 += m < 1.25f ? 1u : 0u;
  a.d2 += m < 1.5625f ? 1u : 0u;
  a.d3 += m < 1.953125f ? 1u : 0u;
}

// grid (chunks, frames).  VEC: n a multiple of 4 and both inputs 16-byte aligned, so every frame starts on a 16-byte boundary and a
// 16-byte load is all inside the frame or all outside it.  The prediction is read only where the ground truth has a hit: lidar
// ground truth is sparse, and a pixel without a hit costs its load and one compare.
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_depth_eval(const float* __restrict__ pred, const float* __restrict__ gt, long long n,
                                                    float max_depth, float min_depth, float bin_width, int n_bins, crd_sum_t* acc) {
  __shared__ unsigned long long tab[CRD_EVAL_MAX_BINS * COLS];
  const int cells = n_bins * COLS;
  for (int i = threadIdx.x; i < cells; i += TPB) tab[i] = 0;
  __syncthreads();
  const long long frame = blockIdx.y;
  const float* p = pred + frame * n;
  const float* g = gt + frame * n;
  const long long c0 = (long long)blockIdx.x * CHUNK;
  const int last_bin = n_bins - 1;
  EvalAcc a = {};
  if (VEC) {
    float4 gv[PIX_PER_THREAD / 4];
#pragma unroll
    for (int j = 0; j < PIX_PER_THREAD / 4; ++j) {
      const long long i = c0 + (long long)(j * TPB + (int)threadIdx.x) * 4;
      gv[j] = i < n ? *reinterpret_cast<const float4*>(g + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < PIX_PER_THREAD / 4; ++j) {
      if (gv[j].x > 0.f || gv[j].y > 0.f || gv[j].z > 0.f || gv[j].w > 0.f) {
        const long long i = c0 + (long long)(j * TPB + (int)threadIdx.x) * 4;
        const float4 pv = *reinterpret_cast<const float4*>(p + i);
        if (gv[j].x > 0.f) eval_pixel(pv.x, gv[j].x, max_depth, min_depth, bin_width, last_bin, a, tab);
        if (gv[j].y > 0.f) eval_pixel(pv.y, gv[j].y, max_depth, min_depth, bin_width, last_bin, a, tab);
        if (gv[j].z > 0.f) eval_pixel(pv.z, gv[j].z, max_depth, min_depth, bin_width, last_bin, a, tab);
        if (gv[j].w > 0.f) eval_pixel(pv.w, gv[j].w, max_depth, min_depth, bin_width, last_bin, a, tab);
      }
    }
  } else {
    float gs[PIX_PER_THREAD];
#pragma unroll
    for (int j = 0; j < PIX_PER_THREAD; ++j) {
      const long long i = c0 + j * TPB + (int)threadIdx.x;
      gs[j] = i < n ? g[i] : 0.f;
    }
#pragma unroll 4
    for (int j = 0; j < PIX_PER_THREAD; ++j) {
      if (gs[j] > 0.f) {
        const long long i = c0 + j * TPB + (int)threadIdx.x;
        eval_pixel(p[i], gs[j], max_depth, min_depth, bin_width, last_bin, a, tab);
      }
    }
  }
  eval_flush(tab, a);
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += TPB) {
    const unsigned long long v = tab[i];
    if (v) fx_add(acc + frame * cells + i, (long long)v);
  }
}

inline bool pos_finite(float v) { return isfinite(v) && v > 0.f; }

}  // namespace

extern "C" int crd_depth_eval(const float* pred, const float* gt, int32_t frames, int64_t n, float max_depth, float min_depth,
                              float bin_width, int32_t n_bins, crd_sum_t* acc, crd_stream_t stream) {
  CRD_CHECK_ARG(pred, "crd_depth_eval: pred is null");
  CRD_CHECK_ARG(gt, "crd_depth_eval: gt is null");
  CRD_CHECK_ARG(acc, "crd_depth_eval: acc is null");
  CRD_CHECK_ARG(frames > 0, "crd_depth_eval: frames = %d must be positive", (int)frames);
  CRD_CHECK_ARG(n > 0, "crd_depth_eval: n = %lld must be positive", (long long)n);
  CRD_CHECK_ARG(pos_finite(max_depth), "crd_depth_eval: max_depth = %g must be finite and > 0", (double)max_depth);
  CRD_CHECK_ARG(pos_finite(min_depth), "crd_depth_eval: min_depth = %g must be finite and > 0", (double)min_depth);
  CRD_CHECK_ARG(pos_finite(bin_width), "crd_depth_eval: bin_width = %g must be finite and > 0", (double)bin_width);
  CRD_CHECK_ARG(min_depth < max_depth, "crd_depth_eval: min_depth = %g must be below max_depth = %g", (double)min_depth, (double)max_depth);
  CRD_CHECK_ARG(n_bins >= 1 && n_bins <= CRD_EVAL_MAX_BINS, "crd_depth_eval: n_bins = %d outside 1..%d (CRD_EVAL_MAX_BINS)", (int)n_bins,
                CRD_EVAL_MAX_BINS);
  CRD_CHECK_ARG((float)n_bins == ceilf(max_depth / bin_width), "crd_depth_eval: n_bins = %d is not ceil(max_depth / bin_width) = %g",
                (int)n_bins, (double)ceilf(max_depth / bin_width));
  CRD_UNSUPPORTED(frames <= 65535, "crd_depth_eval: frames = %d exceeds 65535 per call", (int)frames);
  CRD_UNSUPPORTED(n < (1ll << 35), "crd_depth_eval: n = %lld exceeds 2^35 pixels per frame", (long long)n);
  const dim3 grid((unsigned)((n + CHUNK - 1) / CHUNK), (unsigned)frames);
  const bool vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(k_depth_eval<true>, grid, dim3(TPB), 0, as_stream(stream), pred, gt, (long long)n, max_depth, min_depth,
                       bin_width, (int)n_bins, acc);
  else
    hipLaunchKernelGGL(k_depth_eval<false>, grid, dim3(TPB), 0, as_stream(stream), pred, gt, (long long)n, max_depth, min_depth,
                       bin_width, (int)n_bins, acc);
  CRD_LAUNCH_CHECK("crd_depth_eval");
  return CRD_OK;
}
