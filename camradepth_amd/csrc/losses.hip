// Every loss for gfx950 (src/utils/loss_funcs.py:14-91,118-180): the masked depth criteria -- smooth-L1 / MSE partials, L1 / RMSE,
// the reverse Huber (BerHu) -- the edge-aware smoothness loss, and cross entropy with its focal backward.  Conventions: flat fp32
// pred and target, mask target > 0, every cross-workgroup sum a crd_sum_t (CRD_STAT_FRAC_BITS, bit-reproducible and exact under a
// SUM all-reduce), no host synchronisation.  MaskedHuberLoss is nn.HuberLoss(delta=1), i.e. smooth-L1 with beta = 1: it runs
// crd_masked_l1_fwd / _bwd and has no kernel of its own.  All are HBM-bound streaming kernels.
#include <math.h>
#include <string.h>
#include "common.h"

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }   // torch.sgn: 0 at 0

// the depth criteria that share the masked loop of their forward partials and of their backward, d = pred - target
enum { SMOOTH_L1, DIST, BERHU };

// Forward partials over the mask: acc[1] += count, acc[2] += sum d^2, and
//   SMOOTH_L1 (MaskedSmoothL1Loss / MaskedMSELoss, loss_funcs.py:40-46, 83-91): acc[0] += sum of 0.5 d^2 if |d| < 1, else |d| - 0.5
//   DIST (MaskedL1Loss / MaskedRMSELoss): acc[0] += sum |d|
//   BERHU, phase (a): *maxbits = max |d| (the bit pattern of a non-negative float orders like an unsigned integer, so an integer
//   atomic max is exact in any order); acc[0] is left alone
template <int CRIT>
__global__ __launch_bounds__(TPB) void k_masked_fwd(const float* pred, const float* target, long long n, crd_sum_t* acc,
                                                    unsigned int* maxbits) {
  float s = 0.f, cnt = 0.f, sq = 0.f;
  unsigned int mx = 0u;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
    const float t = target[i];
    if (t > 0.f) {
      const float e = pred[i] - t;
      if constexpr (CRIT == SMOOTH_L1) {
        const float ae = fabsf(e);
        s += ae < 1.f ? 0.5f * e * e : ae - 0.5f;
      }
      if constexpr (CRIT == DIST) s += fabsf(e);
      sq += e * e;
      cnt += 1.f;
      if constexpr (CRIT == BERHU) {
        const unsigned int b = __float_as_uint(fabsf(e));
        mx = b > mx ? b : mx;
      }
    }
  }
  if constexpr (CRIT == BERHU) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned int v = (unsigned int)__shfl_xor((int)mx, o);
      mx = v > mx ? v : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(maxbits, mx);
  }
  block_stat_add3(s, cnt, sq, CRIT == BERHU ? nullptr : acc, acc + 1, acc + 2);
}

// Backward of the one-kernel criteria, g = gmul * gout[0] (1 if NULL):
//   SMOOTH_L1: g clamp(d, -1, 1) / count
//   DIST, mode 0 (L1): g sign(d) / count;  mode 1 (RMSE): g d / (count rmse) -- NaN on the mask when rmse = 0, as torch's sqrt backward
template <int CRIT>
__global__ __launch_bounds__(TPB) void k_masked_bwd(const float* pred, const float* target, long long n, const crd_sum_t* acc,
                                                    const float* gout, float gmul, int mode, float* dpred) {
  float g;
  if constexpr (CRIT == SMOOTH_L1) {
    g = gmul * (gout ? gout[0] : 1.f) / stat_get(acc + 1);
  } else {
    const double cnt = (double)acc[1] * (1.0 / STAT_ONE);
    const double rmse = sqrt((double)acc[2] * (1.0 / STAT_ONE) / cnt);
    g = (float)((double)(gmul * (gout ? gout[0] : 1.f)) / (mode == 0 ? cnt : cnt * rmse));
  }
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
    const float t = target[i];
    float d = 0.f;
    if (t > 0.f) {
      const float e = pred[i] - t;
      if constexpr (CRIT == SMOOTH_L1) d = g * fminf(fmaxf(e, -1.f), 1.f);
      else d = mode == 0 ? g * sgnf(e) : g * e;
    }
    dpred[i] = d;
  }
}

// BerHu phase (b) with c = thresh * (global max |d|) formed in fp64 as the reference's delta, the reference's fp32 edges (F.threshold
// compares strictly, against fp32(c) and fp32(c^2)):
//   part1 = |d| if |d| < c, else 0;   part2 = ((|d|^2 - c^2 > 0 ? |d|^2 - c^2 : -c^2) + c^2) / (2c)
// |d|^2 is rounded to fp32 BEFORE the subtraction, as the reference's diff ** 2 is: contracted into one FMA the difference would be
// exact, and at |d| == fp32(c) it is then positive for about a quarter of all c where the reference's is 0.
// loss[0] += sum part1, loss[1] += sum of part2's numerators (the loss is (loss[0] + loss[1] / (2c)) / count: with c = 0 that is
// NaN, as the reference's, without a NaN partial);  dpred = g sign(d) * (1 if |d| < c, |d| / c if |d|^2 - c^2 > 0, else 0) / count.
// Either output may be NULL.
__global__ __launch_bounds__(TPB) void k_berhu(const float* pred, const float* target, long long n, const crd_sum_t* acc,
                                               const unsigned int* maxbits, double thresh, crd_sum_t* loss, const float* gout, float gmul,
                                               float* dpred) {
#pragma clang fp contract(off)      // hipcc contracts a * b - c into one FMA by default (and __fmul_rn is a plain multiply here)
  const double c = thresh * (double)__uint_as_float(*maxbits);
  const float cf = (float)c, c2 = (float)(c * c), inv2c = 1.f / (float)(2.0 * c);
  const float g = dpred ? (float)((double)(gmul * (gout ? gout[0] : 1.f)) / ((double)acc[1] * (1.0 / STAT_ONE))) : 0.f;
  float s1 = 0.f, s2 = 0.f;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
    const float t = target[i];
    float dp = 0.f;
    if (t > 0.f) {
      const float e = pred[i] - t, ad = fabsf(e), v = ad * ad - c2;
      if (ad < cf) {
        s1 += ad;
        dp = g * sgnf(e);
      } else if (v > 0.f) {
        s2 += v + c2;
        dp = g * ((2.f * ad) * inv2c) * sgnf(e);
      }
    }
    if (dpred) dpred[i] = dp;
  }
  if (loss) block_stat_add3(s1, s2, 0.f, loss, loss + 1, nullptr);
}

// SmoothnessLoss, per sample b: acc[3b] += sum p
__global__ __launch_bounds__(TPB) void k_smooth_sum(const float* pred, int HW, crd_sum_t* acc) {
  const int b = blockIdx.y;
  const float* p = pred + (long long)b * HW;
  float s = 0.f;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) s += p[i];
  block_stat_add3(s, 0.f, 0.f, acc + 3 * b, nullptr, nullptr);
}

// edge weights exp(-mean_c |I[i] - I[j]|)
__device__ __forceinline__ float edge_weight(const float* img, long long plane, int C, int i, int j) {
  float s = 0.f;
  for (int ch = 0; ch < C; ++ch) s += fabsf(img[ch * plane + i] - img[ch * plane + j]);
  return expf(-(s / (float)C));
}

__device__ __forceinline__ float smooth_den(const crd_sum_t* acc_b, int HW) {
  return (float)((double)acc_b[0] * (1.0 / STAT_ONE) / (double)HW) + 1e-7f;      // the per-sample mean + 1e-7
}

// acc[3b+1] += sum over x-pairs of w |n_j - n_{j+1}|, acc[3b+2] += the same over y-pairs, n = p / (mean_b + 1e-7)
__global__ __launch_bounds__(TPB) void k_smooth_fwd(const float* pred, const float* image, int C, int H, int W, crd_sum_t* acc) {
  const int b = blockIdx.y, HW = H * W;
  const float* p = pred + (long long)b * HW;
  const float* img = image + (long long)b * C * HW;
  const float den = smooth_den(acc + 3 * b, HW);
  float sx = 0.f, sy = 0.f;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) {
    const int h = i / W, w = i - h * W;
    const float n0 = p[i] / den;
    if (w < W - 1) sx += fabsf(n0 - p[i + 1] / den) * edge_weight(img, HW, C, i, i + 1);
    if (h < H - 1) sy += fabsf(n0 - p[i + W] / den) * edge_weight(img, HW, C, i, i + W);
  }
  block_stat_add3(0.f, sx, sy, nullptr, acc + 3 * b + 1, acc + 3 * b + 2);
}

// dL/dp_k = (dL/dn_k - L_b / HW) / (mean_b + 1e-7): the mean's term needs sum_j dL/dn_j n_j, which is L_b (L is positively
// homogeneous of degree 1 in n), and L_b = sx_b / Nx + sy_b / Ny comes from the forward's per-sample sums
__global__ __launch_bounds__(TPB) void k_smooth_bwd(const float* pred, const float* image, int B, int C, int H, int W,
                                                    const crd_sum_t* acc, const float* gout, float gmul, float* dpred) {
  const int b = blockIdx.y, HW = H * W;
  const float* p = pred + (long long)b * HW;
  const float* img = image + (long long)b * C * HW;
  const double nx = (double)B * H * (W - 1), ny = (double)B * (H - 1) * W;
  const float den = smooth_den(acc + 3 * b, HW);
  const float ix = (float)(1.0 / nx), iy = (float)(1.0 / ny);
  const float lb = (float)(((double)acc[3 * b + 1] / nx + (double)acc[3 * b + 2] / ny) * (1.0 / STAT_ONE) / (double)HW);
  const float g = gmul * (gout ? gout[0] : 1.f);
  for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) {
    const int h = i / W, w = i - h * W;
    const float n0 = p[i] / den;
    float dn = 0.f;
    if (w < W - 1) dn += ix * edge_weight(img, HW, C, i, i + 1) * sgnf(n0 - p[i + 1] / den);
    if (w > 0) dn -= ix * edge_weight(img, HW, C, i - 1, i) * sgnf(p[i - 1] / den - n0);
    if (h < H - 1) dn += iy * edge_weight(img, HW, C, i, i + W) * sgnf(n0 - p[i + W] / den);
    if (h > 0) dn -= iy * edge_weight(img, HW, C, i - W, i) * sgnf(p[i - W] / den - n0);
    dpred[(long long)b * HW + i] = g * (dn - lb) / den;
  }
}

// Cross entropy over NCHW fp32 logits, labels int64 [B][HW], ignore_index 255 (loss_funcs.py:22,27).  Any other label outside
// [0, C) -- torch raises on it -- never forms an address: the pixel adds nothing to the sum or the count and is counted in acc[2]
// (as k_seg_confusion counts it in oor[f]); the callers raise on a non-zero count.  acc is nonnull (crd_ce_fwd refuses NULL): the
// kernel then carries no NULL test for block_stat_add3's first target.
__global__ __launch_bounds__(TPB) void k_ce_fwd(const float* logits, const long long* labels, int C, long long HW, long long rows,
                                                crd_sum_t* acc __attribute__((nonnull))) {
  float s = 0.f, cnt = 0.f, bad = 0.f;
  for (long long r = (long long)blockIdx.x * TPB + threadIdx.x; r < rows; r += (long long)gridDim.x * TPB) {
    const long long lab = labels[r];
    if (lab == 255) continue;
    if (lab < 0 || lab >= C) { bad += 1.f; continue; }
    const long long b = r / HW, p = r - b * HW;
    const float* base = logits + (b * C) * HW + p;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, base[(long long)c * HW]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(base[(long long)c * HW] - mx);
    // log-sum-exp minus the SHIFTED target logit: (mx + log se) - x[lab] would round at the magnitude of the logits themselves
    // (5e-4 per pixel for logits near 1e4), x[lab] - mx is small and nearly exact
    s += logf(se) - (base[lab * HW] - mx);
    cnt += 1.f;
  }
  block_stat_add3(s, cnt, bad, acc, acc + 1, acc + 2);
}

// focal on the scalar mean CE: F=(1-e^-ce)^2 ce ; dF/dce = 2(1-pt)pt ce + (1-pt)^2
__global__ __launch_bounds__(TPB) void k_ce_focal_bwd(const float* logits, const long long* labels, int C, long long HW,
                                                      long long rows, const crd_sum_t* acc, const float* gout, float gmul,
                                                      float* dlogits) {
  const float cnt = stat_get(acc + 1);
  const float ce = stat_get(acc) / cnt;
  const float pt = expf(-ce);
  const float dF = 2.f * (1.f - pt) * pt * ce + (1.f - pt) * (1.f - pt);
  const float g = gmul * (gout ? gout[0] : 1.f) * dF / cnt;
  for (long long r = (long long)blockIdx.x * TPB + threadIdx.x; r < rows; r += (long long)gridDim.x * TPB) {
    const long long lab = labels[r];
    const long long b = r / HW, p = r - b * HW;
    const float* base = logits + (b * C) * HW + p;
    float* dbase = dlogits + (b * C) * HW + p;
    if (lab == 255 || lab < 0 || lab >= C) {      // ignored, or out of range (counted by k_ce_fwd): no gradient
      for (int c = 0; c < C; ++c) dbase[(long long)c * HW] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, base[(long long)c * HW]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(base[(long long)c * HW] - mx);
    const float inv = 1.f / se;
    for (int c = 0; c < C; ++c) {
      float sm = expf(base[(long long)c * HW] - mx) * inv;
      dbase[(long long)c * HW] = g * (sm - (c == lab ? 1.f : 0.f));
    }
  }
}

}  // namespace

extern "C" int crd_masked_l1_fwd(const float* pred, const float* target, int64_t n, crd_sum_t* acc, crd_stream_t stream) {
  CRD_CHECK_ARG(pred && target && acc && n > 0, "crd_masked_l1_fwd: bad argument");
  hipLaunchKernelGGL(k_masked_fwd<SMOOTH_L1>, dim3(blocks_for(n, TPB, 512)), dim3(TPB), 0, as_stream(stream), pred, target,
                     (long long)n, acc, (unsigned int*)nullptr);
  CRD_LAUNCH_CHECK("crd_masked_l1_fwd");
  return CRD_OK;
}

extern "C" int crd_masked_l1_bwd(const float* pred, const float* target, int64_t n, const crd_sum_t* acc, const float* gout,
                                 float gmul, float* dpred, crd_stream_t stream) {
  CRD_CHECK_ARG(pred && target && acc && dpred && n > 0, "crd_masked_l1_bwd: bad argument");
  hipLaunchKernelGGL(k_masked_bwd<SMOOTH_L1>, dim3(blocks_for(n, TPB, 2048)), dim3(TPB), 0, as_stream(stream), pred, target,
                     (long long)n, acc, gout, gmul, 0, dpred);
  CRD_LAUNCH_CHECK("crd_masked_l1_bwd");
  return CRD_OK;
}

extern "C" int crd_masked_dist_fwd(const float* pred, const float* target, int64_t n, crd_sum_t* acc, crd_stream_t stream) {
  CRD_CHECK_ARG(pred && target && acc && n > 0, "crd_masked_dist_fwd: bad argument");
  hipLaunchKernelGGL(k_masked_fwd<DIST>, dim3(blocks_for(n, TPB, 512)), dim3(TPB), 0, as_stream(stream), pred, target, (long long)n, acc,
                     (unsigned int*)nullptr);
  CRD_LAUNCH_CHECK("crd_masked_dist_fwd");
  return CRD_OK;
}

extern "C" int crd_masked_dist_bwd(const float* pred, const float* target, int64_t n, const crd_sum_t* acc, const float* gout,
                                   float gmul, int32_t mode, float* dpred, crd_stream_t stream) {
  CRD_CHECK_ARG(pred && target && acc && dpred && n > 0 && (mode == 0 || mode == 1), "crd_masked_dist_bwd: bad argument");
  hipLaunchKernelGGL(k_masked_bwd<DIST>, dim3(blocks_for(n, TPB, 2048)), dim3(TPB), 0, as_stream(stream), pred, target, (long long)n,
                     acc, gout, gmul, (int)mode, dpred);
  CRD_LAUNCH_CHECK("crd_masked_dist_bwd");
  return CRD_OK;
}

extern "C" int crd_masked_berhu_max(const float* pred, const float* target, int64_t n, crd_sum_t* acc, int32_t* maxbits,
                                    crd_stream_t stream) {
  CRD_CHECK_ARG(pred && target && acc && maxbits && n > 0, "crd_masked_berhu_max: bad argument");
  hipLaunchKernelGGL(k_masked_fwd<BERHU>, dim3(blocks_for(n, TPB, 512)), dim3(TPB), 0, as_stream(stream), pred, target, (long long)n, acc,
                     reinterpret_cast<unsigned int*>(maxbits));
  CRD_LAUNCH_CHECK("crd_masked_berhu_max");
  return CRD_OK;
}

extern "C" int crd_masked_berhu(const float* pred, const float* target, int64_t n, const crd_sum_t* acc, const int32_t* maxbits,
                                uint64_t thresh_f64_bits, crd_sum_t* loss, const float* gout, float gmul, float* dpred, crd_stream_t stream) {
  double thresh;
  memcpy(&thresh, &thresh_f64_bits, sizeof thresh);
  CRD_CHECK_ARG(pred && target && acc && maxbits && n > 0 && (loss || dpred) && thresh > 0.0 && isfinite(thresh),
                "crd_masked_berhu: bad argument");
  hipLaunchKernelGGL(k_berhu, dim3(blocks_for(n, TPB, dpred ? 2048 : 512)), dim3(TPB), 0, as_stream(stream), pred, target, (long long)n,
                     acc, reinterpret_cast<const unsigned int*>(maxbits), thresh, loss, gout, gmul, dpred);
  CRD_LAUNCH_CHECK("crd_masked_berhu");
  return CRD_OK;
}

extern "C" int crd_smoothness_fwd(const float* pred, const float* image, int32_t B, int32_t C, int32_t H, int32_t W, crd_sum_t* acc,
                                  crd_stream_t stream) {
  CRD_CHECK_ARG(pred && image && acc && B > 0 && C > 0 && H > 1 && W > 1 && (int64_t)H * W < (1ll << 31) && B <= 65535,
                "crd_smoothness_fwd: bad argument");
  const int HW = H * W;
  const int nb = blocks_for(HW, TPB, 256);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_smooth_sum, dim3(nb, B), dim3(TPB), 0, st, pred, HW, acc);
  hipLaunchKernelGGL(k_smooth_fwd, dim3(nb, B), dim3(TPB), 0, st, pred, image, (int)C, (int)H, (int)W, acc);
  CRD_LAUNCH_CHECK("crd_smoothness_fwd");
  return CRD_OK;
}

extern "C" int crd_smoothness_bwd(const float* pred, const float* image, int32_t B, int32_t C, int32_t H, int32_t W, const crd_sum_t* acc,
                                  const float* gout, float gmul, float* dpred, crd_stream_t stream) {
  CRD_CHECK_ARG(pred && image && acc && dpred && B > 0 && C > 0 && H > 1 && W > 1 && (int64_t)H * W < (1ll << 31) && B <= 65535,
                "crd_smoothness_bwd: bad argument");
  const int HW = H * W;
  hipLaunchKernelGGL(k_smooth_bwd, dim3(blocks_for(HW, TPB, 256), B), dim3(TPB), 0, as_stream(stream), pred, image, (int)B, (int)C, (int)H,
                     (int)W, acc, gout, gmul, dpred);
  CRD_LAUNCH_CHECK("crd_smoothness_bwd");
  return CRD_OK;
}

extern "C" int crd_ce_fwd(const float* logits, const int64_t* labels, int32_t B, int32_t C, int64_t HW, crd_sum_t* acc,
                          crd_stream_t stream) {
  CRD_CHECK_ARG(logits && labels && acc && B > 0 && C > 0 && HW > 0, "crd_ce_fwd: bad argument");
  const long long rows = (long long)B * HW;
  hipLaunchKernelGGL(k_ce_fwd, dim3(blocks_for(rows, TPB, 1024)), dim3(TPB), 0, as_stream(stream), logits,
                     reinterpret_cast<const long long*>(labels), C, (long long)HW, rows, acc);
  CRD_LAUNCH_CHECK("crd_ce_fwd");
  return CRD_OK;
}

extern "C" int crd_ce_focal_bwd(const float* logits, const int64_t* labels, int32_t B, int32_t C, int64_t HW, const crd_sum_t* acc,
                                const float* gout, float gmul, float* dlogits, crd_stream_t stream) {
  CRD_CHECK_ARG(logits && labels && acc && dlogits && B > 0 && C > 0 && HW > 0, "crd_ce_focal_bwd: bad argument");
  const long long rows = (long long)B * HW;
  hipLaunchKernelGGL(k_ce_focal_bwd, dim3(blocks_for(rows, TPB, 2048)), dim3(TPB), 0, as_stream(stream), logits,
                     reinterpret_cast<const long long*>(labels), C, (long long)HW, rows, acc, gout, gmul, dlogits);
  CRD_LAUNCH_CHECK("crd_ce_focal_bwd");
  return CRD_OK;
}
