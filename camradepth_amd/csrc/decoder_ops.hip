// Decoder-side streaming kernels for gfx950: layout conversion at the module boundary, Seg_Block argmax, the depth head's
// stencils, slice copies and small elementwise helpers.  (Bicubic x2 and its transpose: bicubic.hip.)
#include "common.h"

namespace {

constexpr int TPB = 256;

__global__ __launch_bounds__(TPB) void k_nchw_to_pm(const float* x, int C, long long HW, bf16_t* y, int y_ld, int Cpad) {
  const int b = blockIdx.y;
  const int CG = Cpad >> 3;
  const long long total = HW * CG;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const long long p = i % HW;          // pixel fastest: coalesced reads of each channel plane
    const int cg = (int)(i / HW);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cg * 8 + j;
      v[j] = c < C ? x[((long long)b * C + c) * HW + p] : 0.f;
    }
    store8_bf16(y, ((long long)b * HW + p) * y_ld + cg * 8, v);
  }
}

__global__ __launch_bounds__(TPB) void k_pm_to_nchw(const void* x, int x_f32, int x_ld, int C, long long HW, float* y) {
  const int b = blockIdx.y;
  const long long total = HW * C;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const long long p = i % HW;
    const int c = (int)(i / HW);
    const long long off = ((long long)b * HW + p) * x_ld + c;
    y[((long long)b * C + c) * HW + p] = x_f32 ? reinterpret_cast<const float*>(x)[off] : bf2f(reinterpret_cast<const bf16_t*>(x)[off]);
  }
}

__global__ __launch_bounds__(TPB) void k_scale_f32(const float* src, float* dst, long long n, float scale) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) dst[i] = scale * src[i];
}

__global__ __launch_bounds__(TPB) void k_seg_argmax(const float* logits, int ld, long long rows, int C, int num_classes,
                                                    void* y, int y_f32, int y_ld) {
  for (long long r = (long long)blockIdx.x * TPB + threadIdx.x; r < rows; r += (long long)gridDim.x * TPB) {
    const float* p = logits + r * ld;
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      float v = p[c];
      if (v > best) { best = v; bi = c; }
    }
    const float v = (float)bi / (float)num_classes;
    if (y_f32) reinterpret_cast<float*>(y)[r * y_ld] = v;
    else reinterpret_cast<bf16_t*>(y)[r * y_ld] = f2bf(v);
  }
}

__global__ __launch_bounds__(TPB) void k_slice_copy(const bf16_t* src, int s_ld, bf16_t* dst, int d_ld, long long rows, int C,
                                                    int accumulate) {
  const int CG = C >> 3;
  const long long total = rows * CG;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int cg = (int)(i % CG);
    const long long r = i / CG;
    uint4 u = *reinterpret_cast<const uint4*>(src + r * s_ld + cg * 8);
    if (accumulate) {
      float a[8], o[8];
      load8(src, r * s_ld + cg * 8, 0, a);
      load8(dst, r * d_ld + cg * 8, 0, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += o[j];
      store8_bf16(dst, r * d_ld + cg * 8, a);
    } else {
      *reinterpret_cast<uint4*>(dst + r * d_ld + cg * 8) = u;
    }
  }
}

// dst[r][c] = bf16(scale[r / rows_per_sample] * src[r*s_ld + c] + add[r*add_ld + c]) for c < C
__global__ __launch_bounds__(TPB) void k_f32_to_bf16_rows(const float* src, int s_ld, bf16_t* dst, int d_ld, long long rows,
                                                          int C, const float* scale, long long rows_per_sample,
                                                          const bf16_t* add, int add_ld, int vec) {
  if (vec) {  // C % 8 == 0 and all strides / offsets 8-aligned
    const int CG = C >> 3;
    const long long total = rows * CG;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
      const int cg = (int)(i % CG);
      const long long r = i / CG;
      const float s = scale ? scale[r / rows_per_sample] : 1.f;
      float v[8];
      load8(src, r * s_ld + cg * 8, 1, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= s;
      if (add) {
        float a[8];
        load8(add, r * add_ld + cg * 8, 0, a);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += a[j];
      }
      store8_bf16(dst, r * d_ld + cg * 8, v);
    }
    return;
  }
  const long long total = rows * C;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int c = (int)(i % C);
    const long long r = i / C;
    float s = scale ? scale[r / rows_per_sample] : 1.f;
    float v = s * src[r * s_ld + c];
    if (add) v += bf2f(add[r * add_ld + c]);
    dst[r * d_ld + c] = f2bf(v);
  }
}

// dz = da * a * (1-a), in place on da (bf16 contiguous)
__global__ __launch_bounds__(TPB) void k_sigmoid_bwd(const bf16_t* a, bf16_t* da, long long n8) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n8; i += (long long)gridDim.x * TPB) {
    float av[8], dv[8];
    load8(a, i * 8, 0, av);
    load8(da, i * 8, 0, dv);
#pragma unroll
    for (int j = 0; j < 8; ++j) dv[j] *= av[j] * (1.f - av[j]);
    store8_bf16(da, i * 8, dv);
  }
}

// ------------------------------------------------------------------------------------------------
// Depth_Activation.conv_2 (utils.py:283,288): 3x3, 32 -> 1 channel.  A GEMM tile would be 1/32 full, so this is a
// stencil-reduce: 4 lanes per pixel (8 channels each), weights in registers, HBM-bound on the 32-channel input.
// w is the reference layout fp32 [1][32][3][3] (index c*9 + tap), rounded to bf16 on load like autocast does.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_head2_fwd(const bf16_t* a, const float* w, const float* bias, int H, int W,
                                                   float* depth, bf16_t* copy, int copy_ld) {
  const int b = blockIdx.y, q = threadIdx.x & 3;
  // the 72 weights of this lane's 8 channels: loaded once, the thread then walks over many pixels (one pixel per thread
  // spent 8x more loads on the weights than on the data)
  float wv[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[t][j] = bf_round(w[(q * 8 + j) * 9 + t]);
  const float bias0 = bias[0];
  const bf16_t* ab = a + (long long)b * H * W * 32 + q * 8;
  const int npix = H * W, stride = (gridDim.x * TPB) >> 2;
  for (int pix = (blockIdx.x * TPB + threadIdx.x) >> 2; pix < npix; pix += stride) {     // uniform per 4-lane pixel group
    const int py = pix / W, px = pix - py * W;
    // the nine taps from clamped addresses, all in flight, zeroed by a select outside the image (under `if (inside) load` every
    // tap's load was waited for before the next was issued: nine dependent memory latencies per pixel)
    uint4 tv[9];
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = py + t / 3 - 1, ix = px + t % 3 - 1;
      in[t] = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const int cy = iy < 0 ? 0 : (iy < H ? iy : H - 1), cx = ix < 0 ? 0 : (ix < W ? ix : W - 1);
      tv[t] = *reinterpret_cast<const uint4*>(ab + ((long long)cy * W + cx) * 32);
    }
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint4 u = in[t] ? tv[t] : make_uint4(0, 0, 0, 0);
      acc += bf_lo(u.x) * wv[t][0]; acc += bf_hi(u.x) * wv[t][1]; acc += bf_lo(u.y) * wv[t][2]; acc += bf_hi(u.y) * wv[t][3];
      acc += bf_lo(u.z) * wv[t][4]; acc += bf_hi(u.z) * wv[t][5]; acc += bf_lo(u.w) * wv[t][6]; acc += bf_hi(u.w) * wv[t][7];
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    if (q == 0) {
      const float r = bf_round(acc + bias0);
      depth[(long long)b * npix + pix] = r;
      if (copy) copy[((long long)b * npix + pix) * copy_ld] = f2bf(r);
    }
  }
}

// dz[p][c] = a(1-a) * sum_tap dy[p - off(tap)] * w[c][tap],  dy = gd (+ add)
__global__ __launch_bounds__(TPB) void k_head2_bwd_data(const float* gd, const bf16_t* add, int add_ld, const bf16_t* a,
                                                        const float* w, int H, int W, bf16_t* dz) {
  const int b = blockIdx.y, q = threadIdx.x & 3;
  float wv[9][8];                                           // loaded once per thread, as in k_head2_fwd
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[t][j] = bf_round(w[(q * 8 + j) * 9 + t]);
  const float* gb = gd + (long long)b * H * W;
  const bf16_t* addb = add ? add + (long long)b * H * W * add_ld : nullptr;
  const int npix = H * W, stride = (gridDim.x * TPB) >> 2;
  for (int pix = (blockIdx.x * TPB + threadIdx.x) >> 2; pix < npix; pix += stride) {
    const int py = pix / W, px = pix - py * W;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    // (the nine taps from clamped addresses, all in flight, zeroed by a select outside the image: as in k_head2_fwd)
    float dyv[9];
    long long oc[9];
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int oy = py + 1 - t / 3, ox = px + 1 - t % 3;
      in[t] = (unsigned)oy < (unsigned)H && (unsigned)ox < (unsigned)W;
      const int cy = oy < 0 ? 0 : (oy < H ? oy : H - 1), cx = ox < 0 ? 0 : (ox < W ? ox : W - 1);
      oc[t] = (long long)cy * W + cx;
      dyv[t] = gb[oc[t]];
    }
    if (addb) {                                             // (kernel argument: uniform)
      bf16_t av9[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) av9[t] = addb[oc[t] * add_ld];
#pragma unroll
      for (int t = 0; t < 9; ++t) dyv[t] += bf2f(av9[t]);
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float dv = in[t] ? bf_round(dyv[t]) : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += dv * wv[t][j];
    }
    float av[8];
    const long long off = ((long long)b * npix + pix) * 32 + q * 8;
    load8(a, off, 0, av);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= av[j] * (1.f - av[j]);
    store8_bf16(dz, off, acc);
  }
}

// rows[r][c*9 + tap] += sum_p dy[p] * a[p + off(tap)][c] ; rows[r][288] += sum_p dy[p], r = workgroup % replicas.
// The 289 sums of a workgroup are folded with shuffles (pixel lanes of a wave) and four LDS rounds (waves); with one
// accumulator for all 2048 workgroups the chain of contended atomics (2048 x 32 per 128-byte line x 2.6 ns) was the
// whole 170 us of this kernel, hence the copies (crd_wgrad_unpack sums them).
__global__ __launch_bounds__(TPB) void k_head2_wgrad(const float* gd, const bf16_t* add, int add_ld, const bf16_t* a, int H, int W,
                                                     int chunk, crd_sum_t* rows, int replicas) {
  __shared__ float sm[9 * 32 + 1];
  const int b = blockIdx.y, q = threadIdx.x & 3, pl = threadIdx.x >> 2;
  const float* gb = gd + (long long)b * H * W;
  const bf16_t* addb = add ? add + (long long)b * H * W * add_ld : nullptr;
  const bf16_t* ab = a + (long long)b * H * W * 32 + q * 8;
  float acc[9][8], bs = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;
  int p0 = blockIdx.x * chunk, p1 = p0 + chunk;
  if (p1 > H * W) p1 = H * W;
  for (int pix = p0 + pl; pix < p1; pix += TPB / 4) {
    const int py = pix / W, px = pix - py * W;
    float dyv = gb[pix];
    if (addb) dyv += bf2f(addb[(long long)pix * add_ld]);
    dyv = bf_round(dyv);
    bs += dyv;
    // all nine taps requested before the first is used: unconditional loads from a clamped address, the tap's weight selected
    // (under `if (in the image) load` every tap was waited for before the next was issued: 94 us for 27 MB at 256 x 416 x 8)
    uint4 raw[9];
    float wt[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = py + ky - 1, ix = px + kx - 1;
        const int cy = iy < 0 ? 0 : (iy < H ? iy : H - 1), cx = ix < 0 ? 0 : (ix < W ? ix : W - 1);
        raw[ky * 3 + kx] = *reinterpret_cast<const uint4*>(ab + ((long long)cy * W + cx) * 32);
        wt[ky * 3 + kx] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? dyv : 0.f;
      }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint4 u = raw[t];
      const float v[8] = {bf_lo(u.x), bf_hi(u.x), bf_lo(u.y), bf_hi(u.y), bf_lo(u.z), bf_hi(u.z), bf_lo(u.w), bf_hi(u.w)};
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[t][j] += wt[t] * v[j];
    }
  }
  // pixel lanes of the wave (lane bits 2..5)
  for (int o = 4; o < 64; o <<= 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[t][j] += __shfl_xor(acc[t][j], o);
    bs += __shfl_xor(bs, o);
  }
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int w = 0; w < TPB / 64; ++w) {
    if (wave == w && l < 4) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float* p = &sm[t * 32 + q * 8 + j];
          *p = w == 0 ? acc[t][j] : *p + acc[t][j];
        }
      if (l == 0) sm[288] = w == 0 ? bs : sm[288] + bs;
    }
    __syncthreads();
  }
  crd_sum_t* dst = rows + (long long)((blockIdx.y * gridDim.x + blockIdx.x) % replicas) * 289;
  for (int i = threadIdx.x; i < 288; i += TPB) grad_add(&dst[(i & 31) * 9 + (i >> 5)], sm[i]);
  if (threadIdx.x == 0) grad_add(&dst[288], sm[288]);
}

// workgroups per sample of the head stencil kernels: 4 lanes per pixel, ~8+ pixels per thread on large grids
inline int head2_blocks(int H, int W, int B) {
  long long n = cdiv(4ll * H * W, TPB);
  long long cap = 4096 / (B > 0 ? B : 1);
  if (cap < 1) cap = 1;
  return (int)(n > cap ? cap : n);
}

}  // namespace

extern "C" int crd_nchw_to_pm(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, void* y, int32_t y_ld, int32_t y_coff,
                              int32_t Cpad, crd_stream_t stream) {
  CRD_CHECK_ARG(x && y, "crd_nchw_to_pm: null pointer");
  CRD_CHECK_ARG(Cpad % 8 == 0 && Cpad >= C && y_ld % 8 == 0 && y_coff % 8 == 0, "crd_nchw_to_pm: alignment");
  const long long HW = (long long)H * W;
  hipLaunchKernelGGL(k_nchw_to_pm, dim3(blocks_for(HW * (Cpad / 8), TPB, 4096), B), dim3(TPB), 0, as_stream(stream), x, C, HW,
                     reinterpret_cast<bf16_t*>(y) + y_coff, y_ld, Cpad);
  CRD_LAUNCH_CHECK("crd_nchw_to_pm");
  return CRD_OK;
}

extern "C" int crd_pm_to_nchw(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t C, int32_t H,
                              int32_t W, float* y, crd_stream_t stream) {
  CRD_CHECK_ARG(x && y, "crd_pm_to_nchw: null pointer");
  const long long HW = (long long)H * W;
  const void* xp = x_f32 ? (const void*)(reinterpret_cast<const float*>(x) + x_coff) : (const void*)(reinterpret_cast<const bf16_t*>(x) + x_coff);
  hipLaunchKernelGGL(k_pm_to_nchw, dim3(blocks_for(HW * C, TPB, 4096), B), dim3(TPB), 0, as_stream(stream), xp, x_f32, x_ld, C, HW, y);
  CRD_LAUNCH_CHECK("crd_pm_to_nchw");
  return CRD_OK;
}

extern "C" int crd_seg_argmax(const void* logits, int32_t ld, int32_t B, int32_t P, int32_t C, int32_t num_classes, void* y,
                              int32_t y_f32, int32_t y_ld, int32_t y_coff, crd_stream_t stream) {
  CRD_CHECK_ARG(logits && y && C >= 1 && num_classes >= 1, "crd_seg_argmax: bad argument");
  const long long rows = (long long)B * P;
  void* yp = y_f32 ? (void*)(reinterpret_cast<float*>(y) + y_coff) : (void*)(reinterpret_cast<bf16_t*>(y) + y_coff);
  hipLaunchKernelGGL(k_seg_argmax, dim3(blocks_for(rows, TPB, 4096)), dim3(TPB), 0, as_stream(stream), reinterpret_cast<const float*>(logits),
                     ld, rows, C, num_classes, yp, y_f32, y_ld);
  CRD_LAUNCH_CHECK("crd_seg_argmax");
  return CRD_OK;
}

extern "C" int crd_scale_f32(const float* src, float* dst, int64_t n, float scale, crd_stream_t stream) {
  CRD_CHECK_ARG(src && dst && n > 0, "crd_scale_f32: bad argument");
  hipLaunchKernelGGL(k_scale_f32, dim3(blocks_for(n, TPB, 4096)), dim3(TPB), 0, as_stream(stream), src, dst, (long long)n, scale);
  CRD_LAUNCH_CHECK("crd_scale_f32");
  return CRD_OK;
}

extern "C" int crd_slice_copy(const void* src, int32_t s_ld, int32_t s_coff, void* dst, int32_t d_ld, int32_t d_coff,
                              int64_t rows, int32_t C, int32_t accumulate, crd_stream_t stream) {
  CRD_CHECK_ARG(src && dst, "crd_slice_copy: null pointer");
  CRD_CHECK_ARG(C % 8 == 0 && s_ld % 8 == 0 && s_coff % 8 == 0 && d_ld % 8 == 0 && d_coff % 8 == 0, "crd_slice_copy: alignment");
  hipLaunchKernelGGL(k_slice_copy, dim3(blocks_for(rows * (C / 8), TPB, 4096)), dim3(TPB), 0, as_stream(stream),
                     reinterpret_cast<const bf16_t*>(src) + s_coff, s_ld, reinterpret_cast<bf16_t*>(dst) + d_coff, d_ld,
                     (long long)rows, C, accumulate);
  CRD_LAUNCH_CHECK("crd_slice_copy");
  return CRD_OK;
}

extern "C" int crd_f32_to_bf16_rows(const float* src, int32_t s_ld, void* dst, int32_t d_ld, int32_t d_coff, int64_t rows,
                                    int32_t C, const float* scale, int64_t rows_per_sample, const void* add, int32_t add_ld,
                                    int32_t add_coff, crd_stream_t stream) {
  CRD_CHECK_ARG(src && dst && rows_per_sample > 0, "crd_f32_to_bf16_rows: bad argument");
  const int vec = (C % 8 == 0) && (s_ld % 8 == 0) && (d_ld % 8 == 0) && (d_coff % 8 == 0) &&
                  (!add || (add_ld % 8 == 0 && add_coff % 8 == 0)) && ((reinterpret_cast<uintptr_t>(src) & 31) == 0);
  hipLaunchKernelGGL(k_f32_to_bf16_rows, dim3(blocks_for(vec ? rows * (C / 8) : rows * C, TPB, 4096)), dim3(TPB), 0, as_stream(stream), src,
                     s_ld, reinterpret_cast<bf16_t*>(dst) + d_coff, d_ld, (long long)rows, C, scale, (long long)rows_per_sample,
                     add ? reinterpret_cast<const bf16_t*>(add) + add_coff : nullptr, add_ld, vec);
  CRD_LAUNCH_CHECK("crd_f32_to_bf16_rows");
  return CRD_OK;
}

extern "C" int crd_head_conv2_fwd(const void* a, const float* w, const float* bias, int32_t B, int32_t H, int32_t W, float* depth,
                                  void* copy, int32_t copy_ld, int32_t copy_coff, crd_stream_t stream) {
  CRD_CHECK_ARG(a && w && bias && depth, "crd_head_conv2_fwd: null pointer");
  hipLaunchKernelGGL(k_head2_fwd, dim3((unsigned)head2_blocks(H, W, B), B), dim3(TPB), 0, as_stream(stream),
                     reinterpret_cast<const bf16_t*>(a), w, bias, H, W, depth,
                     copy ? reinterpret_cast<bf16_t*>(copy) + copy_coff : nullptr, copy_ld);
  CRD_LAUNCH_CHECK("crd_head_conv2_fwd");
  return CRD_OK;
}

static int head2_bwd_launch(const float* gd, const void* add, int32_t add_ld, int32_t add_coff, const void* a, const float* w,
                            int32_t B, int32_t H, int32_t W, void* dz, crd_sum_t* dw_rows, int32_t replicas, int parts,
                            const char* who, crd_stream_t stream) {
  CRD_CHECK_ARG(gd && a && (!(parts & 1) || (w && dz)) && (!(parts & 2) || (dw_rows && replicas >= 1)), "%s: null pointer / replicas < 1", who);
  const bf16_t* addp = add ? reinterpret_cast<const bf16_t*>(add) + add_coff : nullptr;
  hipStream_t st = as_stream(stream);
  if (parts & 1)
    hipLaunchKernelGGL(k_head2_bwd_data, dim3((unsigned)head2_blocks(H, W, B), B), dim3(TPB), 0, st, gd, addp, add_ld,
                       reinterpret_cast<const bf16_t*>(a), w, H, W, reinterpret_cast<bf16_t*>(dz));
  if (parts & 2) {
    const int P = H * W;
    int nblk = cdiv(P, 64 * 4);
    int cap = 2048 / (B > 0 ? B : 1); if (cap < 1) cap = 1;
    if (nblk > cap) nblk = cap;
    const int chunk = cdiv(P, nblk);
    nblk = cdiv(P, chunk);
    hipLaunchKernelGGL(k_head2_wgrad, dim3(nblk, B), dim3(TPB), 0, st, gd, addp, add_ld, reinterpret_cast<const bf16_t*>(a), H, W, chunk,
                       dw_rows, replicas);
  }
  CRD_LAUNCH_CHECK(who);
  return CRD_OK;
}

extern "C" int crd_head_conv2_bwd(const float* gd, const void* add, int32_t add_ld, int32_t add_coff, const void* a, const float* w,
                                  int32_t B, int32_t H, int32_t W, void* dz, crd_sum_t* dw_rows, int32_t replicas,
                                  crd_stream_t stream) {
  return head2_bwd_launch(gd, add, add_ld, add_coff, a, w, B, H, W, dz, dw_rows, replicas, 3, "crd_head_conv2_bwd", stream);
}

extern "C" int crd_head_conv2_bwd_data(const float* gd, const void* add, int32_t add_ld, int32_t add_coff, const void* a,
                                       const float* w, int32_t B, int32_t H, int32_t W, void* dz, crd_stream_t stream) {
  return head2_bwd_launch(gd, add, add_ld, add_coff, a, w, B, H, W, dz, nullptr, 0, 1, "crd_head_conv2_bwd_data", stream);
}

extern "C" int crd_head_conv2_wgrad(const float* gd, const void* add, int32_t add_ld, int32_t add_coff, const void* a, int32_t B,
                                    int32_t H, int32_t W, crd_sum_t* dw_rows, int32_t replicas, crd_stream_t stream) {
  return head2_bwd_launch(gd, add, add_ld, add_coff, a, nullptr, B, H, W, nullptr, dw_rows, replicas, 2, "crd_head_conv2_wgrad", stream);
}

extern "C" int crd_sigmoid_bwd(const void* a, void* da, int64_t n, crd_stream_t stream) {
  CRD_CHECK_ARG(a && da && n % 8 == 0, "crd_sigmoid_bwd: bad argument");
  hipLaunchKernelGGL(k_sigmoid_bwd, dim3(blocks_for(n / 8, TPB, 4096)), dim3(TPB), 0, as_stream(stream), reinterpret_cast<const bf16_t*>(a),
                     reinterpret_cast<bf16_t*>(da), (long long)(n / 8));
  CRD_LAUNCH_CHECK("crd_sigmoid_bwd");
  return CRD_OK;
}
