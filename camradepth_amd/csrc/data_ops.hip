// Batch assembly on the device: the tensor contract of NuscenesDataset.__getitem__ (src/data/dataloader.py:202-333)
// for the radar configuration the reference trains (image + radar depth + radar flow + radial velocity).  SURVEY 8f N1:
// at a few hundred images/s per GPU the reference's 8 CPU workers become the bottleneck; these are small HBM-bound passes.
#include "common.h"

namespace {

constexpr int TPB = 256;

// out[b][0..2] = (img/255 - mean[c]) / std[c] in the channel order the image was read (cv2: BGR -- the reference applies
// the RGB ImageNet constants to it as is, dataloader.py:226-233); out[3] = clip(radar[...,0], 0, max_depth) / max_depth
// (:304-306); out[4..5] = radar[...,1..2] (:309-310); out[6] = rad_vel (:315-318).  img: uint8 [B][H][W][3], radar: fp32
// [B][H][W][3], rad_vel: fp32 [B][H][W] or NULL (then 6 channels).
__global__ __launch_bounds__(TPB) void k_assemble_input(const unsigned char* img, const float* radar, const float* rad_vel,
                                                        long long HW, float max_depth, int channels, float* out) {
  const int b = blockIdx.y;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  for (long long p = (long long)blockIdx.x * TPB + threadIdx.x; p < HW; p += (long long)gridDim.x * TPB) {
    const unsigned char* ip = img + ((long long)b * HW + p) * 3;
    const float* rp = radar + ((long long)b * HW + p) * 3;
    float* o = out + (long long)b * channels * HW + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * HW] = ((float)ip[c] / 255.f - mean[c]) / stdv[c];
    o[3 * HW] = fminf(fmaxf(rp[0], 0.f), max_depth) / max_depth;
    o[4 * HW] = rp[1];
    o[5 * HW] = rp[2];
    if (rad_vel) o[6 * HW] = rad_vel[(long long)b * HW + p];
  }
}

// Inverse-normalised ground truth (dataloader.py:241-247): g = clip(d, 0, max); g > 0 -> (max - g) / max
__global__ __launch_bounds__(TPB) void k_gt_inverse(const float* depth, long long n, float max_depth, float* out) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
    float g = fminf(fmaxf(depth[i], 0.f), max_depth);
    if (g > 0.f) g = (max_depth - g) * (1.f / max_depth);
    out[i] = g;
  }
}

// The reference's `minpool` (dataloader.py:213-222): zeros become 255, -maxpool(-x) with kernel 3, stride 2, padding 1,
// then 255 back to zero -- the minimum over the valid (non-zero) entries of each 3x3 window, 0 if there are none.
__global__ __launch_bounds__(TPB) void k_gt_minpool(const float* src, int H, int W, float* dst) {
  const int b = blockIdx.y;
  const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
  const float* s = src + (long long)b * H * W;
  float* d = dst + (long long)b * OH * OW;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < OH * OW; i += gridDim.x * TPB) {
    const int oy = i / OW, ox = i - oy * OW;
    float m = 255.f;
#pragma unroll
    for (int ky = -1; ky <= 1; ++ky)
#pragma unroll
      for (int kx = -1; kx <= 1; ++kx) {
        const int y = 2 * oy + ky, x = 2 * ox + kx;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
          float v = s[(long long)y * W + x];
          if (v == 0.f) v = 255.f;
          m = fminf(m, v);
        }
      }
    d[i] = m == 255.f ? 0.f : m;
  }
}

// cv2.resize(img, (DW, DH), interpolation=cv2.INTER_NEAREST) on interleaved uint8 pixels (dataloader.py:227): source
// column = min(floor(dx * ifx), SW - 1) with ifx = 1 / (DW / SW) in double, rows alike (OpenCV resizeNN).
__global__ __launch_bounds__(TPB) void k_resize_nearest_u8(const unsigned char* src, int SH, int SW, int C, unsigned char* dst,
                                                           int DH, int DW) {
  const int b = blockIdx.y;
  const double ifx = 1.0 / ((double)DW / (double)SW), ify = 1.0 / ((double)DH / (double)SH);
  const long long total = (long long)DH * DW;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int dy = (int)(i / DW), dx = (int)(i - (long long)dy * DW);
    int sy = (int)floor(dy * ify), sx = (int)floor(dx * ifx);
    sy = sy < SH - 1 ? sy : SH - 1;
    sx = sx < SW - 1 ? sx : SW - 1;
    const unsigned char* s = src + (((long long)b * SH + sy) * SW + sx) * C;
    unsigned char* d = dst + ((long long)b * total + i) * C;
    for (int c = 0; c < C; ++c) d[c] = s[c];
  }
}

// skimage.transform.resize(mseg[:rows], (DH, DW), order=0, preserve_range=True, anti_aliasing=False) (dataloader.py:262-267;
// scikit-image 0.19.3 = scipy.ndimage.zoom(order=0, grid_mode=True)): source index = floor(((o + 0.5) * (S / D) - 0.5) + 0.5)
// in double.  uint8 label maps in, int64 labels out (what the loss consumes, runner.py:189-190).
__global__ __launch_bounds__(TPB) void k_resize_labels(const unsigned char* src, int SH_full, int SH, int SW, long long* dst,
                                                       int DH, int DW) {
  const int b = blockIdx.y;
  const double zy = (double)SH / (double)DH, zx = (double)SW / (double)DW;
  const long long total = (long long)DH * DW;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int dy = (int)(i / DW), dx = (int)(i - (long long)dy * DW);
    int sy = (int)floor(((dy + 0.5) * zy - 0.5) + 0.5), sx = (int)floor(((dx + 0.5) * zx - 0.5) + 0.5);
    sy = sy < 0 ? 0 : (sy < SH ? sy : SH - 1);
    sx = sx < 0 ? 0 : (sx < SW ? sx : SW - 1);
    dst[(long long)b * total + i] = src[((long long)b * SH_full + sy) * SW + sx];
  }
}

// ---- augmentation (include/camradepth_hip.h, "Batch augmentation on the device") ------------------------------------------------
constexpr int AUG_WORDS = CRD_AUGMENT_WORDS;

// One thread per word of params[B][8]; slot k of sample b is element b * 8 + k of the draw, whatever is enabled.
__global__ __launch_bounds__(TPB) void k_augment_draw(int* params, int B, int ny, int nx, float p_flip, float g_lo, float g_hi,
                                                      float b_lo, float b_hi, float c_lo, float c_hi, int enable,
                                                      unsigned long long seed, unsigned long long counter) {
#pragma clang fp contract(off)          // lo + u * (hi - lo): product and sum rounded on their own
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= B * AUG_WORDS) return;
  const unsigned long long hash = splitmix64(splitmix64(seed ^ (counter * 0xD1342543DE82EF95ull)) + (unsigned long long)i);
  const unsigned long long t = hash >> 40;
  const float u = (float)t * (1.0f / 16777216.0f);
  const int k = i & (AUG_WORDS - 1);
  int word;
  if (k == 0) word = (int)((t * (unsigned long long)ny) >> 24);
  else if (k == 1) word = (int)((t * (unsigned long long)nx) >> 24);
  else if (k == 2) word = u < p_flip ? 1 : 0;
  else {
    const bool on = k == 3 ? (enable & CRD_AUGMENT_GAMMA) : k == 4 ? (enable & CRD_AUGMENT_BRIGHTNESS) : (enable & CRD_AUGMENT_COLOUR);
    const float lo = k == 3 ? g_lo : k == 4 ? b_lo : c_lo, hi = k == 3 ? g_hi : k == 4 ? b_hi : c_hi;
    word = __float_as_int(on ? lo + u * (hi - lo) : 1.0f);
  }
  params[i] = word;
}

// lut[b][c][v]: one workgroup per sample, thread v.  The clamp sits between the last product and the subtraction, so nothing
// here contracts into an fma; with nothing enabled the expression is k_assemble_input's.
__global__ __launch_bounds__(256) void k_augment_lut(const int* params, int enable, float* lut) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, v = threadIdx.x;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const int* pr = params + (long long)b * AUG_WORDS;
  const float gamma = __int_as_float(pr[3]), bright = __int_as_float(pr[4]);
  float t0 = (float)v / 255.f;
  if (enable & CRD_AUGMENT_GAMMA) t0 = powf(t0, gamma);
  if (enable & CRD_AUGMENT_BRIGHTNESS) t0 *= bright;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float t = t0;
    if (enable & CRD_AUGMENT_COLOUR) t *= __int_as_float(pr[5 + c]);
    t = fminf(fmaxf(t, 0.f), 1.f);
    lut[((long long)b * 3 + c) * 256 + v] = (t - mean[c]) / stdv[c];
  }
}

struct AugGeom {
  int y0, x0, flip;
};
// the sample's row of the table, offsets clamped into the frame: no table makes a kernel read outside its sources
__device__ __forceinline__ AugGeom aug_geom(const int* params, int b, int H, int W, int h, int w) {
  const int* pr = params + (long long)b * AUG_WORDS;
  AugGeom g;
  g.y0 = min(max(pr[0], 0), H - h);
  g.x0 = min(max(pr[1], 0), W - w);
  g.flip = pr[2] != 0;
  return g;
}
__device__ __forceinline__ float neg_nonzero(float v) { return v == 0.f ? 0.f : -v; }      // mirrored u; no negative zero
__device__ __forceinline__ long long neg_nonzero(long long v) { return v; }
template <int VEC, typename T>
__device__ __forceinline__ void store_vec(T* p, const T (&v)[VEC]) {
  if constexpr (VEC == 4 && sizeof(T) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);          // w % 4 == 0: 16-byte aligned
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = v[k];
  }
}

struct AugAssembleArgs {
  const unsigned char* img;
  const float *radar, *rad_vel, *depth;
  const unsigned char* seg;
  const int* params;
  const float* lut;
  float *out, *gt;
  long long *fseg, *iseg;
  int H, W, h, w, channels;
  float max_depth;
};

// k_assemble_input + k_gt_inverse + the label gather for the crop window of each sample, in one pass.  A thread makes VEC
// neighbouring output pixels of every plane (VEC = 4 when w % 4 == 0: 16-byte stores); a wave's reads of a source row cover one
// contiguous segment whether the sample is flipped (lanes then run through it backwards) or not.  The sample's 3 x 256 image
// table sits in LDS.
template <int VEC>
__global__ __launch_bounds__(TPB) void k_augment_assemble(AugAssembleArgs a) {
  __shared__ float s_lut[3 * 256];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < 3 * 256; i += TPB) s_lut[i] = a.lut[(long long)b * 3 * 256 + i];
  const AugGeom g = aug_geom(a.params, b, a.H, a.W, a.h, a.w);
  __syncthreads();
  const int h = a.h, w = a.w, wv = w / VEC, ih = h / 2, iw = w / 2;
  const long long HWo = (long long)h * w, total = (long long)h * wv;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int y = (int)(i / wv), x = (int)(i - (long long)y * wv) * VEC;
    const long long srow = ((long long)b * a.H + g.y0 + y) * a.W + g.x0;
    float v[7][VEC], gt[VEC];
    long long lab[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const long long sp = srow + (g.flip ? w - 1 - (x + k) : x + k);
      const unsigned char* ip = a.img + sp * 3;
      const float* rp = a.radar + sp * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][k] = s_lut[c * 256 + ip[c]];
      v[3][k] = fminf(fmaxf(rp[0], 0.f), a.max_depth) / a.max_depth;
      v[4][k] = g.flip ? neg_nonzero(rp[1]) : rp[1];
      v[5][k] = rp[2];
      v[6][k] = a.rad_vel ? a.rad_vel[sp] : 0.f;
      float d = fminf(fmaxf(a.depth[sp], 0.f), a.max_depth);
      if (d > 0.f) d = (a.max_depth - d) * (1.f / a.max_depth);
      gt[k] = d;
      lab[k] = a.seg ? (long long)a.seg[sp] : 0;
    }
    const long long o = (long long)y * w + x;
    float* out = a.out + (long long)b * a.channels * HWo + o;
#pragma unroll
    for (int c = 0; c < 7; ++c)
      if (c < a.channels) store_vec<VEC>(out + c * HWo, v[c]);
    store_vec<VEC>(a.gt + (long long)b * HWo + o, gt);
    if (a.seg) {
      store_vec<VEC>(a.fseg + (long long)b * HWo + o, lab);
      if (a.iseg && (y & 1)) {                    // an odd y < h has y / 2 < h / 2, and so for x: always inside [ih][iw]
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          if ((x + k) & 1) a.iseg[((long long)b * ih + (y >> 1)) * iw + ((x + k) >> 1)] = lab[k];
      }
    }
  }
}

// The geometry alone on `planes` planes per sample: blockIdx.y = b * planes + c.  neg_plane: the plane negated on flipped samples
// (-1: none); half (labels only, or NULL): half[y][x] = dst[2y + 1][2x + 1].
template <int VEC, typename T>
__global__ __launch_bounds__(TPB) void k_augment_gather(const T* src, T* dst, T* half, const int* params, int planes, int H, int W,
                                                        int h, int w, int neg_plane) {
  const int b = blockIdx.y / planes, c = blockIdx.y - b * planes;
  const AugGeom g = aug_geom(params, b, H, W, h, w);
  const bool neg = g.flip && c == neg_plane;
  const int wv = w / VEC, ih = h / 2, iw = w / 2;
  const long long total = (long long)h * wv;
  const T* s = src + ((long long)blockIdx.y * H + g.y0) * W + g.x0;
  T* d = dst + (long long)blockIdx.y * h * w;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int y = (int)(i / wv), x = (int)(i - (long long)y * wv) * VEC;
    T v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const T t = s[(long long)y * W + (g.flip ? w - 1 - (x + k) : x + k)];
      v[k] = neg ? neg_nonzero(t) : t;
    }
    store_vec<VEC>(d + (long long)y * w + x, v);
    if (half && (y & 1)) {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if ((x + k) & 1) half[((long long)blockIdx.y * ih + (y >> 1)) * iw + ((x + k) >> 1)] = v[k];
    }
  }
}

// successive min-pool levels of `src` [B][h][w], down to the first NULL
void launch_minpool_levels(const float* src, int B, int h, int w, float* half, float* quarter, float* eighth, hipStream_t st) {
  float* lv[3] = {half, quarter, eighth};
  for (int i = 0; i < 3 && lv[i]; ++i) {
    const int oh = (h + 2 - 3) / 2 + 1, ow = (w + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(k_gt_minpool, dim3(blocks_for((long long)oh * ow, TPB, 256), B), dim3(TPB), 0, st, src, h, w, lv[i]);
    src = lv[i]; h = oh; w = ow;
  }
}

}  // namespace

extern "C" int crd_assemble_input(const void* img_u8, const float* radar, const float* rad_vel, int32_t B, int32_t H, int32_t W,
                                  float max_depth, float* out, crd_stream_t stream) {
  CRD_CHECK_ARG(img_u8 && radar && out && B > 0 && H > 0 && W > 0 && max_depth > 0.f, "crd_assemble_input: bad argument");
  const long long HW = (long long)H * W;
  hipLaunchKernelGGL(k_assemble_input, dim3(blocks_for(HW, TPB, 1024), B), dim3(TPB), 0, as_stream(stream),
                     reinterpret_cast<const unsigned char*>(img_u8), radar, rad_vel, HW, max_depth, rad_vel ? 7 : 6, out);
  CRD_LAUNCH_CHECK("crd_assemble_input");
  return CRD_OK;
}

extern "C" int crd_gt_pyramid(const float* depth, int32_t B, int32_t H, int32_t W, float max_depth, float* full, float* half,
                              float* quarter, float* eighth, crd_stream_t stream) {
  CRD_CHECK_ARG(depth && full && B > 0 && H > 0 && W > 0 && max_depth > 0.f, "crd_gt_pyramid: bad argument");
  CRD_CHECK_ARG(!(quarter && !half) && !(eighth && !quarter), "crd_gt_pyramid: a level needs the one above it");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_gt_inverse, dim3(blocks_for((long long)B * H * W, TPB, 1024)), dim3(TPB), 0, st, depth, (long long)B * H * W, max_depth, full);
  launch_minpool_levels(full, B, H, W, half, quarter, eighth, st);
  CRD_LAUNCH_CHECK("crd_gt_pyramid");
  return CRD_OK;
}

extern "C" int crd_resize_nearest_u8(const void* src, int32_t B, int32_t SH, int32_t SW, int32_t C, void* dst, int32_t DH, int32_t DW,
                                     crd_stream_t stream) {
  CRD_CHECK_ARG(src && dst && B > 0 && SH > 0 && SW > 0 && C > 0 && DH > 0 && DW > 0, "crd_resize_nearest_u8: bad argument");
  hipLaunchKernelGGL(k_resize_nearest_u8, dim3(blocks_for((long long)DH * DW, TPB, 1024), B), dim3(TPB), 0, as_stream(stream),
                     reinterpret_cast<const unsigned char*>(src), SH, SW, C, reinterpret_cast<unsigned char*>(dst), DH, DW);
  CRD_LAUNCH_CHECK("crd_resize_nearest_u8");
  return CRD_OK;
}

extern "C" int crd_resize_labels_nearest(const void* src_u8, int32_t B, int32_t SH, int32_t SW, int32_t rows, int64_t* dst, int32_t DH,
                                         int32_t DW, crd_stream_t stream) {
  CRD_CHECK_ARG(src_u8 && dst && B > 0 && SH > 0 && SW > 0 && rows > 0 && DH > 0 && DW > 0, "crd_resize_labels_nearest: bad argument");
  hipLaunchKernelGGL(k_resize_labels, dim3(blocks_for((long long)DH * DW, TPB, 1024), B), dim3(TPB), 0, as_stream(stream),
                     reinterpret_cast<const unsigned char*>(src_u8), SH, rows < SH ? rows : SH, SW, reinterpret_cast<long long*>(dst), DH, DW);
  CRD_LAUNCH_CHECK("crd_resize_labels_nearest");
  return CRD_OK;
}

// (h, w) is the whole frame or a crop with sides that are multiples of 32 (the network's stride)
#define CRD_CHECK_CROP(name)                                                                                                      \
  do {                                                                                                                            \
    CRD_CHECK_ARG(B > 0 && H > 0 && W > 0 && h > 0 && w > 0, name ": bad argument (sizes must be positive)");                      \
    CRD_CHECK_ARG(h <= H && w <= W, name ": the crop %d x %d is larger than the frame %d x %d", h, w, H, W);                       \
    CRD_CHECK_ARG((h == H && w == W) || (h % 32 == 0 && w % 32 == 0), name ": the crop %d x %d is not a multiple of 32", h, w);    \
    CRD_CHECK_ARG(B <= 65535 / 8, name ": bad argument (at most %d samples per call)", 65535 / 8);                                 \
  } while (0)

extern "C" int crd_augment_draw(int32_t* params, float* lut, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w, float p_flip,
                                float gamma_lo, float gamma_hi, float brightness_lo, float brightness_hi, float colour_lo,
                                float colour_hi, int32_t enable, uint64_t seed, uint64_t counter, crd_stream_t stream) {
  CRD_CHECK_ARG(params, "crd_augment_draw: null params");
  CRD_CHECK_CROP("crd_augment_draw");
  CRD_CHECK_ARG(p_flip >= 0.f && p_flip <= 1.f, "crd_augment_draw: the flip probability %g is outside [0, 1]", (double)p_flip);
  CRD_CHECK_ARG((enable & ~7) == 0, "crd_augment_draw: bad argument (enable has unknown bits)");
  // (a NaN bound fails the comparisons)
  CRD_CHECK_ARG(!(enable & CRD_AUGMENT_GAMMA) || (gamma_lo > 0.f && gamma_lo <= gamma_hi && gamma_hi < INFINITY),
                "crd_augment_draw: bad gamma range (%g, %g): 0 < lo <= hi", (double)gamma_lo, (double)gamma_hi);
  CRD_CHECK_ARG(!(enable & CRD_AUGMENT_BRIGHTNESS) || (brightness_lo >= 0.f && brightness_lo <= brightness_hi && brightness_hi < INFINITY),
                "crd_augment_draw: bad brightness range (%g, %g): 0 <= lo <= hi", (double)brightness_lo, (double)brightness_hi);
  CRD_CHECK_ARG(!(enable & CRD_AUGMENT_COLOUR) || (colour_lo >= 0.f && colour_lo <= colour_hi && colour_hi < INFINITY),
                "crd_augment_draw: bad colour range (%g, %g): 0 <= lo <= hi", (double)colour_lo, (double)colour_hi);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_augment_draw, dim3(blocks_for((long long)B * AUG_WORDS, TPB, 1024)), dim3(TPB), 0, st, params, B, H - h + 1, W - w + 1, p_flip,
                     gamma_lo, gamma_hi, brightness_lo, brightness_hi, colour_lo, colour_hi, enable,
                     (unsigned long long)(seed ^ CRD_AUGMENT_STREAM), (unsigned long long)counter);
  if (lut) hipLaunchKernelGGL(k_augment_lut, dim3(B), dim3(256), 0, st, params, enable, lut);
  CRD_LAUNCH_CHECK("crd_augment_draw");
  return CRD_OK;
}

extern "C" int crd_augment_lut(const int32_t* params, int32_t B, int32_t enable, float* lut, crd_stream_t stream) {
  CRD_CHECK_ARG(params && lut, "crd_augment_lut: null pointer");
  CRD_CHECK_ARG(B > 0 && (enable & ~7) == 0, "crd_augment_lut: bad argument");
  hipLaunchKernelGGL(k_augment_lut, dim3(B), dim3(256), 0, as_stream(stream), params, enable, lut);
  CRD_LAUNCH_CHECK("crd_augment_lut");
  return CRD_OK;
}

extern "C" int crd_augment_assemble(const void* img_u8, const float* radar, const float* rad_vel, const float* depth, const void* seg_u8,
                                    const int32_t* params, const float* lut, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w,
                                    float max_depth, float* out, float* gt_full, int64_t* final_seg, int64_t* inter_seg,
                                    crd_stream_t stream) {
  CRD_CHECK_ARG(img_u8 && radar && depth && params && lut && out && gt_full, "crd_augment_assemble: null pointer");
  CRD_CHECK_ARG(!seg_u8 || final_seg, "crd_augment_assemble: null final_seg (labels were given)");
  CRD_CHECK_ARG(seg_u8 || (!final_seg && !inter_seg), "crd_augment_assemble: null seg_u8 (label outputs were given)");
  CRD_CHECK_CROP("crd_augment_assemble");
  CRD_CHECK_ARG(max_depth > 0.f, "crd_augment_assemble: bad argument (max_depth must be positive)");
  AugAssembleArgs a;
  a.img = reinterpret_cast<const unsigned char*>(img_u8); a.radar = radar; a.rad_vel = rad_vel; a.depth = depth;
  a.seg = reinterpret_cast<const unsigned char*>(seg_u8); a.params = params; a.lut = lut; a.out = out; a.gt = gt_full;
  a.fseg = reinterpret_cast<long long*>(final_seg); a.iseg = reinterpret_cast<long long*>(inter_seg);
  a.H = H; a.W = W; a.h = h; a.w = w; a.channels = rad_vel ? 7 : 6; a.max_depth = max_depth;
  if (w % 4 == 0)
    hipLaunchKernelGGL(k_augment_assemble<4>, dim3(blocks_for((long long)h * (w / 4), TPB, 1024), B), dim3(TPB), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(k_augment_assemble<1>, dim3(blocks_for((long long)h * w, TPB, 1024), B), dim3(TPB), 0, as_stream(stream), a);
  CRD_LAUNCH_CHECK("crd_augment_assemble");
  return CRD_OK;
}

template <typename T>
static void launch_augment_gather(const T* src, T* dst, T* half, const int32_t* params, int B, int planes, int H, int W, int h, int w,
                                  int neg_plane, hipStream_t st) {
  if (w % 4 == 0)
    hipLaunchKernelGGL((k_augment_gather<4, T>), dim3(blocks_for((long long)h * (w / 4), TPB, 1024), B * planes), dim3(TPB), 0, st, src, dst, half,
                       params, planes, H, W, h, w, neg_plane);
  else
    hipLaunchKernelGGL((k_augment_gather<1, T>), dim3(blocks_for((long long)h * w, TPB, 1024), B * planes), dim3(TPB), 0, st, src, dst, half, params,
                       planes, H, W, h, w, neg_plane);
}

extern "C" int crd_augment_gather(const float* image, const float* gt_full, const int64_t* seg, const int32_t* params, int32_t B,
                                  int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, float* image_out, float* gt_out,
                                  int64_t* seg_out, int64_t* inter_out, crd_stream_t stream) {
  CRD_CHECK_ARG(image && gt_full && params && image_out && gt_out, "crd_augment_gather: null pointer");
  CRD_CHECK_ARG(!seg || seg_out, "crd_augment_gather: null seg_out (labels were given)");
  CRD_CHECK_ARG(seg || (!seg_out && !inter_out), "crd_augment_gather: null seg (label outputs were given)");
  CRD_CHECK_ARG(C > 0 && C <= 8, "crd_augment_gather: bad argument (1 to 8 channels)");
  CRD_CHECK_CROP("crd_augment_gather");
  hipStream_t st = as_stream(stream);
  launch_augment_gather<float>(image, image_out, nullptr, params, B, C, H, W, h, w, C >= 6 ? 4 : -1, st);
  launch_augment_gather<float>(gt_full, gt_out, nullptr, params, B, 1, H, W, h, w, -1, st);
  if (seg)
    launch_augment_gather<long long>(reinterpret_cast<const long long*>(seg), reinterpret_cast<long long*>(seg_out),
                                     reinterpret_cast<long long*>(inter_out), params, B, 1, H, W, h, w, -1, st);
  CRD_LAUNCH_CHECK("crd_augment_gather");
  return CRD_OK;
}

extern "C" int crd_gt_pyramid_from_full(const float* full, int32_t B, int32_t H, int32_t W, float* half, float* quarter, float* eighth,
                                        crd_stream_t stream) {
  CRD_CHECK_ARG(full && half && B > 0 && H > 0 && W > 0, "crd_gt_pyramid_from_full: bad argument");
  CRD_CHECK_ARG(!(eighth && !quarter), "crd_gt_pyramid_from_full: a level needs the one above it");
  launch_minpool_levels(full, B, H, W, half, quarter, eighth, as_stream(stream));
  CRD_LAUNCH_CHECK("crd_gt_pyramid_from_full");
  return CRD_OK;
}
