// Visualisation back end on the device: float maps, label maps and the radar channel -> uint8 RGB pictures, and the label map of
// the segmentation logits.  The arithmetic is specified operation by operation in include/camradepth_hip.h ("Visualisation back end")
// and restated in NumPy by tests/viz_ref.py; kernels and restatement agree bit for bit.  crd_viz_range: the per-frame range in two
// launches (per-tile partials, one workgroup per frame folds them), no atomic and no workgroup waiting on another; crd_viz_draw: one
// launch that reads map and image once and writes four pixels as three dwords; crd_seg_labels: one launch.
#include "common.h"
#include <string.h>

// every fp32 / fp64 operation is rounded on its own, as NumPy does it
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int PER = 4;                         // consecutive pixels per thread: 16 bytes of a float map in, 12 bytes of a picture out
constexpr int TILE = TPB * PER;                // pixels per workgroup of the range pass: CRD_VIZ_TILE
constexpr int WAVES = TPB / CRD_WAVE;
static_assert(TILE == CRD_VIZ_TILE, "include/camradepth_hip.h states the tile size");

inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }      // false for NaN as well

// fp32 values as unsigned keys that order as the values do (-0.0 below +0.0): minimum and maximum become integer operations, which
// do not depend on the order of arrival and have no NaN or signed-zero cases.
__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float of_key(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
constexpr unsigned KEY_NONE_LO = 0xffffffffu, KEY_NONE_HI = 0u;      // lo > hi: no finite value seen

// (lo, hi) of the workgroup in thread 0
__device__ __forceinline__ void block_min_max(unsigned& lo, unsigned& hi, unsigned (&lo_s)[WAVES], unsigned (&hi_s)[WAVES]) {
#pragma unroll
  for (int o = CRD_WAVE / 2; o > 0; o >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
  }
  if ((threadIdx.x & (CRD_WAVE - 1)) == 0) { lo_s[threadIdx.x / CRD_WAVE] = lo; hi_s[threadIdx.x / CRD_WAVE] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) { lo = min(lo, lo_s[wv]); hi = max(hi, hi_s[wv]); }
  }
}

// ---- range ------------------------------------------------------------------------------------------------------------------
struct Range {
  const void* src;             // fp32 (KIND 0, 2) or uint8 (KIND 1) [B][h][w]
  float* dilated;              // KIND 2: fp32 [B][h][w], written here
  int h, w, per, tiles_per_frame, rad, vec;
};

// the radar panel's map: 1 - r where there is a return
__device__ __forceinline__ float radar_t(float r) { return (r != 0.f && finite_f(r)) ? 1.f - r : 0.f; }

// The dilated radar map at the n <= PER pixels j0 .. of one frame (frame: its first pixel).  Pixels that share a row share the window's
// rows: k * (k + 3) loads for four pixels.
__device__ __forceinline__ void dilate_quad(const Range& a, const float* frame, int j0, int n, float (&m)[PER]) {
  const int r0 = j0 / a.w, c0 = j0 - r0 * a.w, rad = a.rad;
#pragma unroll
  for (int q = 0; q < PER; ++q) m[q] = -INFINITY;
  if (c0 + n <= a.w) {
    for (int rr = max(r0 - rad, 0); rr <= min(r0 + rad, a.h - 1); ++rr) {
      const float* row = frame + (long long)rr * a.w;
      for (int cc = max(c0 - rad, 0); cc <= min(c0 + n - 1 + rad, a.w - 1); ++cc) {
        const float t = radar_t(row[cc]);
        const int dx = cc - c0;
#pragma unroll
        for (int q = 0; q < PER; ++q)
          if (dx - q >= -rad && dx - q <= rad) m[q] = fmaxf(m[q], t);
      }
    }
  } else {
    for (int q = 0; q < n; ++q) {
      const int r = (j0 + q) / a.w, c = (j0 + q) - r * a.w;
      for (int rr = max(r - rad, 0); rr <= min(r + rad, a.h - 1); ++rr)
        for (int cc = max(c - rad, 0); cc <= min(c + rad, a.w - 1); ++cc) m[q] = fmaxf(m[q], radar_t(frame[(long long)rr * a.w + cc]));
    }
  }
}

// Launch 1: partials[tile] = the keys of the smallest and the largest finite value among the tile's pixels.  Tile t of the launch is
// tile t % tiles_per_frame of frame t / tiles_per_frame: no tile straddles two frames.  KIND 0: a float map; 1: labels; 2: the radar
// channel, whose dilated map is written on the way and is what the range is taken of.
template <int KIND>
__global__ __launch_bounds__(TPB) void k_viz_partials(Range a, uint2* partials) {
  __shared__ unsigned lo_s[WAVES], hi_s[WAVES];
  const int tile = blockIdx.x, b = tile / a.tiles_per_frame;
  const int j0 = (tile - b * a.tiles_per_frame) * TILE + threadIdx.x * PER;
  const int n = min(PER, a.per - j0);                                  // <= 0: nothing of this thread's lies in the frame
  const long long base = (long long)b * a.per;
  float v[PER] = {0.f, 0.f, 0.f, 0.f};
  if (n > 0) {
    if (KIND == 2) {
      dilate_quad(a, reinterpret_cast<const float*>(a.src) + base, j0, n, v);
      if (a.vec) *reinterpret_cast<float4*>(a.dilated + base + j0) = make_float4(v[0], v[1], v[2], v[3]);
      else for (int k = 0; k < n; ++k) a.dilated[base + j0 + k] = v[k];
    } else if (KIND == 0) {
      const float* p = reinterpret_cast<const float*>(a.src) + base + j0;
      if (a.vec) { const float4 f = *reinterpret_cast<const float4*>(p); v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w; }
      else for (int k = 0; k < n; ++k) v[k] = p[k];
    } else {
      const unsigned char* p = reinterpret_cast<const unsigned char*>(a.src) + base + j0;
      if (a.vec) {
        const unsigned u = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
        for (int k = 0; k < PER; ++k) v[k] = (float)((u >> (8 * k)) & 0xffu);
      } else for (int k = 0; k < n; ++k) v[k] = (float)p[k];
    }
  }
  unsigned lo = KEY_NONE_LO, hi = KEY_NONE_HI;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (k < n && finite_f(v[k])) {
      const unsigned key = key_of(v[k]);
      lo = min(lo, key); hi = max(hi, key);
    }
  }
  block_min_max(lo, hi, lo_s, hi_s);
  if (threadIdx.x == 0) partials[tile] = make_uint2(lo, hi);
}

// Launch 2, one workgroup per frame: range[b] = (vmin, vmax) from the frame's partials; (0, 0) for a frame without a finite value.
__global__ __launch_bounds__(TPB) void k_viz_fold(const uint2* partials, int tiles_per_frame, float* range) {
  __shared__ unsigned lo_s[WAVES], hi_s[WAVES];
  const int b = blockIdx.x;
  unsigned lo = KEY_NONE_LO, hi = KEY_NONE_HI;
  for (int i = threadIdx.x; i < tiles_per_frame; i += TPB) {
    const uint2 p = partials[(long long)b * tiles_per_frame + i];
    lo = min(lo, p.x); hi = max(hi, p.y);
  }
  block_min_max(lo, hi, lo_s, hi_s);
  if (threadIdx.x == 0) {
    const bool any = lo <= hi;
    range[2 * b] = any ? of_key(lo) : 0.f;
    range[2 * b + 1] = any ? of_key(hi) : 0.f;
  }
}

// ---- drawing ----------------------------------------------------------------------------------------------------------------
struct Draw {
  const void* src;             // fp32 (kind 0) or uint8 (kind 1) [B][h][w]; unused in mode CRD_VIZ_IMAGE
  const unsigned char* table;  // [256][3]
  const float* range;          // [B][2] or NULL: vmin, vmax below
  const unsigned char* image;  // [B][h][w][3] or NULL
  unsigned char* out;
  long long row_pitch, frame_pitch;
  int h, w, quads_per_row, kind, mode, bgr, grey;
  float vmin, vmax, alpha, beta;
  unsigned bad;                // R | G << 8 | B << 16
};

// the table row of the scaled value y: NaN -> 0
template <class T>
__device__ __forceinline__ int row_of(T y) { return y >= (T)256 ? 255 : (y >= (T)0 ? (int)y : 0); }

__device__ __forceinline__ unsigned blend_channel(unsigned img, unsigned col, float alpha, float beta) {
  const float t = (float)img * alpha;
  const float u = (float)col * beta;
  const float s = t + u;
  return (unsigned)fminf(fmaxf(rintf(s), 0.f), 255.f);
}

// One thread draws the (up to) four pixels c0 .. c0 + 3 of one row.  VEC: w is a multiple of four and every pointer and pitch is
// aligned (the host decides), so the map is one 16-byte (4-byte for labels) load, the image three dword loads, the picture three dword
// stores; otherwise scalar loads and byte stores.  The table sits in LDS as one packed dword per row.
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_viz_draw(Draw a, long long n_quads) {
  __shared__ unsigned lut[256];
  if (a.mode != CRD_VIZ_IMAGE) {
    const unsigned char* e = a.table + 3 * threadIdx.x;
    lut[threadIdx.x] = (unsigned)e[0] | ((unsigned)e[1] << 8) | ((unsigned)e[2] << 16);
  }
  __syncthreads();
  const long long q = (long long)blockIdx.x * TPB + threadIdx.x;
  if (q >= n_quads) return;
  const long long row = q / a.quads_per_row;                          // b * h + r
  const int c0 = (int)(q - row * a.quads_per_row) * PER;
  const int n = VEC ? PER : min(PER, a.w - c0);
  const int b = (int)(row / a.h), r = (int)(row - (long long)b * a.h);
  const long long pix = row * a.w + c0;

  unsigned colour[PER] = {0u, 0u, 0u, 0u};
  bool above[PER] = {false, false, false, false};                    // x > 0: where paste takes the colour
  if (a.mode != CRD_VIZ_IMAGE) {
    const float vmin = a.range ? a.range[2 * b] : a.vmin, vmax = a.range ? a.range[2 * b + 1] : a.vmax;
    const bool flat = vmin == vmax;
    if (a.kind == 0) {
      float x[PER] = {0.f, 0.f, 0.f, 0.f};
      const float* p = reinterpret_cast<const float*>(a.src) + pix;
      if (VEC) { const float4 f = *reinterpret_cast<const float4*>(p); x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w; }
      else for (int k = 0; k < n; ++k) x[k] = p[k];
      const double lo = (double)vmin, d = (double)vmax - (double)vmin;          // the range is held in fp64, the map in fp32
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const float t = (float)((double)x[k] - lo);
        const float qn = (float)((double)t / d);
        const float y = qn * 256.f;
        colour[k] = finite_f(x[k]) ? lut[flat ? 0 : row_of(y)] : a.bad;
        above[k] = x[k] > 0.f;
      }
    } else {
      unsigned l = 0;
      const unsigned char* p = reinterpret_cast<const unsigned char*>(a.src) + pix;
      if (VEC) l = *reinterpret_cast<const unsigned*>(p);
      else for (int k = 0; k < n; ++k) l |= (unsigned)p[k] << (8 * k);
      const double lo = (double)vmin, d = (double)vmax - (double)vmin;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const unsigned lk = (l >> (8 * k)) & 0xffu;
        const double y = ((double)lk - lo) / d * 256.0;
        colour[k] = lut[flat ? 0 : row_of(y)];
        above[k] = lk > 0u;
      }
    }
  }

  unsigned px[PER];                                                   // R | G << 8 | B << 16 of the pixels drawn
  if (a.mode == CRD_VIZ_NONE) {
#pragma unroll
    for (int k = 0; k < PER; ++k) px[k] = colour[k];
  } else {
    unsigned w3[3] = {0u, 0u, 0u};                                    // the image's 12 bytes
    const unsigned char* ip = a.image + pix * 3;
    if (VEC) {
      const unsigned* iw = reinterpret_cast<const unsigned*>(ip);
      w3[0] = iw[0]; w3[1] = iw[1]; w3[2] = iw[2];
    } else {
      for (int k = 0; k < 3 * n; ++k) w3[k >> 2] |= (unsigned)ip[k] << (8 * (k & 3));
    }
    const unsigned raw[PER] = {w3[0] & 0xffffffu, (w3[0] >> 24) | ((w3[1] & 0xffffu) << 8), (w3[1] >> 16) | ((w3[2] & 0xffu) << 16), w3[2] >> 8};
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      unsigned c0_ = raw[k] & 0xffu, c1 = (raw[k] >> 8) & 0xffu, c2 = (raw[k] >> 16) & 0xffu;
      if (a.bgr) { const unsigned t = c0_; c0_ = c2; c2 = t; }        // now R, G, B
      if (a.grey) c0_ = c1 = c2 = (c0_ * 9798u + c1 * 19235u + c2 * 3735u + 16384u) >> 15;
      if (a.mode == CRD_VIZ_BLEND) {
        c0_ = blend_channel(c0_, colour[k] & 0xffu, a.alpha, a.beta);
        c1 = blend_channel(c1, (colour[k] >> 8) & 0xffu, a.alpha, a.beta);
        c2 = blend_channel(c2, (colour[k] >> 16) & 0xffu, a.alpha, a.beta);
      }
      const unsigned img = c0_ | (c1 << 8) | (c2 << 16);
      px[k] = (a.mode == CRD_VIZ_PASTE && above[k]) ? colour[k] : img;
    }
  }

  unsigned char* o = a.out + (long long)b * a.frame_pitch + (long long)r * a.row_pitch + (long long)c0 * 3;
  const unsigned o3[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
  if (VEC) {
    unsigned* ow = reinterpret_cast<unsigned*>(o);
    ow[0] = o3[0]; ow[1] = o3[1]; ow[2] = o3[2];
  } else {
    for (int k = 0; k < 3 * n; ++k) o[k] = (unsigned char)(o3[k >> 2] >> (8 * (k & 3)));
  }
}

// ---- labels from logits -----------------------------------------------------------------------------------------------------
// Four consecutive pixels of one frame per thread, the channel planes read one after the other: every load of a wave is 1 KiB in a row.
// The comparison runs on integer keys that order as np.argmax does -- -0.0 and 0.0 equal, every NaN alike and above +inf -- so "strictly
// larger replaces" is the first maximum and the first NaN.  (Written with float comparisons, `v > best || (v != v && best == best)`,
// the compiler kept the old best in the lanes that took a NaN, and a later channel replaced it.)
__device__ __forceinline__ unsigned argmax_key(float v) {
  unsigned u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;            // NaN
  if (u == 0x80000000u) u = 0u;                                       // -0.0 == 0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(TPB) void k_seg_labels(const float* logits, int C, int per, int quads_per_frame, long long n_quads, int vec,
                                                    unsigned char* labels) {
  const long long q = (long long)blockIdx.x * TPB + threadIdx.x;
  if (q >= n_quads) return;
  const int b = (int)(q / quads_per_frame), j0 = (int)(q - (long long)b * quads_per_frame) * PER;
  const int n = min(PER, per - j0);
  const float* p = logits + (long long)b * C * per + j0;
  unsigned best[PER] = {0u, 0u, 0u, 0u};                              // below the key of every value: channel 0 always takes
  unsigned idx = 0;
  for (int c = 0; c < C; ++c, p += per) {
    float v[PER] = {0.f, 0.f, 0.f, 0.f};
    if (vec) { const float4 f = *reinterpret_cast<const float4*>(p); v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w; }
    else for (int k = 0; k < n; ++k) v[k] = p[k];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const unsigned key = argmax_key(v[k]);
      const bool take = key > best[k];
      best[k] = take ? key : best[k];
      idx = take ? ((idx & ~(0xffu << (8 * k))) | ((unsigned)c << (8 * k))) : idx;
    }
  }
  unsigned char* o = labels + (long long)b * per + j0;
  if (vec) *reinterpret_cast<unsigned*>(o) = idx;
  else for (int k = 0; k < n; ++k) o[k] = (unsigned char)(idx >> (8 * k));
}

// B, h, w of an entry: CRD_OK, or the status to return
int check_shape(const char* name, int32_t B, int32_t h, int32_t w) {
  CRD_CHECK_ARG(B > 0 && h > 0 && w > 0, "%s: bad argument (B %d, map %d x %d)", name, B, h, w);
  const long long per = (long long)h * w;
  CRD_UNSUPPORTED(per <= 0x7fffffffll - TILE && B * ((per + TILE - 1) / TILE) <= 0x7fffffffll && B * ((long long)h * ((w + 3) / 4)) <=
                  0x7fffffffll * TPB, "%s: unsupported shape (B %d, map %d x %d: more pixels than the 32-bit indices hold)", name, B, h, w);
  return CRD_OK;
}

}  // namespace

extern "C" int crd_viz_range(const void* src, int32_t kind, int32_t B, int32_t h, int32_t w, int32_t dilate, float* dilated, void* workspace,
                             int64_t workspace_bytes, float* range, crd_stream_t stream) {
  const int rc = check_shape("crd_viz_range", B, h, w);
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(kind == CRD_VIZ_FLOAT || kind == CRD_VIZ_LABELS, "crd_viz_range: bad argument (kind %d is neither 0, float, nor 1, labels)", kind);
  CRD_CHECK_ARG(dilate == 0 || (dilate >= 1 && dilate <= 9 && (dilate & 1)), "crd_viz_range: bad argument (dilate %d is not 0 or odd in 1 .. 9)",
                dilate);
  CRD_CHECK_ARG(dilate == 0 || kind == CRD_VIZ_FLOAT, "crd_viz_range: bad argument (dilate %d with labels)", dilate);
  CRD_CHECK_ARG(src && workspace && range, "crd_viz_range: null pointer (src, workspace, range)");
  CRD_CHECK_ARG(dilate == 0 || dilated, "crd_viz_range: null pointer (dilated, with dilate %d)", dilate);
  Range a;
  a.src = src; a.dilated = dilated; a.h = h; a.w = w; a.per = h * w; a.tiles_per_frame = (a.per + TILE - 1) / TILE; a.rad = dilate / 2;
  const long long n_tiles = (long long)B * a.tiles_per_frame;
  CRD_CHECK_ARG(workspace_bytes >= 8 * n_tiles, "crd_viz_range: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                8 * n_tiles);
  CRD_CHECK_ARG(aligned(workspace, 8) && aligned(range, 4) && aligned(src, kind == CRD_VIZ_FLOAT ? 4 : 1) && aligned(dilated, 4),
                "crd_viz_range: bad argument (workspace must be 8-byte aligned, range, a float map and dilated 4-byte aligned)");
  // frame bases keep the alignment of the first when a frame is a multiple of four pixels
  a.vec = (a.per & 3) == 0 && aligned(src, kind == CRD_VIZ_FLOAT ? 16 : 4) && aligned(dilated, 16);
  hipStream_t st = as_stream(stream);
  uint2* partials = reinterpret_cast<uint2*>(workspace);
  const dim3 grid((unsigned)n_tiles), block(TPB);
  if (dilate) hipLaunchKernelGGL(k_viz_partials<2>, grid, block, 0, st, a, partials);
  else if (kind == CRD_VIZ_FLOAT) hipLaunchKernelGGL(k_viz_partials<0>, grid, block, 0, st, a, partials);
  else hipLaunchKernelGGL(k_viz_partials<1>, grid, block, 0, st, a, partials);
  hipLaunchKernelGGL(k_viz_fold, dim3(B), block, 0, st, partials, a.tiles_per_frame, range);
  CRD_LAUNCH_CHECK("crd_viz_range");
  return CRD_OK;
}

extern "C" int crd_viz_draw(const void* src, int32_t kind, int32_t B, int32_t h, int32_t w, const uint8_t* table, const float* range,
                            float vmin, float vmax, int32_t bad_rgb, const uint8_t* image, int32_t image_bgr, int32_t mode, float alpha,
                            float beta, int32_t grey, uint8_t* out, int64_t out_row_pitch, int64_t out_frame_pitch, crd_stream_t stream) {
  const int rc = check_shape("crd_viz_draw", B, h, w);
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(kind == CRD_VIZ_FLOAT || kind == CRD_VIZ_LABELS, "crd_viz_draw: bad argument (kind %d is neither 0, float, nor 1, labels)", kind);
  CRD_CHECK_ARG(mode >= CRD_VIZ_NONE && mode <= CRD_VIZ_IMAGE, "crd_viz_draw: bad argument (mode %d outside 0 .. 3)", mode);
  CRD_CHECK_ARG(out, "crd_viz_draw: null pointer (out)");
  CRD_CHECK_ARG(mode == CRD_VIZ_IMAGE || (src && table), "crd_viz_draw: null pointer (src, table)");
  CRD_CHECK_ARG(mode == CRD_VIZ_NONE || image, "crd_viz_draw: null pointer (image, with mode %d)", mode);
  CRD_CHECK_ARG(out_row_pitch >= 3ll * w, "crd_viz_draw: bad argument (the row pitch %lld is smaller than 3 * w = %lld)",
                (long long)out_row_pitch, 3ll * w);
  CRD_CHECK_ARG(B == 1 || out_frame_pitch >= (h - 1) * out_row_pitch + 3ll * w,
                "crd_viz_draw: bad argument (the frame pitch %lld is smaller than a frame, %lld)", (long long)out_frame_pitch,
                (long long)((h - 1) * out_row_pitch + 3ll * w));
  if (mode != CRD_VIZ_IMAGE && !range) {
    CRD_CHECK_ARG(fabsf(vmin) < INFINITY && fabsf(vmax) < INFINITY && vmin <= vmax, "crd_viz_draw: bad argument (vmin %g, vmax %g)", vmin, vmax);
  }
  if (mode == CRD_VIZ_BLEND) {
    CRD_CHECK_ARG(fabsf(alpha) <= 1e30f && fabsf(beta) <= 1e30f, "crd_viz_draw: bad argument (alpha %g, beta %g)", alpha, beta);
  }
  CRD_CHECK_ARG(bad_rgb >= 0 && bad_rgb <= 0xffffff, "crd_viz_draw: bad argument (bad_rgb 0x%x is not R | G << 8 | B << 16)", bad_rgb);
  CRD_CHECK_ARG(aligned(range, 4) && (mode == CRD_VIZ_IMAGE || kind != CRD_VIZ_FLOAT || aligned(src, 4)),
                "crd_viz_draw: bad argument (range and a float map must be 4-byte aligned)");
  Draw a;
  a.src = src; a.table = table; a.range = range; a.image = image; a.out = out; a.row_pitch = out_row_pitch; a.frame_pitch = out_frame_pitch;
  a.h = h; a.w = w; a.quads_per_row = (w + PER - 1) / PER; a.kind = kind; a.mode = mode; a.bgr = image_bgr != 0; a.grey = grey != 0;
  a.vmin = vmin; a.vmax = vmax; a.alpha = alpha; a.beta = beta; a.bad = (unsigned)bad_rgb;
  const long long n_quads = (long long)B * h * a.quads_per_row;
  const bool vec = (w & 3) == 0 && (mode == CRD_VIZ_IMAGE || aligned(src, kind == CRD_VIZ_FLOAT ? 16 : 4)) && aligned(image, 4) &&
                   aligned(out, 4) && (out_row_pitch & 3) == 0 && (out_frame_pitch & 3) == 0;
  const dim3 grid((unsigned)((n_quads + TPB - 1) / TPB)), block(TPB);
  if (vec) hipLaunchKernelGGL(k_viz_draw<true>, grid, block, 0, as_stream(stream), a, n_quads);
  else hipLaunchKernelGGL(k_viz_draw<false>, grid, block, 0, as_stream(stream), a, n_quads);
  CRD_LAUNCH_CHECK("crd_viz_draw");
  return CRD_OK;
}

extern "C" int crd_seg_labels(const float* logits, int32_t B, int32_t C, int32_t h, int32_t w, uint8_t* labels, crd_stream_t stream) {
  const int rc = check_shape("crd_seg_labels", B, h, w);
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(C >= 1 && C <= 256, "crd_seg_labels: bad argument (C %d outside 1 .. 256)", C);
  CRD_CHECK_ARG(logits && labels, "crd_seg_labels: null pointer (logits, labels)");
  CRD_CHECK_ARG(aligned(logits, 4), "crd_seg_labels: bad argument (logits must be 4-byte aligned)");
  const int per = h * w, quads_per_frame = (per + PER - 1) / PER;
  const long long n_quads = (long long)B * quads_per_frame;
  const int vec = (per & 3) == 0 && aligned(logits, 16) && aligned(labels, 4);
  hipLaunchKernelGGL(k_seg_labels, dim3((unsigned)((n_quads + TPB - 1) / TPB)), dim3(TPB), 0, as_stream(stream), logits, C, per, quads_per_frame,
                     n_quads, vec, labels);
  CRD_LAUNCH_CHECK("crd_seg_labels");
  return CRD_OK;
}
