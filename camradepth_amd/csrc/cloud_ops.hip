// Point-cloud back end on the device: a depth map [B][h][w] (the network's normalised inverse depth, or metres) -> 3-D points in the
// caller's frame.  The inverse of the rasterisers of radar_ops.hip / lidar_ops.hip: the pixel-centre convention, K / k_stride, the row
// cutoff and the frame_offsets layout are theirs.  crd_depth_unproject writes the organised cloud in one launch; crd_point_cloud writes
// the valid candidates densely in (b, r, c) order with three launches (count per tile, scan of the tile counts, scatter), no workgroup
// waiting on another and no atomic.  All arithmetic is fp64; each coordinate is rounded to fp32 once.
#include "raster.h"       // the pixel-centre convention (to_full inverts the rasterisers' to_small) and the quad store of a [.][3] map
#include <string.h>

// the results are specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int PER = 4;                         // consecutive candidates per thread
constexpr int TILE = TPB * PER;                // candidates per workgroup of the compact path: CRD_CLOUD_TILE
constexpr int WAVES = TPB / CRD_WAVE;
constexpr int SCAN_TPB = 1024;
static_assert(TILE == CRD_CLOUD_TILE, "include/camradepth_hip.h states the tile size");

struct Cloud {
  const float* depth;
  const unsigned char *mask, *labels, *keep;   // each may be NULL (keep goes with labels)
  const double *K, *T;                         // T may be NULL
  int B, h, w, k_stride, t_stride, y_cutoff, encoding, skip_empty;
  double s, max_depth, min_range, max_range;
};

// Steps 1 and the tests on p and d: the depth in metres of a pixel that reads pf, and whether the pixel passes.  A NaN fails.
__device__ __forceinline__ bool metres(const Cloud& a, float pf, double& d) {
  const double p = (double)pf;
  d = a.encoding == 0 ? a.max_depth * (1.0 - p) : p;
  const bool ok = fabs(p) < INFINITY && d > 0.0 && d >= a.min_range && d <= a.max_range;
  return ok && (a.encoding == 0 ? !(a.skip_empty && p == 0.0) : p > 0.0);
}

// Steps 2 to 5 for pixel (r, c) at depth d: Kb the frame's intrinsics, Tb its out_from_cam or NULL.
__device__ __forceinline__ void point_of(const Cloud& a, const double* Kb, const double* Tb, int r, int c, double d, float& x, float& y,
                                         float& z) {
  const double xf = to_full((double)c, a.s);
  const double yf = to_full((double)(r + a.y_cutoff), a.s);
  const double X = ((xf - Kb[2]) / Kb[0]) * d, Y = ((yf - Kb[5]) / Kb[4]) * d, Z = d;
  if (Tb) {
    x = (float)(((Tb[0] * X + Tb[1] * Y) + Tb[2] * Z) + Tb[3]);
    y = (float)(((Tb[4] * X + Tb[5] * Y) + Tb[6] * Z) + Tb[7]);
    z = (float)(((Tb[8] * X + Tb[9] * Y) + Tb[10] * Z) + Tb[11]);
  } else {
    x = (float)X; y = (float)Y; z = (float)Z;
  }
}

// ---- organised cloud ----------------------------------------------------------------------------------------------------
// Every pixel of points [.][3] and valid, four pixels per thread: one 16-byte load of depth, three 16-byte stores of points.  A quad may
// straddle two frames.
__global__ __launch_bounds__(TPB) void k_cloud_unproject(Cloud a, long long n_pix, float* points, unsigned char* valid) {
  const int per = a.h * a.w;
  const long long n_quads = (n_pix + 3) >> 2;
  for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (long long)gridDim.x * TPB) {
    const long long p0 = q * 4;
    const bool whole = p0 + 4 <= n_pix;
    const int n = whole ? 4 : (int)(n_pix - p0);
    float pv[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned m = 0x01010101u, lb = 0;
    if (whole) {
      const float4 v = *reinterpret_cast<const float4*>(a.depth + p0);
      pv[0] = v.x; pv[1] = v.y; pv[2] = v.z; pv[3] = v.w;
      if (a.mask) m = *reinterpret_cast<const unsigned*>(a.mask + p0);
      if (a.labels) lb = *reinterpret_cast<const unsigned*>(a.labels + p0);
    } else {
      for (int k = 0; k < n; ++k) {
        pv[k] = a.depth[p0 + k];
        if (a.mask) m = (m & ~(0xffu << (8 * k))) | ((unsigned)a.mask[p0 + k] << (8 * k));
        if (a.labels) lb |= (unsigned)a.labels[p0 + k] << (8 * k);
      }
    }
    int b = (int)(p0 / per), rem = (int)(p0 - (long long)b * per);
    float o[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unsigned ok4 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        if (rem >= per) { rem -= per; ++b; }
        double d;
        bool ok = metres(a, pv[k], d) && ((m >> (8 * k)) & 0xffu) != 0;
        if (ok && a.labels) ok = a.keep[(lb >> (8 * k)) & 0xffu] != 0;
        if (ok) {
          const int r = rem / a.w, c = rem - r * a.w;
          point_of(a, a.K + (long long)b * a.k_stride, a.T ? a.T + (long long)b * a.t_stride : nullptr, r, c, d, o[3 * k], o[3 * k + 1],
                   o[3 * k + 2]);
          ok4 |= 1u << (8 * k);
        }
        ++rem;
      }
    }
    if (whole) {
      store_quad3(points, p0, o);
      *reinterpret_cast<unsigned*>(valid + p0) = ok4;
    } else {
      for (int k = 0; k < n; ++k) {
        points[(p0 + k) * 3] = o[3 * k]; points[(p0 + k) * 3 + 1] = o[3 * k + 1]; points[(p0 + k) * 3 + 2] = o[3 * k + 2];
        valid[p0 + k] = (unsigned char)((ok4 >> (8 * k)) & 1u);
      }
    }
  }
}

// ---- compact cloud ------------------------------------------------------------------------------------------------------
// The candidates of a frame are the pixels (i * stride, j * stride), numbered i * cw + j: n_cand = ch * cw of them, in tiles of TILE.
// Tile t of the launch is tile t % tiles_per_frame of frame t / tiles_per_frame: no tile straddles two frames.
struct Tiles { int stride, cw, n_cand, tiles_per_frame; };

// The PER consecutive candidates j0 .. j0 + PER - 1 of frame b: bit k of the result says that candidate j0 + k exists and passes every
// test; d[k] is its depth in metres and pix[k] = r * w + c.  VEC: stride 1 and a frame of a multiple of four pixels (the host decides),
// so a candidate is its pixel, the four lie in one aligned 16-byte word of depth and exist together.
template <bool VEC>
__device__ __forceinline__ unsigned candidates(const Cloud& a, const Tiles& t, int b, int j0, double (&d)[PER], int (&pix)[PER]) {
  const long long base = (long long)b * a.h * a.w;
  float pv[PER] = {0.f, 0.f, 0.f, 0.f};
  unsigned m = 0x01010101u, lb = 0, have = 0;
  if (VEC) {
    if (j0 < t.n_cand) {
      const float4 v = *reinterpret_cast<const float4*>(a.depth + base + j0);
      pv[0] = v.x; pv[1] = v.y; pv[2] = v.z; pv[3] = v.w;
      if (a.mask) m = *reinterpret_cast<const unsigned*>(a.mask + base + j0);
      if (a.labels) lb = *reinterpret_cast<const unsigned*>(a.labels + base + j0);
      have = 0xfu;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) pix[k] = j0 + k;
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int j = j0 + k;
      pix[k] = 0;
      if (j < t.n_cand) {
        const int i = j / t.cw;
        pix[k] = i * t.stride * a.w + (j - i * t.cw) * t.stride;
        pv[k] = a.depth[base + pix[k]];
        if (a.mask) m = (m & ~(0xffu << (8 * k))) | ((unsigned)a.mask[base + pix[k]] << (8 * k));
        if (a.labels) lb |= (unsigned)a.labels[base + pix[k]] << (8 * k);
        have |= 1u << k;
      }
    }
  }
  unsigned flags = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    bool ok = ((have >> k) & 1u) != 0 && metres(a, pv[k], d[k]) && ((m >> (8 * k)) & 0xffu) != 0;
    if (ok && a.labels) ok = a.keep[(lb >> (8 * k)) & 0xffu] != 0;
    flags |= ok ? 1u << k : 0u;
  }
  return flags;
}

__device__ __forceinline__ int lanes_below(unsigned long long ballot) {       // the set bits of the lanes under this one
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// Launch 1: counts[tile] = the valid candidates of the tile.  One ballot per candidate slot, the waves' sums through LDS.
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_cloud_count(Cloud a, Tiles t, int32_t* counts) {
  __shared__ int wave_n[WAVES];
  const int tile = blockIdx.x, b = tile / t.tiles_per_frame;
  const int j0 = (tile - b * t.tiles_per_frame) * TILE + threadIdx.x * PER;
  double d[PER];
  int pix[PER];
  const unsigned flags = candidates<VEC>(a, t, b, j0, d, pix);
  int n = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) n += __popcll(__ballot((flags >> k) & 1u));
  if ((threadIdx.x & (CRD_WAVE - 1)) == 0) wave_n[threadIdx.x / CRD_WAVE] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) sum += wave_n[wv];
    counts[tile] = sum;
  }
}

// Launch 2, ONE workgroup: the counts become their exclusive prefix sums in place, SCAN_TPB tiles per pass with the carry in a
// register that every thread holds alike; frame_offsets[b] is the prefix at frame b's first tile, frame_offsets[B] the total.
__global__ __launch_bounds__(SCAN_TPB) void k_cloud_scan(int32_t* counts, int n_tiles, int tiles_per_frame, int B, int32_t* frame_offsets) {
  __shared__ int wave_sum[SCAN_TPB / CRD_WAVE];
  const int lane = threadIdx.x & (CRD_WAVE - 1), wave = threadIdx.x / CRD_WAVE;
  int carry = 0;
  for (int i0 = 0; i0 < n_tiles; i0 += SCAN_TPB) {
    const int i = i0 + threadIdx.x;
    const int v = i < n_tiles ? counts[i] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < CRD_WAVE; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == CRD_WAVE - 1) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int wv = 0; wv < SCAN_TPB / CRD_WAVE; ++wv) {
      const int ws = wave_sum[wv];
      before += wv < wave ? ws : 0;
      all += ws;
    }
    if (i < n_tiles) {
      const int excl = carry + before + incl - v;
      counts[i] = excl;
      const int b = i / tiles_per_frame;
      if (i == b * tiles_per_frame) frame_offsets[b] = excl;
    }
    carry += all;
    __syncthreads();                           // wave_sum is written again in the next pass
  }
  if (threadIdx.x == 0) frame_offsets[B] = carry;
}

// Launch 3: a valid candidate lands at offsets[tile] + the valid ones of the waves before its wave + those of the lanes below its lane
// + those of its own lane before it: the (b, r, c) order, decided by ballots alone.  cap guards the stores should another stream
// have changed depth since the count (the caller's error; it must not become a write past the buffers).
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_cloud_scatter(Cloud a, Tiles t, const int32_t* offsets, const unsigned char* image, int cap,
                                                       float* xyz, unsigned char* rgb, unsigned char* label, int32_t* pixel) {
  __shared__ int wave_n[WAVES];
  const int tile = blockIdx.x, b = tile / t.tiles_per_frame;
  const int j0 = (tile - b * t.tiles_per_frame) * TILE + threadIdx.x * PER;
  double d[PER];
  int pix[PER];
  const unsigned flags = candidates<VEC>(a, t, b, j0, d, pix);
  int n = 0, below = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned long long ballot = __ballot((flags >> k) & 1u);
    n += __popcll(ballot);
    below += lanes_below(ballot);
  }
  const int wave = threadIdx.x / CRD_WAVE;
  if ((threadIdx.x & (CRD_WAVE - 1)) == 0) wave_n[wave] = n;
  __syncthreads();
  if (flags == 0) return;
  int rank = offsets[tile] + below;
#pragma unroll
  for (int wv = 0; wv < WAVES; ++wv) rank += wv < wave ? wave_n[wv] : 0;
  const double* Kb = a.K + (long long)b * a.k_stride;
  const double* Tb = a.T ? a.T + (long long)b * a.t_stride : nullptr;
  const long long base = (long long)b * a.h * a.w;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (((flags >> k) & 1u) && rank >= 0 && rank < cap) {
      const int r = pix[k] / a.w, c = pix[k] - r * a.w;
      float x, y, z;
      point_of(a, Kb, Tb, r, c, d[k], x, y, z);
      float* o = xyz + (long long)rank * 3;
      o[0] = x; o[1] = y; o[2] = z;
      if (rgb) {
        const unsigned char* src = image + (base + pix[k]) * 3;
        unsigned char* dst = rgb + (long long)rank * 3;
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
      }
      if (label) label[rank] = a.labels[base + pix[k]];
      if (pixel) pixel[rank] = pix[k];
    }
    rank += (flags >> k) & 1u;
  }
}

inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }

// The arguments the two entries share, checked before any GPU call.  -> CRD_OK and `a` filled, or the status to return.
int check_common(const char* name, const float* depth, int32_t B, int32_t im_h, int32_t im_w, int32_t s, int32_t y_cutoff, const double* K,
                 int32_t k_stride, const double* T, int32_t t_stride, int32_t encoding, uint64_t max_depth_bits, uint64_t min_range_bits,
                 uint64_t max_range_bits, int32_t skip_empty, const uint8_t* mask, const uint8_t* labels, const uint8_t* keep, Cloud& a) {
  CRD_CHECK_ARG(B > 0 && B <= 65535 && im_h > 0 && im_w > 0 && s > 0, "%s: bad argument (B %d, image %d x %d, downsample_scale %d)", name, B,
                im_h, im_w, s);
  const int h_new = im_h / s, w_new = im_w / s;
  CRD_CHECK_ARG(h_new > 0 && w_new > 0, "%s: bad argument (downsample_scale %d leaves no pixel of %d x %d)", name, s, im_h, im_w);
  CRD_CHECK_ARG(y_cutoff >= 0 && y_cutoff < h_new, "%s: bad argument (y_cutoff %d outside [0, %d))", name, y_cutoff, h_new);
  CRD_CHECK_ARG(k_stride == 0 || k_stride == 9, "%s: bad argument (k_stride %d is neither 0 nor 9)", name, k_stride);
  CRD_CHECK_ARG(t_stride == 0 || t_stride == 12, "%s: bad argument (t_stride %d is neither 0 nor 12)", name, t_stride);
  CRD_CHECK_ARG(encoding == 0 || encoding == 1, "%s: bad argument (encoding %d is neither 0, inverse, nor 1, metres)", name, encoding);
  const double max_depth = from_bits(max_depth_bits), min_range = from_bits(min_range_bits), max_range = from_bits(max_range_bits);
  CRD_CHECK_ARG(max_depth > 0.0 && max_depth < INFINITY, "%s: bad argument (max_depth %g)", name, max_depth);
  CRD_CHECK_ARG(min_range == min_range && max_range == max_range, "%s: bad argument (min_range %g, max_range %g)", name, min_range,
                max_range);
  CRD_CHECK_ARG(depth && K, "%s: null pointer (depth, K)", name);
  CRD_CHECK_ARG(!labels || keep, "%s: bad argument (labels without keep)", name);
  const long long per = (long long)(h_new - y_cutoff) * w_new;
  CRD_CHECK_ARG(per * 3 <= 0x7fffffffll, "%s: bad argument (%lld pixels per frame are more than the 32-bit indices hold)", name, per);
  CRD_CHECK_ARG(aligned(depth, 16) && aligned(mask, 4) && aligned(labels, 4),
                "%s: bad argument (depth must be 16-byte aligned, mask and labels 4-byte aligned)", name);
  a.depth = depth; a.mask = mask; a.labels = labels; a.keep = keep; a.K = K; a.T = T; a.B = B; a.h = h_new - y_cutoff; a.w = w_new;
  a.k_stride = k_stride; a.t_stride = t_stride; a.y_cutoff = y_cutoff; a.encoding = encoding; a.skip_empty = skip_empty != 0;
  a.s = (double)s; a.max_depth = max_depth; a.min_range = min_range; a.max_range = max_range;
  return CRD_OK;
}

}  // namespace

extern "C" int crd_depth_unproject(const float* depth, int32_t B, int32_t im_h, int32_t im_w, int32_t downsample_scale, int32_t y_cutoff,
                                   const double* K, int32_t k_stride, const double* out_from_cam, int32_t t_stride, int32_t encoding,
                                   uint64_t max_depth_f64_bits, uint64_t min_range_f64_bits, uint64_t max_range_f64_bits,
                                   int32_t skip_empty, const uint8_t* mask, const uint8_t* labels, const uint8_t* keep, float* points,
                                   uint8_t* valid, crd_stream_t stream) {
  Cloud a;
  const int rc = check_common("crd_depth_unproject", depth, B, im_h, im_w, downsample_scale, y_cutoff, K, k_stride, out_from_cam, t_stride,
                              encoding, max_depth_f64_bits, min_range_f64_bits, max_range_f64_bits, skip_empty, mask, labels, keep, a);
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(points && valid, "crd_depth_unproject: null pointer (points, valid)");
  CRD_CHECK_ARG(aligned(points, 16) && aligned(valid, 4),
                "crd_depth_unproject: bad argument (points must be 16-byte aligned, valid 4-byte aligned)");
  const long long n_pix = (long long)B * a.h * a.w;
  static_assert(TPB == ZBUF_TPB, "quad_blocks counts blocks of ZBUF_TPB threads");
  hipLaunchKernelGGL(k_cloud_unproject, dim3(quad_blocks(n_pix)), dim3(TPB), 0, as_stream(stream), a, n_pix, points, valid);
  CRD_LAUNCH_CHECK("crd_depth_unproject");
  return CRD_OK;
}

extern "C" int crd_point_cloud(const float* depth, int32_t B, int32_t im_h, int32_t im_w, int32_t downsample_scale, int32_t y_cutoff,
                               const double* K, int32_t k_stride, const double* out_from_cam, int32_t t_stride, int32_t encoding,
                               uint64_t max_depth_f64_bits, uint64_t min_range_f64_bits, uint64_t max_range_f64_bits, int32_t skip_empty,
                               const uint8_t* mask, const uint8_t* labels, const uint8_t* keep, int32_t stride, const uint8_t* image,
                               void* workspace, int64_t workspace_bytes, float* xyz, uint8_t* rgb, uint8_t* label, int32_t* pixel,
                               int32_t* frame_offsets, crd_stream_t stream) {
  Cloud a;
  const int rc = check_common("crd_point_cloud", depth, B, im_h, im_w, downsample_scale, y_cutoff, K, k_stride, out_from_cam, t_stride,
                              encoding, max_depth_f64_bits, min_range_f64_bits, max_range_f64_bits, skip_empty, mask, labels, keep, a);
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(stride > 0, "crd_point_cloud: bad argument (stride %d)", stride);
  CRD_CHECK_ARG(xyz && frame_offsets && workspace, "crd_point_cloud: null pointer (xyz, frame_offsets, workspace)");
  CRD_CHECK_ARG(!rgb || image, "crd_point_cloud: bad argument (rgb without image)");
  CRD_CHECK_ARG(!label || labels, "crd_point_cloud: bad argument (label without labels)");
  Tiles t;
  t.stride = stride;
  t.cw = (a.w + stride - 1) / stride;
  t.n_cand = ((a.h + stride - 1) / stride) * t.cw;
  t.tiles_per_frame = (t.n_cand + TILE - 1) / TILE;
  const long long n_tiles = (long long)B * t.tiles_per_frame, cap = (long long)B * t.n_cand;
  CRD_CHECK_ARG(cap <= 0x7fffffffll, "crd_point_cloud: bad argument (%lld candidates are more than an int32 frame_offsets holds)", cap);
  CRD_CHECK_ARG(workspace_bytes >= 4 * n_tiles, "crd_point_cloud: the workspace holds %lld bytes, %lld are needed",
                (long long)workspace_bytes, 4 * n_tiles);
  CRD_CHECK_ARG(aligned(workspace, 4), "crd_point_cloud: bad argument (workspace must be 4-byte aligned)");
  hipStream_t st = as_stream(stream);
  int32_t* tiles = reinterpret_cast<int32_t*>(workspace);
  const bool vec = stride == 1 && (t.n_cand & 3) == 0;          // frame bases then keep depth's 16-byte and the bytes' 4-byte alignment
  const dim3 grid((unsigned)n_tiles), block(TPB);
  if (vec) hipLaunchKernelGGL(k_cloud_count<true>, grid, block, 0, st, a, t, tiles);
  else hipLaunchKernelGGL(k_cloud_count<false>, grid, block, 0, st, a, t, tiles);
  hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(SCAN_TPB), 0, st, tiles, (int)n_tiles, t.tiles_per_frame, B, frame_offsets);
  if (vec) hipLaunchKernelGGL(k_cloud_scatter<true>, grid, block, 0, st, a, t, tiles, image, (int)cap, xyz, rgb, label, pixel);
  else hipLaunchKernelGGL(k_cloud_scatter<false>, grid, block, 0, st, a, t, tiles, image, (int)cap, xyz, rgb, label, pixel);
  CRD_LAUNCH_CHECK("crd_point_cloud");
  return CRD_OK;
}
