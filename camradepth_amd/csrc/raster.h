// The z-buffer rasteriser the radar and lidar front ends share (radar_ops.hip, lidar_ops.hip), with the projection arithmetic in front of
// it and the pixel-centre convention that cloud_ops.hip inverts.  It is pinned bit for bit to the reference's NumPy loop
// (cal_depthMap_flow of lib/fuse_radar.py:156-204 and lib/fuse_lidar.py:281-323): per pixel the smallest depth wins, the lowest index among
// equal depths; pixel centres, the clip, round half to even, the cutoff row.  All arithmetic is fp64.  Everything here has internal
// linkage: a translation unit that includes this header gets its own copy of the three pass kernels.
#pragma once
#include "common.h"

// NumPy never fuses a multiply into an add
#pragma clang fp contract(off)

namespace {

constexpr int ZBUF_TPB = 256;
constexpr unsigned NO_POINT = 0xffffffffu;

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < INFINITY; }      // false for NaN as well

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The frame of point p: the b with off[b] <= p < off[b + 1], or -1.  off has B + 1 non-decreasing entries (empty frames repeat a value).
__device__ __forceinline__ int frame_of(const int32_t* off, int B, int p) {
  int lo = 0, hi = B + 1;                      // first j in [0, B + 1] with off[j] > p
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] > p) hi = mid; else lo = mid + 1;
  }
  return (lo == 0 || lo == B + 1) ? -1 : lo - 1;
}

// ---- projection ---------------------------------------------------------------------------------------------------------
// M . (x, y, z, 1) for a row-major 3 x 4 matrix
__device__ __forceinline__ void rigid(const double* M, double x, double y, double z, double& X, double& Y, double& Z) {
  X = M[0] * x + M[1] * y + M[2] * z + M[3];
  Y = M[4] * x + M[5] * y + M[6] * z + M[7];
  Z = M[8] * x + M[9] * y + M[10] * z + M[11];
}

struct Cam { double px, py, Z; };

// view_points(..., normalize=True): K . (X, Y, Z) / Z.  Kb is the frame's row-major 3 x 3 matrix.
__device__ __forceinline__ Cam pinhole(const double* Kb, double X, double Y, double Z) {
  const double fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
  Cam c;
  c.px = (fx * X + cx * Z) / Z;
  c.py = (fy * Y + cy * Z) / Z;
  c.Z = Z;
  return c;
}

// remove_close keeps a sensor-frame point unless |x| < d and |y| < d; a camera sees it at min_z or farther and strictly inside the
// image.  Every comparison is written so that a NaN fails it.
__device__ __forceinline__ bool far_enough(double x, double y, double min_dist) { return fabs(x) >= min_dist || fabs(y) >= min_dist; }
__device__ __forceinline__ bool in_view(const Cam& c, double min_z, double im_w, double im_h) {
  return c.Z >= min_z && c.px > 0.0 && c.px < im_w && c.py > 0.0 && c.py < im_h;
}

// ---- pixel centres ------------------------------------------------------------------------------------------------------
// Full-resolution coordinate v in the image downsampled by s, and the centre of small-image pixel c back at full resolution
__device__ __forceinline__ double to_small(double v, double s) { return (v + 0.5) / s - 0.5; }
__device__ __forceinline__ double to_full(double c, double s) { return (c + 0.5) * s - 0.5; }
// ... clipped into the small image (fuse_radar.py:169-177, fuse_lidar.py:293-301)
__device__ __forceinline__ double scaled(double v, double s, double hi) { return fmin(fmax(to_small(v, s), 0.0), hi); }

// ---- the passes ---------------------------------------------------------------------------------------------------------
// What the passes read.  The workspace holds the winner image (uint32 [n_pix]) and, from the next 16-byte boundary, the key image
// (uint64 [n_pix], the bits of the smallest depth).
struct Zbuf {
  const unsigned char* valid;        // NULL: every point
  const int32_t* off;
  const double* extra;               // NULL, or one more value per point that has to be finite (radar's v_comp)
  const double *x1, *y1, *d1, *x2, *y2;
  const double* K;
  int B, n, k_stride;
  int h_out, w_new, y_cutoff;        // h_out = h_new - y_cutoff rows are kept
  double s, x_hi, y_hi;              // downsample_scale, w_new - 1, h_new - 1
};

// The flat index of point p's pixel in the [B][h_out][w_new] images, or -1: the point is masked out, belongs to no frame, is one the
// reference would raise on (non-finite) or read as an empty pixel (depth <= 0), or falls on a row above the cutoff.  The reference
// rounds half to even (Python's round).
__device__ __forceinline__ long long pixel_of(const Zbuf& r, int p) {
  if (r.valid && !r.valid[p]) return -1;
  const int b = frame_of(r.off, r.B, p);
  if (b < 0) return -1;
  const double x1 = r.x1[p], y1 = r.y1[p], d = r.d1[p];
  if (!(finite_d(x1) && finite_d(y1) && finite_d(r.x2[p]) && finite_d(r.y2[p]) && finite_d(d) && d > 0.0)) return -1;
  if (r.extra && !finite_d(r.extra[p])) return -1;
  const int col = (int)rint(scaled(x1, r.s, r.x_hi));
  const int row = (int)rint(scaled(y1, r.s, r.y_hi)) - r.y_cutoff;
  if (row < 0) return -1;
  return ((long long)b * r.h_out + row) * r.w_new + col;                // row < h_out, col < w_new: the clip
}

// Pass 0: both key images to all ones -- no point (winner), above every depth (key).  n_words 8-byte words from a 16-byte boundary.
__global__ __launch_bounds__(ZBUF_TPB) void k_zbuf_clear(unsigned long long* ws, long long n_words) {
  const long long n_vec = n_words >> 1, t = (long long)blockIdx.x * ZBUF_TPB + threadIdx.x;
  for (long long v = t; v < n_vec; v += (long long)gridDim.x * ZBUF_TPB)
    reinterpret_cast<uint4*>(ws)[v] = make_uint4(NO_POINT, NO_POINT, NO_POINT, NO_POINT);
  if ((n_words & 1) && t == 0) ws[n_words - 1] = ~0ull;
}

// Pass 1: the smallest depth of every pixel.  Positive doubles order as their bit patterns do, so an unsigned 64-bit minimum is exact
// and does not depend on the order of arrival.  A key only ever falls, so a plain read that already shows a depth at or below this
// point's settles it without an atomic: with three lidar points to a pixel and more on near surfaces most points take that way out.
__global__ __launch_bounds__(ZBUF_TPB) void k_zbuf_min_depth(Zbuf r, unsigned long long* key) {
  const int p = blockIdx.x * ZBUF_TPB + threadIdx.x;
  if (p >= r.n) return;
  const long long pix = pixel_of(r, p);
  if (pix < 0) return;
  const unsigned long long mine = (unsigned long long)__double_as_longlong(r.d1[p]);
  if (__hip_atomic_load(key + pix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= mine) return;
  __hip_atomic_fetch_min(key + pix, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 2: among the points that have that depth the lowest index wins -- the reference's loop replaces on a strictly smaller depth
// only, so the first of equal depths stays.
__global__ __launch_bounds__(ZBUF_TPB) void k_zbuf_min_index(Zbuf r, const unsigned long long* key, unsigned* winner) {
  const int p = blockIdx.x * ZBUF_TPB + threadIdx.x;
  if (p >= r.n) return;
  const long long pix = pixel_of(r, p);
  if (pix < 0) return;
  if (key[pix] != (unsigned long long)__double_as_longlong(r.d1[p])) return;
  if (__hip_atomic_load(winner + pix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)p) return;
  __hip_atomic_fetch_min(winner + pix, (unsigned)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- what a resolve pass needs ------------------------------------------------------------------------------------------
struct Pixel { int b, row, col; };

// Frame, row and column of the flat pixel index pix
__device__ __forceinline__ Pixel pixel_at(const Zbuf& r, long long pix) {
  const long long per = (long long)r.h_out * r.w_new;
  Pixel a;
  a.b = (int)(pix / per);
  const int rem = (int)(pix - a.b * per);
  a.row = rem / r.w_new;
  a.col = rem - a.row * r.w_new;
  return a;
}

// The flow of point i in the small image: where camera 2 sees it minus where camera 1 does
__device__ __forceinline__ void flow_of(const Zbuf& r, unsigned i, double& fx, double& fy) {
  const double xa = scaled(r.x1[i], r.s, r.x_hi), ya = scaled(r.y1[i], r.s, r.y_hi);
  const double xb = scaled(r.x2[i], r.s, r.x_hi), yb = scaled(r.y2[i], r.s, r.y_hi);
  fx = xb - xa;
  fy = yb - ya;
}

// radarFlow2uv / lidarFlow2uv: the flow's end point in normalised camera coordinates.  x_map and y_map are float32 there, so the sum is
// rounded once into one; the principal point moves with the downsampling and the cutoff, and fx divides both.
__device__ __forceinline__ void flow_uv(const Zbuf& r, const Pixel& a, double fx, double fy, float& u, float& v) {
  const float xm = (float)((double)a.col + fx);
  const float ym = (float)((double)a.row + fy);
  const double* Kb = r.K + (long long)a.b * r.k_stride;
  const double f = Kb[0] / r.s, cx = Kb[2] / r.s, cy = Kb[5] / r.s - (double)r.y_cutoff;
  u = (float)(((double)xm - cx) / f);
  v = (float)(((double)ym - cy) / f);
}

// Four pixels of a [.][3] fp32 map from pixel p0 (a multiple of four; the map is 16-byte aligned): three 16-byte stores
__device__ __forceinline__ void store_quad3(float* map, long long p0, const float (&o)[12]) {
  float4* dst = reinterpret_cast<float4*>(map + p0 * 3);
  dst[0] = make_float4(o[0], o[1], o[2], o[3]);
  dst[1] = make_float4(o[4], o[5], o[6], o[7]);
  dst[2] = make_float4(o[8], o[9], o[10], o[11]);
}

// Blocks of ZBUF_TPB threads for a grid-stride pass over n_quads groups of four pixels
inline unsigned quad_blocks(long long n_pix) {
  const long long blocks = ((n_pix + 3) / 4 + ZBUF_TPB - 1) / ZBUF_TPB;
  return (unsigned)(blocks < 2048 ? blocks : 2048);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct ZbufImages {
  long long n_pix, key_end;          // pixels of the [B][h_out][w_new] images; bytes of the winner and key images
  unsigned* winner;
  unsigned long long* key;
};

// The checks crd_radar_rasterize and crd_lidar_ground_truth share, under the entry point's name; then r and im filled and passes 0 to 2
// launched on st.  r arrives with the point arrays, valid, off and K set.  need_of(key_end) is the entry point's workspace need in
// bytes, as include/camradepth_hip.h states it.  -> CRD_OK, or the status to return.
template <class NeedOf>
int zbuf_passes(const char* name, Zbuf& r, int32_t B, int32_t n_points, int32_t k_stride, int32_t im_h, int32_t im_w, int32_t downsample_scale,
                int32_t y_cutoff, void* workspace, int64_t workspace_bytes, NeedOf need_of, hipStream_t st, ZbufImages& im) {
  CRD_CHECK_ARG(B > 0 && B <= 65535 && n_points >= 0 && im_h > 0 && im_w > 0 && downsample_scale > 0,
                "%s: bad argument (B %d, n_points %d, image %d x %d, downsample_scale %d)", name, B, n_points, im_h, im_w, downsample_scale);
  const int h_new = im_h / downsample_scale, w_new = im_w / downsample_scale;
  CRD_CHECK_ARG(h_new > 0 && w_new > 0, "%s: bad argument (downsample_scale %d leaves no pixel of %d x %d)", name, downsample_scale, im_h,
                im_w);
  CRD_CHECK_ARG(y_cutoff >= 0 && y_cutoff < h_new, "%s: bad argument (y_cutoff %d outside [0, %d))", name, y_cutoff, h_new);
  CRD_CHECK_ARG(k_stride == 0 || k_stride == 9, "%s: bad argument (k_stride %d is neither 0 nor 9)", name, k_stride);
  CRD_CHECK_ARG(r.K && workspace, "%s: null pointer", name);
  CRD_CHECK_ARG(n_points == 0 || (r.x1 && r.y1 && r.d1 && r.x2 && r.y2 && r.off), "%s: null pointer (points)", name);
  r.B = B; r.n = n_points; r.k_stride = k_stride; r.h_out = h_new - y_cutoff; r.w_new = w_new; r.y_cutoff = y_cutoff;
  r.s = (double)downsample_scale; r.x_hi = (double)(w_new - 1); r.y_hi = (double)(h_new - 1);
  im.n_pix = (long long)B * r.h_out * w_new;
  const long long key_off = (im.n_pix * 4 + 15) & ~15ll;
  im.key_end = key_off + im.n_pix * 8;
  const long long need = need_of(im.key_end);
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  im.winner = reinterpret_cast<unsigned*>(workspace);
  im.key = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + key_off);
  const long long clear_blocks = (im.key_end / 16 + ZBUF_TPB - 1) / ZBUF_TPB;
  hipLaunchKernelGGL(k_zbuf_clear, dim3((unsigned)(clear_blocks < 2048 ? (clear_blocks > 0 ? clear_blocks : 1) : 2048)), dim3(ZBUF_TPB), 0, st,
                     reinterpret_cast<unsigned long long*>(workspace), im.key_end / 8);
  if (n_points > 0) {
    hipLaunchKernelGGL(k_zbuf_min_depth, dim3(cdiv(n_points, ZBUF_TPB)), dim3(ZBUF_TPB), 0, st, r, im.key);
    hipLaunchKernelGGL(k_zbuf_min_index, dim3(cdiv(n_points, ZBUF_TPB)), dim3(ZBUF_TPB), 0, st, r, im.key, im.winner);
  }
  return CRD_OK;
}

}  // namespace
