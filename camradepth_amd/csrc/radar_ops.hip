// Radar front end on the device: accumulated radar sweeps -> the radar [B][H][W][3] and rad_vel [B][H][W] maps crd_assemble_input
// reads.  Two stages of the reference's offline preprocessing (lib/fuse_radar.py): the projection nested in merge_selected_radar
// (:30-74, :144-151) and the rasteriser cal_depthMap_flow (:156-204) + radarFlow2uv (:276-303).  All arithmetic is fp64, as NumPy's.
// The input is a few thousand detections; the only pass that touches every pixel is the resolve at the end.
#include "common.h"

// the rasteriser is pinned bit for bit to NumPy, which never fuses a multiply into an add
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr unsigned NO_POINT = 0xffffffffu;

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < INFINITY; }      // false for NaN as well

// The frame of point p: the b with off[b] <= p < off[b + 1], or -1.  off has B + 1 non-decreasing entries (empty frames repeat a value).
__device__ __forceinline__ int frame_of(const int32_t* off, int B, int p) {
  int lo = 0, hi = B + 1;                      // first j in [0, B + 1] with off[j] > p
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] > p) hi = mid; else lo = mid + 1;
  }
  return (lo == 0 || lo == B + 1) ? -1 : lo - 1;
}

struct Cam { double px, py, Z; };

// fuse_radar.py:49-52 (Doppler compensation, then the pose chain) and view_points(..., normalize=True) of :69: K . (X, Y, Z) / Z
__device__ __forceinline__ Cam project_one(const double* M, double lag, double x, double y, double z, double vx, double vy,
                                           double fx, double fy, double cx, double cy) {
  const double xs = x + vx * lag, ys = y + vy * lag;
  const double X = M[0] * xs + M[1] * ys + M[2] * z + M[3];
  const double Y = M[4] * xs + M[5] * ys + M[6] * z + M[7];
  const double Z = M[8] * xs + M[9] * ys + M[10] * z + M[11];
  Cam c;
  c.px = (fx * X + cx * Z) / Z;
  c.py = (fy * Y + cy * Z) / Z;
  c.Z = Z;
  return c;
}

// One thread per point.  Every comparison is written so that a NaN fails it (:68, :73); a NaN coordinate that passes remove_close (:32)
// reaches px and py and fails there.
__global__ __launch_bounds__(TPB) void k_radar_project(const double* pts, const int32_t* sweep, const int32_t* off, int B, int n,
                                                       const double* M1, const double* M2, const double* lags, int n_sweeps,
                                                       const double* K, int k_stride, double im_h, double im_w, double min_dist,
                                                       double min_z, double* x1, double* y1, double* d1, double* x2, double* y2,
                                                       double* vc, unsigned char* valid) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= n) return;
  const int b = frame_of(off, B, p);
  const int s = sweep[p];
  double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = false;
  if (b >= 0 && s >= 0 && s < n_sweeps) {
    const double* q = pts + (long long)p * 5;
    const double x = q[0], y = q[1], z = q[2], vx = q[3], vy = q[4];
    const double* Kb = K + (long long)b * k_stride;
    const double fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
    const Cam a = project_one(M1 + (long long)s * 12, lags[2 * s], x, y, z, vx, vy, fx, fy, cx, cy);
    const Cam c = project_one(M2 + (long long)s * 12, lags[2 * s + 1], x, y, z, vx, vy, fx, fy, cx, cy);
    o[0] = a.px; o[1] = a.py; o[2] = a.Z; o[3] = c.px; o[4] = c.py;
    o[5] = sqrt(vx * vx + vy * vy);
    const bool far = fabs(x) >= min_dist || fabs(y) >= min_dist;          // not (|x| < d and |y| < d)
    ok = far && a.Z >= min_z && c.Z >= min_z && a.px > 0.0 && a.px < im_w && a.py > 0.0 && a.py < im_h &&
         c.px > 0.0 && c.px < im_w && c.py > 0.0 && c.py < im_h;
  }
  x1[p] = o[0]; y1[p] = o[1]; d1[p] = o[2]; x2[p] = o[3]; y2[p] = o[4]; vc[p] = o[5];
  valid[p] = ok ? 1 : 0;
}

// ---- rasteriser ---------------------------------------------------------------------------------------------------------
struct Raster {
  const double *x1, *y1, *d1, *x2, *y2, *vc;
  const unsigned char* valid;        // NULL: every point
  const int32_t* off;
  const double* K;
  int B, n, k_stride;
  int h_out, w_new, y_cutoff;        // h_out = h_new - y_cutoff rows are kept
  double s, x_hi, y_hi;              // downsample_scale, w_new - 1, h_new - 1
};

// fuse_radar.py:169-177: pixel centres of the small image, clipped into it
__device__ __forceinline__ double scaled(double v, double s, double hi) { return fmin(fmax((v + 0.5) / s - 0.5, 0.0), hi); }

// The flat index of point p's pixel in the [B][h_out][w_new] images, or -1: the point is masked out, belongs to no frame, is one the
// reference would raise on (non-finite, depth <= 0), or falls on a row above the cutoff.  :183 rounds half to even (Python's round).
__device__ __forceinline__ long long pixel_of(const Raster& r, int p) {
  if (r.valid && !r.valid[p]) return -1;
  const int b = frame_of(r.off, r.B, p);
  if (b < 0) return -1;
  const double x1 = r.x1[p], y1 = r.y1[p], d = r.d1[p];
  if (!(finite_d(x1) && finite_d(y1) && finite_d(r.x2[p]) && finite_d(r.y2[p]) && finite_d(r.vc[p]) && finite_d(d) && d > 0.0)) return -1;
  const int col = (int)rint(scaled(x1, r.s, r.x_hi));
  const int row = (int)rint(scaled(y1, r.s, r.y_hi)) - r.y_cutoff;
  if (row < 0) return -1;
  return ((long long)b * r.h_out + row) * r.w_new + col;                // row < h_out, col < w_new: the clip
}

// Pass 0: both key images to all ones -- no point (winner), above every depth (key).  n_words 8-byte words from a 16-byte boundary.
__global__ __launch_bounds__(TPB) void k_radar_clear(unsigned long long* ws, long long n_words) {
  const long long n_vec = n_words >> 1, t = (long long)blockIdx.x * TPB + threadIdx.x;
  for (long long v = t; v < n_vec; v += (long long)gridDim.x * TPB)
    reinterpret_cast<uint4*>(ws)[v] = make_uint4(NO_POINT, NO_POINT, NO_POINT, NO_POINT);
  if ((n_words & 1) && t == 0) ws[n_words - 1] = ~0ull;
}

// Pass 1: the smallest depth of every pixel.  Positive doubles order as their bit patterns do, so an unsigned 64-bit minimum is exact
// and does not depend on the order of arrival.
__global__ __launch_bounds__(TPB) void k_radar_min_depth(Raster r, unsigned long long* key) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= r.n) return;
  const long long pix = pixel_of(r, p);
  if (pix < 0) return;
  __hip_atomic_fetch_min(key + pix, (unsigned long long)__double_as_longlong(r.d1[p]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 2: among the points that have that depth the lowest index wins -- the reference's loop (:185-197) replaces on a strictly
// smaller depth only, so the first of equal depths stays.
__global__ __launch_bounds__(TPB) void k_radar_min_index(Raster r, const unsigned long long* key, unsigned* winner) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= r.n) return;
  const long long pix = pixel_of(r, p);
  if (pix < 0) return;
  if (key[pix] == (unsigned long long)__double_as_longlong(r.d1[p]))
    __hip_atomic_fetch_min(winner + pix, (unsigned)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The four values of a won pixel (:187, :202, :284-295).  pix is its flat index.
__device__ __forceinline__ void resolve_one(const Raster& r, long long pix, unsigned i, float& depth, float& u, float& v, float& vel) {
  const long long per = (long long)r.h_out * r.w_new;
  const int b = (int)(pix / per);
  const int rem = (int)(pix - b * per);
  const int row = rem / r.w_new, col = rem - row * r.w_new;
  const double xa = scaled(r.x1[i], r.s, r.x_hi), ya = scaled(r.y1[i], r.s, r.y_hi);
  const double xb = scaled(r.x2[i], r.s, r.x_hi), yb = scaled(r.y2[i], r.s, r.y_hi);
  const float xm = (float)((double)col + (xb - xa));                     // x_map is float32 (:286); the sum is rounded once into it
  const float ym = (float)((double)row + (yb - ya));
  const double* Kb = r.K + (long long)b * r.k_stride;
  const double f = Kb[0] / r.s, cx = Kb[2] / r.s, cy = Kb[5] / r.s - (double)r.y_cutoff;      // :290-292; f is fx for both (:294-295)
  depth = (float)r.d1[i];
  u = (float)(((double)xm - cx) / f);
  v = (float)(((double)ym - cy) / f);
  vel = r.vc[i] > 0.5 ? 1.f : 0.f;
}

// Pass 3: every pixel of radar [.][3] and rad_vel, four pixels (64 bytes out, 16 in) per thread; a quad nobody won is four vector stores
// of zeros, and almost every quad is one.  A winner is an index below n (NO_POINT is not): nothing read from the image is trusted.
__global__ __launch_bounds__(TPB) void k_radar_resolve(Raster r, const unsigned* winner, long long n_pix, float* radar, float* rad_vel) {
  const long long n_quads = (n_pix + 3) >> 2;
  for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (long long)gridDim.x * TPB) {
    const long long p0 = q * 4;
    float o[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vel[4] = {0.f, 0.f, 0.f, 0.f};
    if (p0 + 4 <= n_pix) {
      const uint4 w = *reinterpret_cast<const uint4*>(winner + p0);
      const unsigned wi[4] = {w.x, w.y, w.z, w.w};
      if ((w.x & w.y & w.z & w.w) != NO_POINT) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (wi[k] < (unsigned)r.n) resolve_one(r, p0 + k, wi[k], o[3 * k], o[3 * k + 1], o[3 * k + 2], vel[k]);
      }
      float4* dst = reinterpret_cast<float4*>(radar + p0 * 3);
      dst[0] = make_float4(o[0], o[1], o[2], o[3]);
      dst[1] = make_float4(o[4], o[5], o[6], o[7]);
      dst[2] = make_float4(o[8], o[9], o[10], o[11]);
      *reinterpret_cast<float4*>(rad_vel + p0) = make_float4(vel[0], vel[1], vel[2], vel[3]);
    } else {                                                              // the last, short quad
      for (long long p = p0; p < n_pix; ++p) {
        float d = 0.f, u = 0.f, v = 0.f, m = 0.f;
        const unsigned i = winner[p];
        if (i < (unsigned)r.n) resolve_one(r, p, i, d, u, v, m);
        radar[p * 3] = d; radar[p * 3 + 1] = u; radar[p * 3 + 2] = v;
        rad_vel[p] = m;
      }
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int crd_radar_project(const double* points, const int32_t* sweep_index, const int32_t* frame_offsets, int32_t B,
                                 int32_t n_points, const double* cam1_from_sensor, const double* cam2_from_sensor, const double* lags,
                                 int32_t n_sweeps, const double* K, int32_t k_stride, int32_t im_h, int32_t im_w, float min_distance,
                                 float min_z, double* x1, double* y1, double* depth1, double* x2, double* y2, double* v_comp,
                                 uint8_t* valid, crd_stream_t stream) {
  CRD_CHECK_ARG(B > 0 && B <= 65535 && n_points >= 0 && n_sweeps >= 0 && im_h > 0 && im_w > 0,
                "crd_radar_project: bad argument (B %d, n_points %d, n_sweeps %d, image %d x %d)", B, n_points, n_sweeps, im_h, im_w);
  CRD_CHECK_ARG(k_stride == 0 || k_stride == 9, "crd_radar_project: bad argument (k_stride %d is neither 0 nor 9)", k_stride);
  CRD_CHECK_ARG(min_distance >= 0.f && min_z == min_z, "crd_radar_project: bad argument (min_distance %g, min_z %g)",
                (double)min_distance, (double)min_z);
  if (n_points == 0) return CRD_OK;
  CRD_CHECK_ARG(points && sweep_index && frame_offsets && K && x1 && y1 && depth1 && x2 && y2 && v_comp && valid,
                "crd_radar_project: null pointer");
  CRD_CHECK_ARG(n_sweeps == 0 || (cam1_from_sensor && cam2_from_sensor && lags), "crd_radar_project: null pointer (sweep tables)");
  hipLaunchKernelGGL(k_radar_project, dim3(cdiv(n_points, TPB)), dim3(TPB), 0, as_stream(stream), points, sweep_index, frame_offsets,
                     B, n_points, cam1_from_sensor, cam2_from_sensor, lags, n_sweeps, K, k_stride, (double)im_h, (double)im_w,
                     (double)min_distance, (double)min_z, x1, y1, depth1, x2, y2, v_comp, valid);
  CRD_LAUNCH_CHECK("crd_radar_project");
  return CRD_OK;
}

extern "C" int crd_radar_rasterize(const double* x1, const double* y1, const double* depth1, const double* x2, const double* y2,
                                   const double* v_comp, const uint8_t* valid, const int32_t* frame_offsets, int32_t B, int32_t n_points,
                                   const double* K, int32_t k_stride, int32_t im_h, int32_t im_w, int32_t downsample_scale,
                                   int32_t y_cutoff, void* workspace, int64_t workspace_bytes, float* radar, float* rad_vel,
                                   crd_stream_t stream) {
  CRD_CHECK_ARG(B > 0 && B <= 65535 && n_points >= 0 && im_h > 0 && im_w > 0 && downsample_scale > 0,
                "crd_radar_rasterize: bad argument (B %d, n_points %d, image %d x %d, downsample_scale %d)", B, n_points, im_h, im_w,
                downsample_scale);
  const int h_new = im_h / downsample_scale, w_new = im_w / downsample_scale;
  CRD_CHECK_ARG(h_new > 0 && w_new > 0, "crd_radar_rasterize: bad argument (downsample_scale %d leaves no pixel of %d x %d)",
                downsample_scale, im_h, im_w);
  CRD_CHECK_ARG(y_cutoff >= 0 && y_cutoff < h_new, "crd_radar_rasterize: bad argument (y_cutoff %d outside [0, %d))", y_cutoff, h_new);
  CRD_CHECK_ARG(k_stride == 0 || k_stride == 9, "crd_radar_rasterize: bad argument (k_stride %d is neither 0 nor 9)", k_stride);
  CRD_CHECK_ARG(K && workspace && radar && rad_vel, "crd_radar_rasterize: null pointer");
  CRD_CHECK_ARG(n_points == 0 || (x1 && y1 && depth1 && x2 && y2 && v_comp && frame_offsets), "crd_radar_rasterize: null pointer (points)");
  const int h_out = h_new - y_cutoff;
  const long long n_pix = (long long)B * h_out * w_new;
  const long long key_off = (n_pix * 4 + 15) & ~15ll, need = key_off + n_pix * 8;
  CRD_CHECK_ARG(workspace_bytes >= need, "crd_radar_rasterize: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                need);
  CRD_CHECK_ARG(aligned16(workspace) && aligned16(radar) && aligned16(rad_vel),
                "crd_radar_rasterize: bad argument (workspace, radar and rad_vel must be 16-byte aligned)");
  hipStream_t st = as_stream(stream);
  unsigned* winner = reinterpret_cast<unsigned*>(workspace);
  unsigned long long* key = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + key_off);
  const long long clear_blocks = (need / 16 + TPB - 1) / TPB;
  hipLaunchKernelGGL(k_radar_clear, dim3((unsigned)(clear_blocks < 2048 ? (clear_blocks > 0 ? clear_blocks : 1) : 2048)), dim3(TPB), 0, st,
                     reinterpret_cast<unsigned long long*>(workspace), need / 8);
  Raster r;
  r.x1 = x1; r.y1 = y1; r.d1 = depth1; r.x2 = x2; r.y2 = y2; r.vc = v_comp; r.valid = valid; r.off = frame_offsets; r.K = K;
  r.B = B; r.n = n_points; r.k_stride = k_stride; r.h_out = h_out; r.w_new = w_new; r.y_cutoff = y_cutoff;
  r.s = (double)downsample_scale; r.x_hi = (double)(w_new - 1); r.y_hi = (double)(h_new - 1);
  if (n_points > 0) {
    hipLaunchKernelGGL(k_radar_min_depth, dim3(cdiv(n_points, TPB)), dim3(TPB), 0, st, r, key);
    hipLaunchKernelGGL(k_radar_min_index, dim3(cdiv(n_points, TPB)), dim3(TPB), 0, st, r, key, winner);
  }
  const long long n_quads = (n_pix + 3) / 4;
  const long long blocks = (n_quads + TPB - 1) / TPB;
  hipLaunchKernelGGL(k_radar_resolve, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(TPB), 0, st, r, winner, n_pix, radar, rad_vel);
  CRD_LAUNCH_CHECK("crd_radar_rasterize");
  return CRD_OK;
}
