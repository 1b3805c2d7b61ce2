// Lidar ground-truth front end on the device: accumulated lidar sweeps -> the gt [B][h][w][3] (depth, u, v), depth [B][h][w] and
// msk_lh [B][h][w] maps the reference prepares offline (lib/fuse_lidar.py, driven by scripts/cal_gt.py).  crd_lidar_project is
// current_to_global_at_ref_time + proj2im (:84-179) with the pose chains multiplied by the caller; crd_lidar_ground_truth is
// cal_depthMap_flow (:281-323), filter_occlusion_by_bbox (:634-676), filter_occlusion (:554-568) and lidarFlow2uv (:571-598).  All
// arithmetic is fp64, as NumPy's.  A key frame is about a million points on a third of a million pixels: the two atomic passes of the
// rasteriser are the hot path.
#include "common.h"
#include <string.h>

// the ground-truth stage is pinned bit for bit to NumPy, which never fuses a multiply into an add
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr unsigned NO_POINT = 0xffffffffu;
constexpr int ENTRY = 15;                      // doubles per box entry: box_from_sensor [3][4], then l/2, w/2, h/2

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

// M . (x, y, z, 1) for a row-major 3 x 4 matrix
__device__ __forceinline__ void rigid(const double* M, double x, double y, double z, double& X, double& Y, double& Z) {
  X = M[0] * x + M[1] * y + M[2] * z + M[3];
  Y = M[4] * x + M[5] * y + M[6] * z + M[7];
  Z = M[8] * x + M[9] * y + M[10] * z + M[11];
}

struct Project {
  const double* pts;
  const int32_t *sweep, *off;
  const double *cam1_s, *cam2_s, *car_z;
  const int32_t* sweep_boxes;
  const double* entries;
  const int32_t* box_id;
  const double *cam1_b, *cam2_b;
  const unsigned char* vehicle;
  const double* K;
  int B, n, n_sweeps, n_entries, n_boxes, k_stride;
  double im_h, im_w, min_dist, min_z, h_min, h_max;
  double *x1, *y1, *d1, *x2, *y2;
  unsigned char *low_h, *in_box, *valid;
  int32_t* box_entry;
};

// One thread per point.  The box entries of a sweep are a few tens of rows that every point of the sweep walks through, and the points
// of a sweep are contiguous: a wave takes the sweeps of its lanes one at a time (almost always there is one), so the sweep number, the
// entry index and with them every address of the table are wave-uniform -- the rows arrive through the scalar data cache, once per
// wave, not once per lane, and the six comparisons read them as scalar operands.  No lane leaves before the loop: the ballot
// counts all 64.  Every comparison is written so that a NaN fails it.
__global__ __launch_bounds__(TPB) void k_lidar_project(Project a) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  int b = -1, s = -1;
  double x = 0.0, y = 0.0, z = 0.0;
  if (p < a.n) {
    b = frame_of(a.off, a.B, p);
    s = a.sweep[p];
    if (b >= 0 && s >= 0 && s < a.n_sweeps) {
      const double* q = a.pts + (long long)p * 3;
      x = q[0]; y = q[1]; z = q[2];
    } else {
      s = -1;
    }
  }
  int hit = -1;                                // the first entry of the point's sweep whose box holds it
  double bx = 0.0, by = 0.0, bz = 0.0;         // the point in that box's frame
  unsigned long long pending = __ballot(s >= 0);
  while (pending) {
    const int lane = __builtin_amdgcn_readfirstlane(__ffsll((long long)pending) - 1);
    const int su = __builtin_amdgcn_readlane(s, lane);           // in [0, n_sweeps): only such lanes are pending
    const bool mine = s == su;
    int e0 = a.sweep_boxes[su], e1 = a.sweep_boxes[su + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > a.n_entries ? a.n_entries : e1;
    for (int e = e0; e < e1; ++e) {
      const double* E = a.entries + (long long)e * ENTRY;
      double X, Y, Z;
      rigid(E, x, y, z, X, Y, Z);
      const bool in = X > -E[12] && X < E[12] && Y > -E[13] && Y < E[13] && Z > -E[14] && Z < E[14];      // :132-137, all strict
      if (mine && hit < 0 && in) { hit = e; bx = X; by = Y; bz = Z; }
    }
    pending &= ~__ballot(mine);
  }
  if (p >= a.n) return;
  double o[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = false, low = false, boxed = false;
  int k = -1;
  if (hit >= 0) {
    k = a.box_id[hit];
    if (k < 0 || k >= a.n_boxes) s = -1;       // an entry that names no box: the point is invalid
  }
  if (s >= 0) {
    const double* c = a.car_z + (long long)s * 4;
    const double zc = c[0] * x + c[1] * y + c[2] * z + c[3];
    low = zc >= a.h_min && zc <= a.h_max;                                  // :54, both bounds inclusive
    double X1, Y1, Z1, X2, Y2, Z2;
    if (hit >= 0) {
      rigid(a.cam1_b + (long long)k * 12, bx, by, bz, X1, Y1, Z1);
      rigid(a.cam2_b + (long long)k * 12, bx, by, bz, X2, Y2, Z2);
      boxed = a.vehicle[k] != 0;                                           // :153
    } else {
      rigid(a.cam1_s + (long long)s * 12, x, y, z, X1, Y1, Z1);
      rigid(a.cam2_s + (long long)s * 12, x, y, z, X2, Y2, Z2);
    }
    const double* Kb = a.K + (long long)b * a.k_stride;
    const double fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
    o[0] = (fx * X1 + cx * Z1) / Z1; o[1] = (fy * Y1 + cy * Z1) / Z1; o[2] = Z1;        // view_points(normalize=True), :176
    o[3] = (fx * X2 + cx * Z2) / Z2; o[4] = (fy * Y2 + cy * Z2) / Z2;
    const bool far = fabs(x) >= a.min_dist || fabs(y) >= a.min_dist;       // remove_close: not (|x| < d and |y| < d)
    ok = far && Z1 >= a.min_z && Z2 >= a.min_z && o[0] > 0.0 && o[0] < a.im_w && o[1] > 0.0 && o[1] < a.im_h &&
         o[3] > 0.0 && o[3] < a.im_w && o[4] > 0.0 && o[4] < a.im_h;       // :175-178
  } else {
    hit = -1;
  }
  a.x1[p] = o[0]; a.y1[p] = o[1]; a.d1[p] = o[2]; a.x2[p] = o[3]; a.y2[p] = o[4];
  a.low_h[p] = low ? 1 : 0; a.in_box[p] = boxed ? 1 : 0; a.valid[p] = ok ? 1 : 0;
  a.box_entry[p] = hit;
}

// ---- ground truth -------------------------------------------------------------------------------------------------------
struct Raster {
  const double *x1, *y1, *d1, *x2, *y2;
  const unsigned char *low_h, *in_box;
  const unsigned char* valid;        // NULL: every point
  const int32_t* off;
  const double* K;
  int B, n, k_stride;
  int h_out, w_new, y_cutoff;        // h_out = h_new - y_cutoff rows are kept
  double s, x_hi, y_hi;              // downsample_scale, w_new - 1, h_new - 1
};

// fuse_lidar.py:293-301: pixel centres of the small image, clipped into it
__device__ __forceinline__ double scaled(double v, double s, double hi) { return fmin(fmax((v + 0.5) / s - 0.5, 0.0), hi); }

// The flat index of point p's pixel in the [B][h_out][w_new] images, or -1: the point is masked out, belongs to no frame, is one the
// reference would raise on (non-finite) or read as an empty pixel (depth <= 0), or falls on a row above the cutoff.  :305 rounds half
// to even (Python's round).
__device__ __forceinline__ long long pixel_of(const Raster& r, int p) {
  if (r.valid && !r.valid[p]) return -1;
  const int b = frame_of(r.off, r.B, p);
  if (b < 0) return -1;
  const double x1 = r.x1[p], y1 = r.y1[p], d = r.d1[p];
  if (!(finite_d(x1) && finite_d(y1) && finite_d(r.x2[p]) && finite_d(r.y2[p]) && finite_d(d) && d > 0.0)) return -1;
  const int col = (int)rint(scaled(x1, r.s, r.x_hi));
  const int row = (int)rint(scaled(y1, r.s, r.y_hi)) - r.y_cutoff;
  if (row < 0) return -1;
  return ((long long)b * r.h_out + row) * r.w_new + col;                // row < h_out, col < w_new: the clip
}

// Pass 0: the key images to all ones -- no point (winner), above every depth (key).  n_words 8-byte words from a 16-byte boundary.
__global__ __launch_bounds__(TPB) void k_lidar_clear(unsigned long long* ws, long long n_words) {
  const long long n_vec = n_words >> 1, t = (long long)blockIdx.x * TPB + threadIdx.x;
  for (long long v = t; v < n_vec; v += (long long)gridDim.x * TPB)
    reinterpret_cast<uint4*>(ws)[v] = make_uint4(NO_POINT, NO_POINT, NO_POINT, NO_POINT);
  if ((n_words & 1) && t == 0) ws[n_words - 1] = ~0ull;
}

// Pass 1: the smallest depth of every pixel.  Positive doubles order as their bit patterns do, so an unsigned 64-bit minimum is exact
// and does not depend on the order of arrival.  A key only ever falls, so a plain read that already shows a depth at or below this
// point's settles it without an atomic: with three points to a pixel and more on near surfaces most points take that way out.
__global__ __launch_bounds__(TPB) void k_lidar_min_depth(Raster r, unsigned long long* key) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= r.n) return;
  const long long pix = pixel_of(r, p);
  if (pix < 0) return;
  const unsigned long long mine = (unsigned long long)__double_as_longlong(r.d1[p]);
  if (__hip_atomic_load(key + pix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= mine) return;
  __hip_atomic_fetch_min(key + pix, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 2: among the points that have that depth the lowest index wins -- the reference's loop (:308-317) replaces on a strictly
// smaller depth only, so the first of equal depths stays.
__global__ __launch_bounds__(TPB) void k_lidar_min_index(Raster r, const unsigned long long* key, unsigned* winner) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= r.n) return;
  const long long pix = pixel_of(r, p);
  if (pix < 0) return;
  if (key[pix] != (unsigned long long)__double_as_longlong(r.d1[p])) return;
  if (__hip_atomic_load(winner + pix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)p) return;
  __hip_atomic_fetch_min(winner + pix, (unsigned)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The rectangle and depth bound of one box in the output map (:650-668), 32 bytes per box: column and row ranges (inclusive), d_max.
struct Rect { int x0, x1, y0, y1; double d_max; double pad; };

// One thread per box: corners fp64 [n][8][4] = x, y, depth, in_view.  The rectangle spans the in-view corners only, d_max all eight.
// A box with no corner in view, or with a value the reference would raise on (a non-finite coordinate of an in-view corner), gets
// an empty rectangle.
__global__ __launch_bounds__(TPB) void k_lidar_boxes(const double* corners, int n, Raster r, Rect* rects) {
  const int j = blockIdx.x * TPB + threadIdx.x;
  if (j >= n) return;
  const double* c = corners + (long long)j * 32;
  double xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY, dm = -INFINITY;
  bool any = false, bad = false;
  for (int i = 0; i < 8; ++i) {
    const double x = c[4 * i], y = c[4 * i + 1], d = c[4 * i + 2];
    dm = (d > dm || d != d) ? d : dm;                                      // np.max: a NaN stays
    if (c[4 * i + 3] != 0.0) {
      any = true;
      bad = bad || !(finite_d(x) && finite_d(y));
      const double xs = fmin(fmax((x + 0.5) / r.s - 0.5, 0.0), r.x_hi);
      const double ys = fmin(fmax(((y + 0.5) / r.s - 0.5) - (double)r.y_cutoff, 0.0), (double)(r.h_out - 1));
      xlo = fmin(xlo, xs); xhi = fmax(xhi, xs); ylo = fmin(ylo, ys); yhi = fmax(yhi, ys);
    }
  }
  Rect o;
  o.x0 = 1; o.x1 = 0; o.y0 = 1; o.y1 = 0; o.d_max = dm; o.pad = 0.0;
  if (any && !bad) { o.x0 = (int)rint(xlo); o.x1 = (int)rint(xhi); o.y0 = (int)rint(ylo); o.y1 = (int)rint(yhi); }
  rects[j] = o;
}

struct Filters {
  const unsigned char* seg;          // NULL: no box filter
  const Rect* rects;
  const int32_t* box_off;            // [B + 1]: frame b owns the boxes box_off[b] .. box_off[b + 1] - 1
  int n_boxes;
  const float* flow_im;              // NULL: no flow filter
  double thres;
};

// What is left of a won pixel after both filters, and its u, v (:571-598).  pix is its flat index, i its winner.
__device__ __forceinline__ void resolve_one(const Raster& r, const Filters& f, long long pix, unsigned i, float& depth, float& u, float& v,
                                            unsigned char& lh) {
  const long long per = (long long)r.h_out * r.w_new;
  const int b = (int)(pix / per);
  const int rem = (int)(pix - b * per);
  const int row = rem / r.w_new, col = rem - row * r.w_new;
  const double d = r.d1[i];
  if (f.seg && f.seg[pix] && !r.in_box[i]) {                               // :672
    int j0 = f.box_off[b], j1 = f.box_off[b + 1];
    j0 = j0 < 0 ? 0 : j0;
    j1 = j1 > f.n_boxes ? f.n_boxes : j1;
    for (int j = j0; j < j1; ++j) {
      const Rect q = f.rects[j];
      if (col >= q.x0 && col <= q.x1 && row >= q.y0 && row <= q.y1 && d > q.d_max) return;
    }
  }
  const double xa = scaled(r.x1[i], r.s, r.x_hi), ya = scaled(r.y1[i], r.s, r.y_hi);
  const double xb = scaled(r.x2[i], r.s, r.x_hi), yb = scaled(r.y2[i], r.s, r.y_hi);
  const double fx_ = xb - xa, fy_ = yb - ya;                               // :310
  if (f.flow_im) {                                                         // :557-560
    const double ex = fx_ - (double)f.flow_im[pix * 2], ey = fy_ - (double)f.flow_im[pix * 2 + 1];
    if (sqrt(ex * ex + ey * ey) > f.thres) return;
  }
  const float xm = (float)((double)col + fx_);                             // x_map is float32 (:581-582); the sum is rounded once into it
  const float ym = (float)((double)row + fy_);
  const double* Kb = r.K + (long long)b * r.k_stride;
  const double fl = Kb[0] / r.s, cx = Kb[2] / r.s, cy = Kb[5] / r.s - (double)r.y_cutoff;      // :585-587; fx divides both (:589-590)
  depth = (float)d;
  u = (float)(((double)xm - cx) / fl);
  v = (float)(((double)ym - cy) / fl);
  lh = r.low_h[i] ? 1 : 0;
}

// Pass 3: every pixel of gt [.][3], depth and msk_lh, four pixels per thread.  A winner is an index below n (NO_POINT is not): nothing
// read from the image is trusted.
__global__ __launch_bounds__(TPB) void k_lidar_resolve(Raster r, Filters f, const unsigned* winner, long long n_pix, float* gt, float* depth,
                                                       unsigned char* msk) {
  const long long n_quads = (n_pix + 3) >> 2;
  for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (long long)gridDim.x * TPB) {
    const long long p0 = q * 4;
    if (p0 + 4 <= n_pix) {
      float o[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dep[4] = {0.f, 0.f, 0.f, 0.f};
      unsigned char lh[4] = {0, 0, 0, 0};
      const uint4 w = *reinterpret_cast<const uint4*>(winner + p0);
      const unsigned wi[4] = {w.x, w.y, w.z, w.w};
      if ((w.x & w.y & w.z & w.w) != NO_POINT) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (wi[k] < (unsigned)r.n) {
            resolve_one(r, f, p0 + k, wi[k], o[3 * k], o[3 * k + 1], o[3 * k + 2], lh[k]);
            dep[k] = o[3 * k];
          }
      }
      float4* dst = reinterpret_cast<float4*>(gt + p0 * 3);
      dst[0] = make_float4(o[0], o[1], o[2], o[3]);
      dst[1] = make_float4(o[4], o[5], o[6], o[7]);
      dst[2] = make_float4(o[8], o[9], o[10], o[11]);
      *reinterpret_cast<float4*>(depth + p0) = make_float4(dep[0], dep[1], dep[2], dep[3]);
      *reinterpret_cast<unsigned*>(msk + p0) = (unsigned)lh[0] | ((unsigned)lh[1] << 8) | ((unsigned)lh[2] << 16) | ((unsigned)lh[3] << 24);
    } else {                                                              // the last, short quad
      for (long long p = p0; p < n_pix; ++p) {
        float d = 0.f, u = 0.f, v = 0.f;
        unsigned char m = 0;
        const unsigned i = winner[p];
        if (i < (unsigned)r.n) resolve_one(r, f, p, i, d, u, v, m);
        gt[p * 3] = d; gt[p * 3 + 1] = u; gt[p * 3 + 2] = v;
        depth[p] = d;
        msk[p] = m;
      }
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }

}  // namespace

extern "C" int crd_lidar_project(const double* points, const int32_t* sweep_index, const int32_t* frame_offsets, int32_t B,
                                 int32_t n_points, const double* cam1_from_sensor, const double* cam2_from_sensor,
                                 const double* car_z_from_sensor, const int32_t* sweep_boxes, int32_t n_sweeps, const double* box_entries,
                                 const int32_t* box_id, int32_t n_entries, const double* cam1_from_box, const double* cam2_from_box,
                                 const uint8_t* vehicle, int32_t n_boxes, const double* K, int32_t k_stride, int32_t im_h, int32_t im_w,
                                 float min_distance, float min_z, uint64_t h_min_f64_bits, uint64_t h_max_f64_bits, double* x1, double* y1,
                                 double* depth1, double* x2, double* y2, uint8_t* low_h, uint8_t* in_box, uint8_t* valid,
                                 int32_t* box_entry, crd_stream_t stream) {
  CRD_CHECK_ARG(B > 0 && B <= 65535 && n_points >= 0 && n_sweeps >= 0 && n_entries >= 0 && n_boxes >= 0 && im_h > 0 && im_w > 0,
                "crd_lidar_project: bad argument (B %d, n_points %d, n_sweeps %d, n_entries %d, n_boxes %d, image %d x %d)", B, n_points,
                n_sweeps, n_entries, n_boxes, im_h, im_w);
  CRD_CHECK_ARG(k_stride == 0 || k_stride == 9, "crd_lidar_project: bad argument (k_stride %d is neither 0 nor 9)", k_stride);
  CRD_CHECK_ARG(min_distance >= 0.f && min_z == min_z, "crd_lidar_project: bad argument (min_distance %g, min_z %g)",
                (double)min_distance, (double)min_z);
  const double h_min = from_bits(h_min_f64_bits), h_max = from_bits(h_max_f64_bits);
  CRD_CHECK_ARG(h_min == h_min && h_max == h_max, "crd_lidar_project: bad argument (h_min %g, h_max %g)", h_min, h_max);
  if (n_points == 0) return CRD_OK;
  CRD_CHECK_ARG(points && sweep_index && frame_offsets && K && x1 && y1 && depth1 && x2 && y2 && low_h && in_box && valid && box_entry,
                "crd_lidar_project: null pointer");
  CRD_CHECK_ARG(n_sweeps == 0 || (cam1_from_sensor && cam2_from_sensor && car_z_from_sensor && sweep_boxes),
                "crd_lidar_project: null pointer (sweep tables)");
  CRD_CHECK_ARG(n_entries == 0 || (box_entries && box_id && cam1_from_box && cam2_from_box && vehicle),
                "crd_lidar_project: null pointer (box tables)");
  Project a;
  a.pts = points; a.sweep = sweep_index; a.off = frame_offsets; a.cam1_s = cam1_from_sensor; a.cam2_s = cam2_from_sensor;
  a.car_z = car_z_from_sensor; a.sweep_boxes = sweep_boxes; a.entries = box_entries; a.box_id = box_id; a.cam1_b = cam1_from_box;
  a.cam2_b = cam2_from_box; a.vehicle = vehicle; a.K = K; a.B = B; a.n = n_points; a.n_sweeps = n_sweeps; a.n_entries = n_entries;
  a.n_boxes = n_boxes; a.k_stride = k_stride; a.im_h = (double)im_h; a.im_w = (double)im_w; a.min_dist = (double)min_distance;
  a.min_z = (double)min_z; a.h_min = h_min; a.h_max = h_max; a.x1 = x1; a.y1 = y1; a.d1 = depth1; a.x2 = x2; a.y2 = y2;
  a.low_h = low_h; a.in_box = in_box; a.valid = valid; a.box_entry = box_entry;
  hipLaunchKernelGGL(k_lidar_project, dim3(cdiv(n_points, TPB)), dim3(TPB), 0, as_stream(stream), a);
  CRD_LAUNCH_CHECK("crd_lidar_project");
  return CRD_OK;
}

extern "C" int crd_lidar_ground_truth(const double* x1, const double* y1, const double* depth1, const double* x2, const double* y2,
                                      const uint8_t* low_h, const uint8_t* in_box, const uint8_t* valid, const int32_t* frame_offsets,
                                      int32_t B, int32_t n_points, const double* K, int32_t k_stride, int32_t im_h, int32_t im_w,
                                      int32_t downsample_scale, int32_t y_cutoff, const uint8_t* seg, const double* corners,
                                      const int32_t* corner_offsets, int32_t n_boxes, const float* flow_im, uint64_t thres_f64_bits,
                                      void* workspace, int64_t workspace_bytes, float* gt, float* depth, uint8_t* msk_lh,
                                      crd_stream_t stream) {
  CRD_CHECK_ARG(B > 0 && B <= 65535 && n_points >= 0 && n_boxes >= 0 && im_h > 0 && im_w > 0 && downsample_scale > 0,
                "crd_lidar_ground_truth: bad argument (B %d, n_points %d, n_boxes %d, image %d x %d, downsample_scale %d)", B, n_points,
                n_boxes, im_h, im_w, downsample_scale);
  const int h_new = im_h / downsample_scale, w_new = im_w / downsample_scale;
  CRD_CHECK_ARG(h_new > 0 && w_new > 0, "crd_lidar_ground_truth: bad argument (downsample_scale %d leaves no pixel of %d x %d)",
                downsample_scale, im_h, im_w);
  CRD_CHECK_ARG(y_cutoff >= 0 && y_cutoff < h_new, "crd_lidar_ground_truth: bad argument (y_cutoff %d outside [0, %d))", y_cutoff, h_new);
  CRD_CHECK_ARG(k_stride == 0 || k_stride == 9, "crd_lidar_ground_truth: bad argument (k_stride %d is neither 0 nor 9)", k_stride);
  const double thres = from_bits(thres_f64_bits);
  CRD_CHECK_ARG(!flow_im || thres == thres, "crd_lidar_ground_truth: bad argument (thres is NaN)");
  CRD_CHECK_ARG(K && workspace && gt && depth && msk_lh, "crd_lidar_ground_truth: null pointer");
  CRD_CHECK_ARG(n_points == 0 || (x1 && y1 && depth1 && x2 && y2 && low_h && in_box && frame_offsets),
                "crd_lidar_ground_truth: null pointer (points)");
  CRD_CHECK_ARG((seg != nullptr) == (corner_offsets != nullptr) && (!seg || n_boxes == 0 || corners),
                "crd_lidar_ground_truth: bad argument (the box filter takes seg, corners and corner_offsets together)");
  const int h_out = h_new - y_cutoff;
  const long long n_pix = (long long)B * h_out * w_new;
  const long long key_off = (n_pix * 4 + 15) & ~15ll, rect_off = (key_off + n_pix * 8 + 15) & ~15ll;
  const long long need = rect_off + (seg ? 32ll * n_boxes : 0ll);
  CRD_CHECK_ARG(workspace_bytes >= need, "crd_lidar_ground_truth: the workspace holds %lld bytes, %lld are needed",
                (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace) && aligned16(gt) && aligned16(depth) && (reinterpret_cast<uintptr_t>(msk_lh) & 3) == 0,
                "crd_lidar_ground_truth: bad argument (workspace, gt and depth must be 16-byte aligned, msk_lh 4-byte aligned)");
  hipStream_t st = as_stream(stream);
  unsigned* winner = reinterpret_cast<unsigned*>(workspace);
  unsigned long long* key = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + key_off);
  Rect* rects = reinterpret_cast<Rect*>(reinterpret_cast<char*>(workspace) + rect_off);
  const long long clear_words = rect_off / 8, clear_blocks = (clear_words / 2 + TPB - 1) / TPB;
  hipLaunchKernelGGL(k_lidar_clear, dim3((unsigned)(clear_blocks < 2048 ? (clear_blocks > 0 ? clear_blocks : 1) : 2048)), dim3(TPB), 0, st,
                     reinterpret_cast<unsigned long long*>(workspace), clear_words);
  Raster r;
  r.x1 = x1; r.y1 = y1; r.d1 = depth1; r.x2 = x2; r.y2 = y2; r.low_h = low_h; r.in_box = in_box; r.valid = valid;
  r.off = frame_offsets; r.K = K; r.B = B; r.n = n_points; r.k_stride = k_stride; r.h_out = h_out; r.w_new = w_new;
  r.y_cutoff = y_cutoff; r.s = (double)downsample_scale; r.x_hi = (double)(w_new - 1); r.y_hi = (double)(h_new - 1);
  Filters f;
  f.seg = seg; f.rects = rects; f.box_off = corner_offsets; f.n_boxes = n_boxes; f.flow_im = flow_im; f.thres = thres;
  if (seg && n_boxes > 0) hipLaunchKernelGGL(k_lidar_boxes, dim3(cdiv(n_boxes, TPB)), dim3(TPB), 0, st, corners, n_boxes, r, rects);
  if (n_points > 0) {
    hipLaunchKernelGGL(k_lidar_min_depth, dim3(cdiv(n_points, TPB)), dim3(TPB), 0, st, r, key);
    hipLaunchKernelGGL(k_lidar_min_index, dim3(cdiv(n_points, TPB)), dim3(TPB), 0, st, r, key, winner);
  }
  const long long n_quads = (n_pix + 3) / 4;
  const long long blocks = (n_quads + TPB - 1) / TPB;
  hipLaunchKernelGGL(k_lidar_resolve, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(TPB), 0, st, r, f, winner, n_pix, gt, depth,
                     msk_lh);
  CRD_LAUNCH_CHECK("crd_lidar_ground_truth");
  return CRD_OK;
}
