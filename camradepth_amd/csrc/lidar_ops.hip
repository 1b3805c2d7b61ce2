// Lidar ground-truth front end on the device: accumulated lidar sweeps -> the gt [B][h][w][3] (depth, u, v), depth [B][h][w] and
// msk_lh [B][h][w] maps the reference prepares offline (lib/fuse_lidar.py, driven by scripts/cal_gt.py).  crd_lidar_project is
// current_to_global_at_ref_time + proj2im (:84-179) with the pose chains multiplied by the caller; crd_lidar_ground_truth is
// cal_depthMap_flow (:281-323), filter_occlusion_by_bbox (:634-676), filter_occlusion (:554-568) and lidarFlow2uv (:571-598).  All
// arithmetic is fp64, as NumPy's.  A key frame is about a million points on a third of a million pixels: the two atomic passes of the
// rasteriser are the hot path.
#include "raster.h"       // the projection arithmetic, the z-buffer passes and the helpers of the resolve pass are shared with radar_ops.hip
#include <string.h>

// the ground-truth stage is pinned bit for bit to NumPy, which never fuses a multiply into an add
#pragma clang fp contract(off)

namespace {

constexpr int TPB = ZBUF_TPB;
constexpr int ENTRY = 15;                      // doubles per box entry: box_from_sensor [3][4], then l/2, w/2, h/2

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
    const Cam c1 = pinhole(Kb, X1, Y1, Z1), c2 = pinhole(Kb, X2, Y2, Z2);                // view_points(normalize=True), :176
    o[0] = c1.px; o[1] = c1.py; o[2] = c1.Z; o[3] = c2.px; o[4] = c2.py;
    ok = far_enough(x, y, a.min_dist) && in_view(c1, a.min_z, a.im_w, a.im_h) && in_view(c2, a.min_z, a.im_w, a.im_h);      // :175-178
  } else {
    hit = -1;
  }
  a.x1[p] = o[0]; a.y1[p] = o[1]; a.d1[p] = o[2]; a.x2[p] = o[3]; a.y2[p] = o[4];
  a.low_h[p] = low ? 1 : 0; a.in_box[p] = boxed ? 1 : 0; a.valid[p] = ok ? 1 : 0;
  a.box_entry[p] = hit;
}

// ---- ground truth -------------------------------------------------------------------------------------------------------
// The rectangle and depth bound of one box in the output map (:650-668), 32 bytes per box: column and row ranges (inclusive), d_max.
struct Rect { int x0, x1, y0, y1; double d_max; double pad; };

// One thread per box: corners fp64 [n][8][4] = x, y, depth, in_view.  The rectangle spans the in-view corners only, d_max all eight.
// A box with no corner in view, or with a value the reference would raise on (a non-finite coordinate of an in-view corner), gets
// an empty rectangle.
__global__ __launch_bounds__(TPB) void k_lidar_boxes(const double* corners, int n, Zbuf r, Rect* rects) {
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
      const double xs = scaled(x, r.s, r.x_hi);
      const double ys = fmin(fmax(to_small(y, r.s) - (double)r.y_cutoff, 0.0), (double)(r.h_out - 1));
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
  const unsigned char *low_h, *in_box;         // per point, from the projection
};

// What is left of a won pixel after both filters, and its u, v (:571-598).  pix is its flat index, i its winner.
__device__ __forceinline__ void resolve_one(const Zbuf& r, const Filters& f, long long pix, unsigned i, float& depth, float& u, float& v,
                                            unsigned char& lh) {
  const Pixel a = pixel_at(r, pix);
  const int b = a.b, row = a.row, col = a.col;         // (as locals: through `a` the kernel, at its SGPR limit, spills scalars into vector lanes)
  const double d = r.d1[i];
  if (f.seg && f.seg[pix] && !f.in_box[i]) {                               // :672
    int j0 = f.box_off[b], j1 = f.box_off[b + 1];
    j0 = j0 < 0 ? 0 : j0;
    j1 = j1 > f.n_boxes ? f.n_boxes : j1;
    for (int j = j0; j < j1; ++j) {
      const Rect q = f.rects[j];
      if (col >= q.x0 && col <= q.x1 && row >= q.y0 && row <= q.y1 && d > q.d_max) return;
    }
  }
  double fx_, fy_;                                                         // :310
  flow_of(r, i, fx_, fy_);
  if (f.flow_im) {                                                         // :557-560
    const double ex = fx_ - (double)f.flow_im[pix * 2], ey = fy_ - (double)f.flow_im[pix * 2 + 1];
    if (sqrt(ex * ex + ey * ey) > f.thres) return;
  }
  depth = (float)d;
  flow_uv(r, a, fx_, fy_, u, v);                                       // :581-590
  lh = f.low_h[i] ? 1 : 0;
}

// Pass 3: every pixel of gt [.][3], depth and msk_lh, four pixels per thread.  A winner is an index below n (NO_POINT is not): nothing
// read from the image is trusted.
__global__ __launch_bounds__(TPB) void k_lidar_resolve(Zbuf r, Filters f, const unsigned* winner, long long n_pix, float* gt, float* depth,
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
      store_quad3(gt, p0, o);
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
  CRD_CHECK_ARG(n_boxes >= 0, "crd_lidar_ground_truth: bad argument (n_boxes %d)", n_boxes);
  const double thres = from_bits(thres_f64_bits);
  CRD_CHECK_ARG(!flow_im || thres == thres, "crd_lidar_ground_truth: bad argument (thres is NaN)");
  CRD_CHECK_ARG(gt && depth && msk_lh && (n_points == 0 || (low_h && in_box)),
                "crd_lidar_ground_truth: null pointer (gt, depth, msk_lh, low_h, in_box)");
  CRD_CHECK_ARG((seg != nullptr) == (corner_offsets != nullptr) && (!seg || n_boxes == 0 || corners),
                "crd_lidar_ground_truth: bad argument (the box filter takes seg, corners and corner_offsets together)");
  CRD_CHECK_ARG(aligned16(gt) && aligned16(depth) && (reinterpret_cast<uintptr_t>(msk_lh) & 3) == 0,
                "crd_lidar_ground_truth: bad argument (gt and depth must be 16-byte aligned, msk_lh 4-byte aligned)");
  hipStream_t st = as_stream(stream);
  Zbuf r;
  r.x1 = x1; r.y1 = y1; r.d1 = depth1; r.x2 = x2; r.y2 = y2; r.extra = nullptr; r.valid = valid; r.off = frame_offsets; r.K = K;
  ZbufImages im;
  const long long rect_bytes = seg ? 32ll * n_boxes : 0ll;                 // the rectangles lie behind the key images, from a 16-byte boundary
  const int rc = zbuf_passes("crd_lidar_ground_truth", r, B, n_points, k_stride, im_h, im_w, downsample_scale, y_cutoff, workspace,
                             workspace_bytes, [=](long long key_end) { return ((key_end + 15) & ~15ll) + rect_bytes; }, st, im);
  if (rc != CRD_OK) return rc;
  Filters f;
  f.low_h = low_h; f.in_box = in_box; f.seg = seg; f.box_off = corner_offsets; f.n_boxes = n_boxes; f.flow_im = flow_im; f.thres = thres;
  Rect* rects = reinterpret_cast<Rect*>(reinterpret_cast<char*>(workspace) + ((im.key_end + 15) & ~15ll));
  f.rects = rects;
  if (seg && n_boxes > 0) hipLaunchKernelGGL(k_lidar_boxes, dim3(cdiv(n_boxes, TPB)), dim3(TPB), 0, st, corners, n_boxes, r, rects);
  hipLaunchKernelGGL(k_lidar_resolve, dim3(quad_blocks(im.n_pix)), dim3(TPB), 0, st, r, f, im.winner, im.n_pix, gt, depth, msk_lh);
  CRD_LAUNCH_CHECK("crd_lidar_ground_truth");
  return CRD_OK;
}
