// Radar front end on the device: accumulated radar sweeps -> the radar [B][H][W][3] and rad_vel [B][H][W] maps crd_assemble_input
// reads.  Two stages of the reference's offline preprocessing (lib/fuse_radar.py): the projection nested in merge_selected_radar
// (:30-74, :144-151) and the rasteriser cal_depthMap_flow (:156-204) + radarFlow2uv (:276-303).  All arithmetic is fp64, as NumPy's.
// The input is a few thousand detections; the only pass that touches every pixel is the resolve at the end.
#include "raster.h"       // the projection arithmetic, the z-buffer passes and the helpers of the resolve pass are shared with lidar_ops.hip

// the rasteriser is pinned bit for bit to NumPy, which never fuses a multiply into an add
#pragma clang fp contract(off)

namespace {

constexpr int TPB = ZBUF_TPB;

// fuse_radar.py:49-52 (Doppler compensation, then the pose chain) and view_points(..., normalize=True) of :69
__device__ __forceinline__ Cam project_one(const double* M, double lag, double x, double y, double z, double vx, double vy, const double* Kb) {
  const double xs = x + vx * lag, ys = y + vy * lag;
  double X, Y, Z;
  rigid(M, xs, ys, z, X, Y, Z);
  return pinhole(Kb, X, Y, Z);
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
    const Cam a = project_one(M1 + (long long)s * 12, lags[2 * s], x, y, z, vx, vy, Kb);
    const Cam c = project_one(M2 + (long long)s * 12, lags[2 * s + 1], x, y, z, vx, vy, Kb);
    o[0] = a.px; o[1] = a.py; o[2] = a.Z; o[3] = c.px; o[4] = c.py;
    o[5] = sqrt(vx * vx + vy * vy);
    ok = far_enough(x, y, min_dist) && in_view(a, min_z, im_w, im_h) && in_view(c, min_z, im_w, im_h);
  }
  x1[p] = o[0]; y1[p] = o[1]; d1[p] = o[2]; x2[p] = o[3]; y2[p] = o[4]; vc[p] = o[5];
  valid[p] = ok ? 1 : 0;
}

// ---- rasteriser ---------------------------------------------------------------------------------------------------------
// The four values of a won pixel (:187, :202, :284-295).  pix is its flat index, i its winner; r.extra is v_comp.
__device__ __forceinline__ void resolve_one(const Zbuf& r, long long pix, unsigned i, float& depth, float& u, float& v, float& vel) {
  const Pixel a = pixel_at(r, pix);
  double fx, fy;
  flow_of(r, i, fx, fy);
  depth = (float)r.d1[i];
  flow_uv(r, a, fx, fy, u, v);
  vel = r.extra[i] > 0.5 ? 1.f : 0.f;
}

// Pass 3: every pixel of radar [.][3] and rad_vel, four pixels (64 bytes out, 16 in) per thread; a quad nobody won is four vector stores
// of zeros, and almost every quad is one.  A winner is an index below n (NO_POINT is not): nothing read from the image is trusted.
__global__ __launch_bounds__(TPB) void k_radar_resolve(Zbuf r, const unsigned* winner, long long n_pix, float* radar, float* rad_vel) {
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
      store_quad3(radar, p0, o);
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
  CRD_CHECK_ARG(radar && rad_vel && (n_points == 0 || v_comp), "crd_radar_rasterize: null pointer (radar, rad_vel, v_comp)");
  CRD_CHECK_ARG(aligned16(radar) && aligned16(rad_vel), "crd_radar_rasterize: bad argument (radar and rad_vel must be 16-byte aligned)");
  hipStream_t st = as_stream(stream);
  Zbuf r;
  r.x1 = x1; r.y1 = y1; r.d1 = depth1; r.x2 = x2; r.y2 = y2; r.extra = v_comp; r.valid = valid; r.off = frame_offsets; r.K = K;
  ZbufImages im;
  const int rc = zbuf_passes("crd_radar_rasterize", r, B, n_points, k_stride, im_h, im_w, downsample_scale, y_cutoff, workspace,
                             workspace_bytes, [](long long key_end) { return key_end; }, st, im);
  if (rc != CRD_OK) return rc;
  hipLaunchKernelGGL(k_radar_resolve, dim3(quad_blocks(im.n_pix)), dim3(TPB), 0, st, r, im.winner, im.n_pix, radar, rad_vel);
  CRD_LAUNCH_CHECK("crd_radar_rasterize");
  return CRD_OK;
}
