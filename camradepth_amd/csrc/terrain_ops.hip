// Terrain map on the device: a point cloud (the forms bev_ops.hip takes) -> a ground height per cell of occupancy_ops.hip's rolling
// window, fused over frames in integers of z_quantum metres, and the traversability of every cell from local height differences: the
// step inside it, the step to its neighbours, the slope.  Per cell and call the lowest point and the highest one within the headroom
// above it, both as order-independent int32 atomics.  Five launches on the caller's stream (prepare, points A, points B, fuse, derive);
// no workgroup waits for another.  The rows' arithmetic is fp64 add, multiply, divide, floor and compare; the cells' is integer
// (terrain_cell.h).
#include "raster.h"       // frame_of, rigid, finite_d, aligned16
#include "terrain_cell.h"
#include <string.h>

// the results are specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr double ORIGIN_LIMIT = 2147418112.0;        // 2^31 - 65536: a window of up to 65535 cells around it stays inside int32
constexpr int SKIPPED = 2, WAS_INITIALISED = 1;      // flags[m] of one call
constexpr int32_t NO_LO = INT32_MAX, NO_HI = INT32_MIN;
constexpr double Q_LIMIT = 16777216.0;               // 2^24: every height in quanta stays below it

struct Ter {
  const float* xyz;
  const unsigned char* valid;                        // may be NULL
  const int32_t* off;                                // NULL: frame b owns the rows b * rows_per_frame ..
  const double *T, *sensor, *centre;                 // each may be NULL: the identity, the origin, the sensor
  int B, n, rows_per_frame, t_stride, s_stride, c_stride, M, nx, ny, head_q, min_points, w_max, step_max_q;
  long long slope2_max;
  double cell, max_r2, z_quantum, z_min, z_max;
  int32_t *ground, *top;                             // the caller's state
  int16_t* weight;
  long long *prev, *cur;
  int32_t *initialised, *status;
  int32_t *lo, *hi, *count;                          // the workspace
  double* S;
  int32_t* flags;
};

// T_b . v for a point v of the points' frame (NULL: the origin)
__device__ __forceinline__ void to_map(const Ter& a, int b, const double* v, double& X, double& Y, double& Z) {
  const double x = v ? v[0] : 0.0, y = v ? v[1] : 0.0, z = v ? v[2] : 0.0;
  X = x; Y = y; Z = z;
  if (a.T) rigid(a.T + (long long)b * a.t_stride, x, y, z, X, Y, Z);
}

// Launch 1: this call's observation cleared, every frame's sensor in the map frame, every map's window moved (k_occ_prepare's rule).
__global__ __launch_bounds__(TPB) void k_ter_prepare(Ter a, long long n_cells) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
  for (long long i = t; i < n_cells; i += step) {
    a.lo[i] = NO_LO;
    a.hi[i] = NO_HI;
    a.count[i] = 0;
  }
  for (long long b = t; b < a.B; b += step) {
    double X, Y, Z;
    to_map(a, (int)b, a.sensor ? a.sensor + b * a.s_stride : nullptr, X, Y, Z);
    a.S[b * 3] = X; a.S[b * 3 + 1] = Y; a.S[b * 3 + 2] = Z;
    if (!(finite_d(X) && finite_d(Y) && finite_d(Z)))
      __hip_atomic_fetch_or(a.status + (a.M == 1 ? 0 : b), 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (long long m = t; m < a.M; m += step) {
    const int b = a.M == 1 ? 0 : (int)m;
    const double* c = a.centre ? a.centre + (long long)b * a.c_stride : (a.sensor ? a.sensor + (long long)b * a.s_stride : nullptr);
    double X, Y, Z;
    to_map(a, b, c, X, Y, Z);
    const double fx = floor(X / a.cell), fy = floor(Y / a.cell);
    const bool ok = finite_d(X) && finite_d(Y) && finite_d(Z) && fabs(fx) < ORIGIN_LIMIT && fabs(fy) < ORIGIN_LIMIT;
    a.flags[m] = (a.initialised[m] != 0 ? WAS_INITIALISED : 0) | (ok ? 0 : SKIPPED);
    if (ok) {
      a.prev[m * 2] = a.cur[m * 2];
      a.prev[m * 2 + 1] = a.cur[m * 2 + 1];
      a.cur[m * 2] = (long long)fx - a.nx / 2;
      a.cur[m * 2 + 1] = (long long)fy - a.ny / 2;
    } else {
      __hip_atomic_fetch_or(a.status + m, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// What row p brings: the flat index c of the window cell it falls into (c < 0: nothing) and its height q in quanta
struct Row { int c, q; };

__device__ __forceinline__ Row row_of(const Ter& a, int p) {
  Row r = {-1, 0};
  if (a.valid && !a.valid[p]) return r;
  const int b = a.off ? frame_of(a.off, a.B, p) : p / a.rows_per_frame;
  if (b < 0 || b >= a.B) return r;
  const float* s = a.xyz + (long long)p * 3;
  double X = (double)s[0], Y = (double)s[1], Z = (double)s[2];
  if (a.T) rigid(a.T + (long long)b * a.t_stride, (double)s[0], (double)s[1], (double)s[2], X, Y, Z);
  const double Sx = a.S[b * 3], Sy = a.S[b * 3 + 1], Sz = a.S[b * 3 + 2];
  if (!(finite_d(X) && finite_d(Y) && finite_d(Z) && finite_d(Sx) && finite_d(Sy) && finite_d(Sz))) return r;
  const double dx = X - Sx, dy = Y - Sy, r2 = dx * dx + dy * dy;
  if (r2 > a.max_r2) return r;
  if (Z < a.z_min || Z > a.z_max) return r;
  const int m = a.M == 1 ? 0 : b;
  const long long ox = a.cur[m * 2], oy = a.cur[m * 2 + 1];
  const double wx = floor(X / a.cell), wy = floor(Y / a.cell);
  if (!(wx >= (double)ox && wx < (double)(ox + a.nx) && wy >= (double)oy && wy < (double)(oy + a.ny))) return r;   // on the doubles
  const long long i = (long long)wx - ox, j = (long long)wy - oy;
  if (i < 0 || i >= a.nx || j < 0 || j >= a.ny) return r;            // never with an origin launch 1 wrote: the caller's may be anything
  r.q = (int)floor(Z / a.z_quantum);                                  // |Z| / z_quantum < 2^24 by the entry's check of z_min and z_max
  r.c = (m * a.nx + (int)i) * a.ny + (int)j;
  return r;
}

// The end of the run of equal keys among neighbouring lanes that this lane belongs to, and whether the lane is its head
// (occupancy_ops.hip's run_end)
__device__ __forceinline__ int run_end(int key, int lane, bool& head) {
  const int before = __shfl_up(key, 1);
  const unsigned long long heads = __ballot(lane == 0 || before != key);
  const unsigned long long later = lane == CRD_WAVE - 1 ? 0ull : heads >> (lane + 1);
  head = (heads >> lane) & 1ull;
  return later ? lane + __ffsll(later) : CRD_WAVE;
}

// Launch 2: one thread per row.  A cloud in image order puts thousands of neighbouring pixels of the road into one cell near the
// vehicle, and a hot address serialises its atomics, so each run of equal cells among the neighbouring lanes of a wave is folded first
// -- the heights by a segmented minimum, the count as the run's length -- and its first lane alone goes to memory (k_occ_points's
// fold): integer minimum and sum, the same in any grouping.  lo only falls, so a plain read that already shows a height at or below
// the run's settles it without an atomic.
__global__ __launch_bounds__(TPB) void k_ter_points_lo(Ter a) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & (CRD_WAVE - 1);
  Row r = {-1, 0};
  if (t < a.n) r = row_of(a, (int)t);                                 // every lane stays for the wave operations
  bool head;
  const int end = run_end(r.c, lane, head);
  int q = r.q;
#pragma unroll
  for (int d = 1; d < CRD_WAVE; d <<= 1) {                            // afterwards q of a head covers its whole run
    const int o = __shfl_down(q, d);
    if (lane + d < end) q = o < q ? o : q;
  }
  if (r.c >= 0 && head) {
    if (__hip_atomic_load(a.lo + r.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > q)
      __hip_atomic_fetch_min(a.lo + r.c, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(a.count + r.c, end - lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Launch 3: one thread per row, the same arithmetic again.  lo is final because launch 2 has ended; a row within the headroom above
// its cell's lowest point is a candidate for hi, folded and settled as in launch 2 with the maximum.
__global__ __launch_bounds__(TPB) void k_ter_points_hi(Ter a) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & (CRD_WAVE - 1);
  Row r = {-1, 0};
  if (t < a.n) r = row_of(a, (int)t);
  int q = NO_HI;
  if (r.c >= 0 && (long long)r.q <= (long long)a.lo[r.c] + a.head_q) q = r.q;
  bool head;
  const int end = run_end(r.c, lane, head);
#pragma unroll
  for (int d = 1; d < CRD_WAVE; d <<= 1) {
    const int o = __shfl_down(q, d);
    if (lane + d < end) q = o > q ? o : q;
  }
  if (r.c >= 0 && head && q != NO_HI && __hip_atomic_load(a.hi + r.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < q)
    __hip_atomic_fetch_max(a.hi + r.c, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct Cell { int m, i, j, rem; };

__device__ __forceinline__ Cell cell_at(const Ter& a, long long idx) {
  const unsigned per = (unsigned)a.nx * (unsigned)a.ny;                // M * nx * ny < 2^31 by the entry's check: 32-bit division
  Cell c;
  c.m = (int)((unsigned)idx / per);
  c.rem = (int)((unsigned)idx - (unsigned)c.m * per);
  c.i = c.rem / a.ny;
  c.j = c.rem - c.i * a.ny;
  return c;
}

// w mod n, the mathematical modulo
__device__ __forceinline__ int wrapped(long long w, int n) {
  const long long s = w % n;
  return (int)(s < 0 ? s + n : s);
}

// The slot of window cell (i, j) of map m in the torus, with (ax, ay) = (ox mod nx, oy mod ny): ((ox + i) mod nx, (oy + j) mod ny)
// without a 64-bit division per cell, since ax + i < 2 nx
__device__ __forceinline__ long long slot_of(const Ter& a, int m, int ax, int ay, int i, int j) {
  int sx = ax + i, sy = ay + j;
  sx -= sx >= a.nx ? a.nx : 0;
  sy -= sy >= a.ny ? a.ny : 0;
  return ((long long)m * a.nx + sx) * a.ny + sy;
}

// Launch 4: one window cell per thread, its own slot fused in place (tc_fuse).  A skipped map is left alone.
__global__ __launch_bounds__(TPB) void k_ter_fuse(Ter a, long long n_cells) {
  for (long long idx = (long long)blockIdx.x * TPB + threadIdx.x; idx < n_cells; idx += (long long)gridDim.x * TPB) {
    const Cell c = cell_at(a, idx);
    const int flags = a.flags[c.m];
    if (flags & SKIPPED) continue;
    const long long ox = a.cur[c.m * 2], oy = a.cur[c.m * 2 + 1], wx = ox + c.i, wy = oy + c.j, px = a.prev[c.m * 2], py = a.prev[c.m * 2 + 1];
    const long long slot = slot_of(a, c.m, wrapped(ox, a.nx), wrapped(oy, a.ny), c.i, c.j);
    const bool kept = (flags & WAS_INITIALISED) && wx >= px && wx < px + a.nx && wy >= py && wy < py + a.ny;
    const TcFused f = tc_fuse(kept ? (int)a.weight[slot] : 0, a.ground[slot], a.top[slot], a.count[idx] >= a.min_points, a.lo[idx], a.hi[idx],
                              a.w_max);
    a.ground[slot] = f.ground;
    a.top[slot] = f.top;
    a.weight[slot] = (int16_t)f.weight;
  }
}

// Launch 5: one window cell per thread -- the 3 x 3 stencil on the fused torus (tc_derive) and the outputs in window order.  After
// launch 4 every slot belongs to the window cell it holds; a skipped map reads what the update before left, nothing if there was none.
__global__ __launch_bounds__(TPB) void k_ter_derive(Ter a, long long n_cells, int32_t* ground, int32_t* top, int32_t* step, long long* slope2,
                                                    int16_t* weight, unsigned char* state, unsigned char* hazard, unsigned char* evidence,
                                                    float* value, long long* origin) {
  for (long long idx = (long long)blockIdx.x * TPB + threadIdx.x; idx < n_cells; idx += (long long)gridDim.x * TPB) {
    const Cell c = cell_at(a, idx);
    const int flags = a.flags[c.m];
    const bool skipped = (flags & SKIPPED) != 0, holds = !skipped || (flags & WAS_INITIALISED);
    const long long ox = a.cur[c.m * 2], oy = a.cur[c.m * 2 + 1];
    const int ax = wrapped(ox, a.nx), ay = wrapped(oy, a.ny);
    int32_t g[9], w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int i = c.i + k / 3 - 1, j = c.j + k % 3 - 1;
      g[k] = 0;
      w[k] = 0;
      if (holds && i >= 0 && i < a.nx && j >= 0 && j < a.ny) {
        const long long slot = slot_of(a, c.m, ax, ay, i, j);
        w[k] = a.weight[slot];
        g[k] = a.ground[slot];
      }
    }
    const int32_t t = w[4] ? a.top[slot_of(a, c.m, ax, ay, c.i, c.j)] : 0;
    const TcDerived d = tc_derive(g, w, t, a.step_max_q, a.slope2_max);
    const bool known = w[4] != 0;
    ground[idx] = known ? g[4] : INT32_MIN;
    top[idx] = known ? t : INT32_MIN;
    step[idx] = d.step;
    slope2[idx] = d.slope2;
    weight[idx] = (int16_t)w[4];
    state[idx] = d.state;
    hazard[idx] = d.hazard;
    evidence[idx] = (unsigned char)(!skipped && a.count[idx] >= a.min_points);
    value[idx] = known ? (float)((double)g[4] * a.z_quantum) : __int_as_float(0x7fc00000);
    if (c.rem == 0) {
      origin[c.m * 2] = ox;
      origin[c.m * 2 + 1] = oy;
      if (!skipped) a.initialised[c.m] = 1;
    }
  }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf
inline long long up16(long long n) { return (n + 15) & ~15ll; }

}  // namespace

extern "C" int crd_terrain_update(const float* xyz, const uint8_t* valid, const int32_t* frame_offsets, int32_t rows_per_frame, int32_t B,
                                  int32_t n_rows, const double* map_from_points, int32_t t_stride, const double* sensor,
                                  int32_t sensor_stride, const double* centre, int32_t centre_stride, int32_t M, int32_t nx, int32_t ny,
                                  uint64_t cell_f64_bits, uint64_t z_quantum_f64_bits, uint64_t z_min_f64_bits, uint64_t z_max_f64_bits,
                                  uint64_t max_range_f64_bits, int32_t head_q, int32_t min_points, int32_t w_max, int32_t step_max_q,
                                  int64_t slope2_max, int32_t* map_ground, int32_t* map_top, int16_t* map_weight, int64_t* prev_origin,
                                  int64_t* cur_origin, int32_t* initialised, int32_t* status, void* workspace, int64_t workspace_bytes,
                                  int32_t* ground, int32_t* top, int32_t* step, int64_t* slope2, int16_t* weight, uint8_t* state,
                                  uint8_t* hazard, uint8_t* evidence, float* value, int64_t* origin, crd_stream_t stream) {
  const char* name = "crd_terrain_update";
  CRD_CHECK_ARG(B > 0 && n_rows >= 0, "%s: bad argument (B %d, n_rows %d)", name, B, n_rows);
  CRD_CHECK_ARG(M == B || M == 1, "%s: bad argument (M %d maps for B %d frames: M is B, one map per frame, or 1, one map for all)", name, M, B);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  const long long n_cells = (long long)M * nx * ny;
  CRD_CHECK_ARG(n_cells < 0x80000000ll, "%s: bad argument (M * nx * ny = %lld cells are more than the 32-bit indices hold)", name, n_cells);
  const double cell = from_bits(cell_f64_bits), max_range = from_bits(max_range_f64_bits), z_quantum = from_bits(z_quantum_f64_bits);
  const double z_min = from_bits(z_min_f64_bits), z_max = from_bits(z_max_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(max_range > 0.0 && finite_h(max_range * max_range), "%s: bad argument (max_range %g: positive, with a finite square)", name,
                max_range);
  CRD_CHECK_ARG(z_quantum > 0.0 && finite_h(z_quantum), "%s: bad argument (z_quantum %g is not a finite positive size)", name, z_quantum);
  CRD_CHECK_ARG(z_min <= z_max && finite_h(z_min) && finite_h(z_max) && fabs(z_min) / z_quantum < Q_LIMIT && fabs(z_max) / z_quantum < Q_LIMIT,
                "%s: bad argument (z_range %g .. %g: finite, ordered, |z| / z_quantum %g below 2^24)", name, z_min, z_max, z_quantum);
  CRD_CHECK_ARG(t_stride == 0 || t_stride == 12, "%s: bad argument (t_stride %d is neither 0 nor 12)", name, t_stride);
  CRD_CHECK_ARG((sensor_stride == 0 || sensor_stride == 3) && (centre_stride == 0 || centre_stride == 3),
                "%s: bad argument (sensor_stride %d, centre_stride %d: each is 0 or 3)", name, sensor_stride, centre_stride);
  CRD_CHECK_ARG((frame_offsets != nullptr) != (rows_per_frame > 0) && rows_per_frame >= 0,
                "%s: bad argument (frame_offsets %s with rows_per_frame %d: exactly one of the two says which frame owns a row)", name,
                frame_offsets ? "given" : "NULL", rows_per_frame);
  CRD_CHECK_ARG(min_points >= 1, "%s: bad argument (min_points %d)", name, min_points);
  CRD_CHECK_ARG(w_max >= 1 && w_max <= 32767, "%s: bad argument (w_max %d is not in 1 .. 32767)", name, w_max);
  CRD_CHECK_ARG(head_q >= 0 && head_q <= (1 << 30), "%s: bad argument (head_q %d is not in 0 .. 2^30)", name, head_q);
  CRD_CHECK_ARG(step_max_q >= 1 && step_max_q <= (1 << 30), "%s: bad argument (step_max_q %d is not in 1 .. 2^30)", name, step_max_q);
  CRD_CHECK_ARG(slope2_max >= 1 && slope2_max <= (1ll << 62), "%s: bad argument (slope2_max %lld is not in 1 .. 2^62)", name,
                (long long)slope2_max);
  CRD_CHECK_ARG(workspace && map_ground && map_top && map_weight && prev_origin && cur_origin && initialised && status && ground && top && step &&
                    slope2 && weight && state && hazard && evidence && value && origin,
                "%s: null pointer (workspace, map_ground, map_top, map_weight, prev_origin, cur_origin, initialised, status, ground, top, "
                "step, slope2, weight, state, hazard, evidence, value, origin)", name);
  CRD_CHECK_ARG(n_rows == 0 || xyz, "%s: null pointer (xyz)", name);
  const long long cell_bytes = up16(4 * n_cells), s_bytes = up16(24ll * B);
  const long long need = 3 * cell_bytes + s_bytes + up16(4ll * M);
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  CRD_CHECK_ARG(aligned_to(xyz, 4) && aligned_to(frame_offsets, 4) && aligned_to(initialised, 4) && aligned_to(status, 4) && aligned_to(value, 4) &&
                    aligned_to(map_ground, 4) && aligned_to(map_top, 4) && aligned_to(ground, 4) && aligned_to(top, 4) && aligned_to(step, 4) &&
                    aligned_to(map_weight, 2) && aligned_to(weight, 2) && aligned_to(map_from_points, 8) && aligned_to(sensor, 8) &&
                    aligned_to(centre, 8) && aligned_to(prev_origin, 8) && aligned_to(cur_origin, 8) && aligned_to(origin, 8) &&
                    aligned_to(slope2, 8),
                "%s: bad argument (xyz, frame_offsets, initialised, status, value, map_ground, map_top, ground, top and step must be 4-byte "
                "aligned, map_weight and weight 2-byte, map_from_points, sensor, centre, slope2 and the origins 8-byte)", name);
  Ter a;
  a.xyz = xyz; a.valid = valid; a.off = frame_offsets; a.T = map_from_points; a.sensor = sensor; a.centre = centre; a.B = B; a.n = n_rows;
  a.rows_per_frame = rows_per_frame; a.t_stride = t_stride; a.s_stride = sensor_stride; a.c_stride = centre_stride; a.M = M; a.nx = nx;
  a.ny = ny; a.head_q = head_q; a.min_points = min_points; a.w_max = w_max; a.step_max_q = step_max_q; a.slope2_max = slope2_max;
  a.cell = cell; a.max_r2 = max_range * max_range; a.z_quantum = z_quantum; a.z_min = z_min; a.z_max = z_max; a.ground = map_ground;
  a.top = map_top; a.weight = map_weight; a.prev = reinterpret_cast<long long*>(prev_origin);
  a.cur = reinterpret_cast<long long*>(cur_origin); a.initialised = initialised; a.status = status;
  char* ws = reinterpret_cast<char*>(workspace);
  a.lo = reinterpret_cast<int32_t*>(ws);
  a.hi = reinterpret_cast<int32_t*>(ws + cell_bytes);
  a.count = reinterpret_cast<int32_t*>(ws + 2 * cell_bytes);
  a.S = reinterpret_cast<double*>(ws + 3 * cell_bytes);
  a.flags = reinterpret_cast<int32_t*>(ws + 3 * cell_bytes + s_bytes);
  hipStream_t st = as_stream(stream);
  const dim3 block(TPB), cells(blocks_for(n_cells, TPB, 2048));
  hipLaunchKernelGGL(k_ter_prepare, cells, block, 0, st, a, n_cells);
  if (n_rows > 0) {
    hipLaunchKernelGGL(k_ter_points_lo, dim3(cdiv(n_rows, TPB)), block, 0, st, a);
    hipLaunchKernelGGL(k_ter_points_hi, dim3(cdiv(n_rows, TPB)), block, 0, st, a);
  }
  hipLaunchKernelGGL(k_ter_fuse, cells, block, 0, st, a, n_cells);
  hipLaunchKernelGGL(k_ter_derive, cells, block, 0, st, a, n_cells, ground, top, step, reinterpret_cast<long long*>(slope2), weight, state,
                     hazard, evidence, value, reinterpret_cast<long long*>(origin));
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
