// Occupancy map on the device: a point cloud (the forms bev_ops.hip takes) -> free / occupied / unknown per cell of a world-aligned
// rolling window, fused over frames into an int16 log-odds image that is stored as a torus, so the window moves by whole cells and
// nothing is copied.  Free space comes from bearing bins around the sensor: per bin the nearest hit and the farthest thing seen, both
// as order-independent 64-bit integer atomics on the bits of a squared range.  Three launches on the caller's stream (prepare, points,
// cells); no workgroup waits for another.  All arithmetic is fp64 add, multiply, divide, floor and compare.
#include "raster.h"       // frame_of, rigid, finite_d, aligned16
#include <string.h>

// the results are specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr unsigned long long INF_BITS = 0x7ff0000000000000ull;
constexpr double ORIGIN_LIMIT = 2147418112.0;        // 2^31 - 65536: a window of up to 65535 cells around it stays inside int32
constexpr int SKIPPED = 2, WAS_INITIALISED = 1;      // flags[m] of one call

struct Occ {
  const float* xyz;
  const unsigned char* valid;                        // may be NULL
  const int32_t* off;                                // NULL: frame b owns the rows b * rows_per_frame ..
  const double *T, *sensor, *centre;                 // each may be NULL: the identity, the origin, the sensor
  int B, n, rows_per_frame, t_stride, s_stride, c_stride, M, nx, ny, n_bins, min_points, l_occ, l_free, l_max, occupied_at, free_at;
  double cell, max_r2, z_floor, z_lo, z_hi;
  int16_t* map;                                      // the caller's state
  long long *prev, *cur;
  int32_t *initialised, *status;
  unsigned long long *hit_min, *seen_max;            // the workspace
  double* S;
  int32_t *hits, *flags;
};

// T_b . v for a point v of the points' frame (NULL: the origin)
__device__ __forceinline__ void to_map(const Occ& a, int b, const double* v, double& X, double& Y, double& Z) {
  const double x = v ? v[0] : 0.0, y = v ? v[1] : 0.0, z = v ? v[2] : 0.0;
  X = x; Y = y; Z = z;
  if (a.T) rigid(a.T + (long long)b * a.t_stride, x, y, z, X, Y, Z);
}

// The bearing bin of a direction with finite components, not both zero: four faces of a square, qb bins along each
__device__ __forceinline__ int bin_of(double dx, double dy, int qb) {
  const double ax = fabs(dx), ay = fabs(dy);
  int face;
  double s;
  if (ax >= ay) { face = dx > 0.0 ? 0 : 2; s = dy / ax; } else { face = dy > 0.0 ? 1 : 3; s = dx / ay; }
  const double q = fmin(floor(((s + 1.0) * 0.5) * (double)qb), (double)(qb - 1));
  return face * qb + (int)q;
}

// Launch 1: the bins and the hit counts cleared, every frame's sensor in the map frame, every map's window moved.
__global__ __launch_bounds__(TPB) void k_occ_prepare(Occ a, long long n_keys, long long n_cells) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
  for (long long i = t; i < n_keys; i += step) {
    a.hit_min[i] = INF_BITS;
    a.seen_max[i] = 0ull;
  }
  for (long long i = t; i < n_cells; i += step) a.hits[i] = 0;
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

// What row p brings: its bin k (flat over the frames) with the bits of its squared range as a candidate for seen_max (0: none) and
// for hit_min (all ones: none), and the flat index c of the window cell it hits; k < 0: nothing, c < 0: no cell.
struct Row { long long k; unsigned long long seen, hit; int c; };

__device__ __forceinline__ Row row_of(const Occ& a, int p) {
  Row r = {-1, 0ull, ~0ull, -1};
  if (a.valid && !a.valid[p]) return r;
  const int b = a.off ? frame_of(a.off, a.B, p) : p / a.rows_per_frame;
  if (b < 0 || b >= a.B) return r;
  const float* s = a.xyz + (long long)p * 3;
  double X = (double)s[0], Y = (double)s[1], Z = (double)s[2];
  if (a.T) rigid(a.T + (long long)b * a.t_stride, (double)s[0], (double)s[1], (double)s[2], X, Y, Z);
  const double Sx = a.S[b * 3], Sy = a.S[b * 3 + 1], Sz = a.S[b * 3 + 2];
  if (!(finite_d(X) && finite_d(Y) && finite_d(Z) && finite_d(Sx) && finite_d(Sy) && finite_d(Sz))) return r;
  const double dx = X - Sx, dy = Y - Sy, r2 = dx * dx + dy * dy;
  if (!(r2 > 0.0 && r2 <= a.max_r2)) return r;                        // dx and dy are finite from here on
  const bool seen = Z >= a.z_floor && Z <= a.z_hi, hit = Z >= a.z_lo && Z <= a.z_hi;
  if (!seen && !hit) return r;
  r.k = (long long)b * a.n_bins + bin_of(dx, dy, a.n_bins >> 2);
  const unsigned long long mine = (unsigned long long)__double_as_longlong(r2);
  if (seen) r.seen = mine;
  if (!hit) return r;
  r.hit = mine;
  const int m = a.M == 1 ? 0 : b;
  const long long ox = a.cur[m * 2], oy = a.cur[m * 2 + 1];
  const double wx = floor(X / a.cell), wy = floor(Y / a.cell);
  if (!(wx >= (double)ox && wx < (double)(ox + a.nx) && wy >= (double)oy && wy < (double)(oy + a.ny))) return r;   // on the doubles
  const long long i = (long long)wx - ox, j = (long long)wy - oy;
  if (i < 0 || i >= a.nx || j < 0 || j >= a.ny) return r;            // never with an origin launch 1 wrote: the caller's may be anything
  r.c = (m * a.nx + (int)i) * a.ny + (int)j;
  return r;
}

// The end of the run of equal keys among neighbouring lanes that this lane belongs to, and whether the lane is its head
__device__ __forceinline__ int run_end(long long key, int lane, bool& head) {
  const long long before = __shfl_up(key, 1);
  const unsigned long long heads = __ballot(lane == 0 || before != key);
  const unsigned long long later = lane == CRD_WAVE - 1 ? 0ull : heads >> (lane + 1);
  head = (heads >> lane) & 1ull;
  return later ? lane + __ffsll(later) : CRD_WAVE;
}

// Launch 2: one thread per row.  A cloud in image order puts runs of neighbouring rows into one bearing bin (a few pixels of an image
// row) and into one cell (a stretch of wall), and a hot address serialises its atomics, so each run of equal bins and each run of
// equal cells among the neighbouring lanes of a wave is folded first -- the keys by a segmented maximum and minimum, the hits as the
// run's length -- and its first lane alone goes to memory (k_bev_keys's fold): integer maximum, minimum and sum, the same in any
// grouping.  seen_max only rises and hit_min only falls, so a plain read that already shows a key at or beyond the run's settles it
// without an atomic (k_bev_keys's way out).
__global__ __launch_bounds__(TPB) void k_occ_points(Occ a) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & (CRD_WAVE - 1);
  Row r = {-1, 0ull, ~0ull, -1};
  if (t < a.n) r = row_of(a, (int)t);                                 // every lane stays for the wave operations
  bool head;
  int end = run_end(r.k, lane, head);
#pragma unroll
  for (int d = 1; d < CRD_WAVE; d <<= 1) {                            // afterwards seen and hit of a head cover its whole run
    const unsigned long long os = __shfl_down(r.seen, d), oh = __shfl_down(r.hit, d);
    if (lane + d < end) {
      r.seen = os > r.seen ? os : r.seen;
      r.hit = oh < r.hit ? oh : r.hit;
    }
  }
  if (r.k >= 0 && head) {
    if (r.seen != 0ull && __hip_atomic_load(a.seen_max + r.k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < r.seen)
      __hip_atomic_fetch_max(a.seen_max + r.k, r.seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r.hit != ~0ull && __hip_atomic_load(a.hit_min + r.k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > r.hit)
      __hip_atomic_fetch_min(a.hit_min + r.k, r.hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  end = run_end(r.c, lane, head);
  if (r.c >= 0 && head) __hip_atomic_fetch_add(a.hits + r.c, end - lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Launch 3: one window cell per thread -- its evidence, the slot of the torus updated in place, the outputs in window order.
__global__ __launch_bounds__(TPB) void k_occ_cells(Occ a, long long n_cells, int16_t* log_odds, unsigned char* state, unsigned char* evidence,
                                                   float* value, long long* origin) {
  const long long per = (long long)a.nx * a.ny;
  for (long long idx = (long long)blockIdx.x * TPB + threadIdx.x; idx < n_cells; idx += (long long)gridDim.x * TPB) {
    const int m = (int)(idx / per), rem = (int)(idx - m * per), i = rem / a.ny, j = rem - i * a.ny;
    const int flags = a.flags[m];
    const bool skipped = (flags & SKIPPED) != 0, live = (flags & WAS_INITIALISED) != 0;
    const long long ox = a.cur[m * 2], oy = a.cur[m * 2 + 1], wx = ox + i, wy = oy + j;
    long long sx = wx % a.nx, sy = wy % a.ny;
    sx += sx < 0 ? a.nx : 0;
    sy += sy < 0 ? a.ny : 0;
    int16_t* slot = a.map + ((long long)m * a.nx + sx) * a.ny + sy;
    const long long px = a.prev[m * 2], py = a.prev[m * 2 + 1];
    const bool kept = skipped || (wx >= px && wx < px + a.nx && wy >= py && wy < py + a.ny);
    const int old = live && kept ? (int)*slot : 0;
    int ev = 0;
    if (!skipped) {
      if (a.hits[idx] >= a.min_points) {
        ev = 2;
      } else {
        const double cx = ((double)wx + 0.5) * a.cell, cy = ((double)wy + 0.5) * a.cell;
        const int b0 = a.M == 1 ? 0 : m, b1 = a.M == 1 ? a.B : m + 1;
        for (int b = b0; b < b1 && !ev; ++b) {
          const double dx = cx - a.S[b * 3], dy = cy - a.S[b * 3 + 1], r2c = dx * dx + dy * dy;
          if (!(r2c > 0.0 && r2c <= a.max_r2)) continue;              // beyond anything seen; dx and dy are finite from here on
          const long long k = (long long)b * a.n_bins + bin_of(dx, dy, a.n_bins >> 2);
          if (r2c < __longlong_as_double((long long)a.hit_min[k]) && r2c <= __longlong_as_double((long long)a.seen_max[k])) ev = 1;
        }
      }
    }
    int now = old + (ev == 2 ? a.l_occ : ev == 1 ? -a.l_free : 0);
    now = now < -a.l_max ? -a.l_max : (now > a.l_max ? a.l_max : now);
    if (skipped) now = old;
    if (!skipped) *slot = (int16_t)now;
    log_odds[idx] = (int16_t)now;
    state[idx] = (unsigned char)(now >= a.occupied_at ? 2 : (now <= -a.free_at ? 1 : 0));
    evidence[idx] = (unsigned char)ev;
    if (value) value[idx] = (float)now;
    if (rem == 0) {
      origin[m * 2] = ox;
      origin[m * 2 + 1] = oy;
      if (!skipped) a.initialised[m] = 1;
    }
  }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf
inline long long up16(long long n) { return (n + 15) & ~15ll; }

}  // namespace

extern "C" int crd_occupancy_update(const float* xyz, const uint8_t* valid, const int32_t* frame_offsets, int32_t rows_per_frame, int32_t B,
                                    int32_t n_rows, const double* map_from_points, int32_t t_stride, const double* sensor,
                                    int32_t sensor_stride, const double* centre, int32_t centre_stride, int32_t M, int32_t nx, int32_t ny,
                                    uint64_t cell_f64_bits, int32_t n_bins, uint64_t max_range_f64_bits, uint64_t z_floor_f64_bits,
                                    uint64_t z_lo_f64_bits, uint64_t z_hi_f64_bits, int32_t min_points, int32_t l_occ, int32_t l_free,
                                    int32_t l_max, int32_t occupied_at, int32_t free_at, int16_t* map, int64_t* prev_origin,
                                    int64_t* cur_origin, int32_t* initialised, int32_t* status, void* workspace, int64_t workspace_bytes,
                                    int16_t* log_odds, uint8_t* state, uint8_t* evidence, float* value, int64_t* origin,
                                    crd_stream_t stream) {
  const char* name = "crd_occupancy_update";
  CRD_CHECK_ARG(B > 0 && n_rows >= 0, "%s: bad argument (B %d, n_rows %d)", name, B, n_rows);
  CRD_CHECK_ARG(M == B || M == 1, "%s: bad argument (M %d maps for B %d frames: M is B, one map per frame, or 1, one map for all)", name, M, B);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  const long long n_cells = (long long)M * nx * ny;
  CRD_CHECK_ARG(n_cells < 0x80000000ll, "%s: bad argument (M * nx * ny = %lld cells are more than the 32-bit indices hold)", name, n_cells);
  CRD_CHECK_ARG(n_bins >= 4 && n_bins <= 65536 && n_bins % 4 == 0, "%s: bad argument (n_bins %d is not a multiple of 4 in 4 .. 65536)", name,
                n_bins);
  const double cell = from_bits(cell_f64_bits), max_range = from_bits(max_range_f64_bits), z_floor = from_bits(z_floor_f64_bits);
  const double z_lo = from_bits(z_lo_f64_bits), z_hi = from_bits(z_hi_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(max_range > 0.0 && finite_h(max_range * max_range), "%s: bad argument (max_range %g: positive, with a finite square)", name,
                max_range);
  CRD_CHECK_ARG(z_floor <= z_lo && z_lo <= z_hi, "%s: bad argument (z_floor %g, z_lo %g, z_hi %g: no NaN, z_floor <= z_lo <= z_hi)", name,
                z_floor, z_lo, z_hi);
  CRD_CHECK_ARG(t_stride == 0 || t_stride == 12, "%s: bad argument (t_stride %d is neither 0 nor 12)", name, t_stride);
  CRD_CHECK_ARG((sensor_stride == 0 || sensor_stride == 3) && (centre_stride == 0 || centre_stride == 3),
                "%s: bad argument (sensor_stride %d, centre_stride %d: each is 0 or 3)", name, sensor_stride, centre_stride);
  CRD_CHECK_ARG((frame_offsets != nullptr) != (rows_per_frame > 0) && rows_per_frame >= 0,
                "%s: bad argument (frame_offsets %s with rows_per_frame %d: exactly one of the two says which frame owns a row)", name,
                frame_offsets ? "given" : "NULL", rows_per_frame);
  CRD_CHECK_ARG(min_points >= 1, "%s: bad argument (min_points %d)", name, min_points);
  CRD_CHECK_ARG(l_occ >= 1 && l_free >= 1 && l_occ <= l_max && l_free <= l_max && l_max <= 32767,
                "%s: bad argument (l_occ %d, l_free %d, l_max %d: 1 <= l_occ, l_free <= l_max <= 32767)", name, l_occ, l_free, l_max);
  CRD_CHECK_ARG(occupied_at >= 1 && occupied_at <= l_max && free_at >= 1 && free_at <= l_max,
                "%s: bad argument (occupied_at %d, free_at %d: each is 1 .. l_max %d)", name, occupied_at, free_at, l_max);
  CRD_CHECK_ARG(workspace && map && prev_origin && cur_origin && initialised && status && log_odds && state && evidence && origin,
                "%s: null pointer (workspace, map, prev_origin, cur_origin, initialised, status, log_odds, state, evidence, origin)", name);
  CRD_CHECK_ARG(n_rows == 0 || xyz, "%s: null pointer (xyz)", name);
  const long long key_bytes = up16(8ll * B * n_bins), s_bytes = up16(24ll * B), hit_bytes = up16(4 * n_cells);
  const long long need = 2 * key_bytes + s_bytes + hit_bytes + up16(4ll * M);
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  CRD_CHECK_ARG(aligned_to(xyz, 4) && aligned_to(frame_offsets, 4) && aligned_to(initialised, 4) && aligned_to(status, 4) && aligned_to(value, 4) &&
                    aligned_to(map, 2) && aligned_to(log_odds, 2) && aligned_to(map_from_points, 8) && aligned_to(sensor, 8) &&
                    aligned_to(centre, 8) && aligned_to(prev_origin, 8) && aligned_to(cur_origin, 8) && aligned_to(origin, 8),
                "%s: bad argument (xyz, frame_offsets, initialised, status and value must be 4-byte aligned, map and log_odds 2-byte, "
                "map_from_points, sensor, centre and the origins 8-byte)", name);
  Occ a;
  a.xyz = xyz; a.valid = valid; a.off = frame_offsets; a.T = map_from_points; a.sensor = sensor; a.centre = centre; a.B = B; a.n = n_rows;
  a.rows_per_frame = rows_per_frame; a.t_stride = t_stride; a.s_stride = sensor_stride; a.c_stride = centre_stride; a.M = M; a.nx = nx;
  a.ny = ny; a.n_bins = n_bins; a.min_points = min_points; a.l_occ = l_occ; a.l_free = l_free; a.l_max = l_max; a.occupied_at = occupied_at;
  a.free_at = free_at; a.cell = cell; a.max_r2 = max_range * max_range; a.z_floor = z_floor; a.z_lo = z_lo; a.z_hi = z_hi; a.map = map;
  a.prev = reinterpret_cast<long long*>(prev_origin); a.cur = reinterpret_cast<long long*>(cur_origin); a.initialised = initialised;
  a.status = status;
  char* ws = reinterpret_cast<char*>(workspace);
  a.hit_min = reinterpret_cast<unsigned long long*>(ws);
  a.seen_max = reinterpret_cast<unsigned long long*>(ws + key_bytes);
  a.S = reinterpret_cast<double*>(ws + 2 * key_bytes);
  a.hits = reinterpret_cast<int32_t*>(ws + 2 * key_bytes + s_bytes);
  a.flags = reinterpret_cast<int32_t*>(ws + 2 * key_bytes + s_bytes + hit_bytes);
  hipStream_t st = as_stream(stream);
  const long long n_keys = (long long)B * n_bins;
  const dim3 block(TPB);
  hipLaunchKernelGGL(k_occ_prepare, dim3(blocks_for(n_keys > n_cells ? n_keys : n_cells, TPB, 2048)), block, 0, st, a, n_keys, n_cells);
  if (n_rows > 0) hipLaunchKernelGGL(k_occ_points, dim3(cdiv(n_rows, TPB)), block, 0, st, a);
  hipLaunchKernelGGL(k_occ_cells, dim3(blocks_for(n_cells, TPB, 2048)), block, 0, st, a, n_cells, log_odds, state, evidence, value,
                     reinterpret_cast<long long*>(origin));
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
