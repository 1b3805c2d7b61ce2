// Scan matcher on the device: a point cloud (the forms occupancy_ops.hip takes), its prior pose and the occupancy map as it stands ->
// a window of turns and whole-cell shifts of the cloud's obstacle cells scored against the map's log-odds, the best one applied to the
// pose (include/camradepth_hip.h, crd_match_scan).  The map is read only.  Four launches on the caller's stream:
//   prepare  T'[b][t] for every frame and turn (match_pick.h), every frame's sensor in the map frame, the count grids, the score table
//            and n_cells cleared
//   points   one thread per row: the row's test of k_occ_points with the unturned pose, then for every turn its world cell in the
//            count grid of (map, turn), the window grown by n_xy cells on every side; neighbouring lanes that share a cell are folded
//            first (k_occ_points' fold) and the run's first lane adds its length
//   scores   one workgroup per (tile of 32 x 32 cells of a count grid, turn, map): the tile's scan cells compacted by ballot into LDS
//            -- a workgroup without one leaves here, and most do --, the map's log-odds under the tile with a halo of n_xy cells in
//            LDS as int16, every thread owns shifts and sums the log-odds under the tile's scan cells; one 64-bit atomic add per
//            shift and workgroup into the score table
//   pick     one workgroup per map: the least candidate in mp_better's order by a strided scan and a tree over LDS, the guards, the
//            poses of the map's frames
// Integer atomics only (add), whose sums do not depend on the order of arrival, and the pick is the least element of a total order: the
// same bits every run.  No workgroup waits for another; every loop's bound is an argument of the launch.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_match_scores 10248 bytes of LDS, k_match_pick 24584 (a workgroup of 16 waves), no scratch
// in any of the four.
#include "raster.h"       // frame_of, rigid, finite_d, aligned16
#include "match_pick.h"
#include <string.h>

// the results are specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int PICK_TPB = 1024;                                          // one workgroup per map scans up to 65 * 33 * 33 candidates
constexpr int TILE = 32;                                                // cells of a count grid along each side of a tile
constexpr int HALO_MAX = TILE + 2 * MP_MAX_XY;

struct Mat {
  const float* xyz;
  const unsigned char* valid;                        // may be NULL
  const int32_t* off;                                // NULL: frame b owns the rows b * rows_per_frame ..
  const double *T, *sensor, *rot;                    // T and sensor may be NULL: the identity, the origin
  int B, n, rows_per_frame, t_stride, s_stride, M, nx, ny, min_points, n_xy, n_theta, min_cells;
  int nt, ns, ex, ey;                                // turns, shifts along an axis, the sides of a count grid
  double cell, max_r2, z_lo, z_hi;
  long long min_score;
  const int16_t* map;                                // the caller's state, read only
  const long long* cur;
  const int32_t* initialised;
  double *Tc, *S;                                    // the workspace
  int32_t* counts;
  long long* table;
  double* pose;                                      // the outputs
  int32_t *pick, *n_cells, *status;
  long long *score, *prior_score, *scores;           // scores may be NULL
};

__device__ __forceinline__ void pose_of(const Mat& a, int b, double* T) {
  if (a.T) {
    for (int k = 0; k < 12; ++k) T[k] = a.T[(long long)b * a.t_stride + k];
  } else {
    for (int k = 0; k < 12; ++k) T[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
  }
}

// S_b = T_b . sensor_b
__device__ __forceinline__ void sensor_of(const Mat& a, int b, const double* T, double* S) {
  const double* v = a.sensor ? a.sensor + (long long)b * a.s_stride : nullptr;
  const double x = v ? v[0] : 0.0, y = v ? v[1] : 0.0, z = v ? v[2] : 0.0;
  rigid(T, x, y, z, S[0], S[1], S[2]);
}

// Launch 1
__global__ __launch_bounds__(TPB) void k_match_prepare(Mat a, long long n_counts, long long n_table) {
  const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
  int4* quads = reinterpret_cast<int4*>(a.counts);                     // from a 16-byte boundary of the workspace
  for (long long i = t0; i < n_counts >> 2; i += step) quads[i] = make_int4(0, 0, 0, 0);
  for (long long i = (n_counts & ~3ll) + t0; i < n_counts; i += step) a.counts[i] = 0;
  for (long long i = t0; i < n_table; i += step) a.table[i] = 0;
  for (long long m = t0; m < a.M; m += step) a.n_cells[m] = 0;
  for (long long i = t0; i < (long long)a.B * a.nt; i += step) {
    const int b = (int)(i / a.nt), t = (int)(i - (long long)b * a.nt), b0 = a.M == 1 ? 0 : b;
    double T[12], T0[12], S[3], S0[3];
    pose_of(a, b, T);
    pose_of(a, b0, T0);
    sensor_of(a, b0, T0, S0);
    mp_candidate(T, S0, a.rot[t * 2], a.rot[t * 2 + 1], t == a.n_theta, a.Tc + i * 12);
    if (t == 0) {
      sensor_of(a, b, T, S);
      a.S[b * 3] = S[0]; a.S[b * 3 + 1] = S[1]; a.S[b * 3 + 2] = S[2];
    }
  }
}

// k_occ_points' row test with the unturned pose: the frame of row p, or -1 when the row is no obstacle point of the update
__device__ __forceinline__ int hit_frame(const Mat& a, int p, double& x, double& y, double& z) {
  if (a.valid && !a.valid[p]) return -1;
  const int b = a.off ? frame_of(a.off, a.B, p) : p / a.rows_per_frame;
  if (b < 0 || b >= a.B) return -1;
  const float* s = a.xyz + (long long)p * 3;
  x = (double)s[0]; y = (double)s[1]; z = (double)s[2];
  double X, Y, Z;
  rigid(a.Tc + ((long long)b * a.nt + a.n_theta) * 12, x, y, z, X, Y, Z);                 // the centre turn holds T_b itself
  const double Sx = a.S[b * 3], Sy = a.S[b * 3 + 1], Sz = a.S[b * 3 + 2];
  if (!(finite_d(X) && finite_d(Y) && finite_d(Z) && finite_d(Sx) && finite_d(Sy) && finite_d(Sz))) return -1;
  const double dx = X - Sx, dy = Y - Sy, r2 = dx * dx + dy * dy;
  if (!(r2 > 0.0 && r2 <= a.max_r2)) return -1;
  if (!(Z >= a.z_lo && Z <= a.z_hi)) return -1;
  return b;
}

// k_occ_points' run_end
__device__ __forceinline__ int run_end(int key, int lane, bool& head) {
  const int before = __shfl_up(key, 1);
  const unsigned long long heads = __ballot(lane == 0 || before != key);
  const unsigned long long later = lane == CRD_WAVE - 1 ? 0ull : heads >> (lane + 1);
  head = (heads >> lane) & 1ull;
  return later ? lane + __ffsll(later) : CRD_WAVE;
}

// Launch 2: one thread per row, every turn.  A stretch of wall puts neighbouring rows of an image-ordered cloud into one cell, turned
// or not, so each run of equal cells among the neighbouring lanes of a wave issues one add of its length.
__global__ __launch_bounds__(TPB) void k_match_points(Mat a) {
  const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & (CRD_WAVE - 1);
  double x = 0.0, y = 0.0, z = 0.0;
  const int b = p < a.n ? hit_frame(a, (int)p, x, y, z) : -1;         // every lane stays for the wave operations
  if (__ballot(b >= 0) == 0ull) return;                                 // a wave of ground and sky: all its lanes leave together
  const int m = a.M == 1 ? 0 : b;
  long long ox = 0, oy = 0;
  if (b >= 0) {
    ox = (long long)((unsigned long long)a.cur[m * 2] - (unsigned long long)a.n_xy);
    oy = (long long)((unsigned long long)a.cur[m * 2 + 1] - (unsigned long long)a.n_xy);
  }
  const double x_lo = (double)ox, x_hi = (double)(long long)((unsigned long long)ox + (unsigned long long)a.ex);
  const double y_lo = (double)oy, y_hi = (double)(long long)((unsigned long long)oy + (unsigned long long)a.ey);
  for (int t = 0; t < a.nt; ++t) {
    int key = -1;
    if (b >= 0) {
      const double* Tc = a.Tc + ((long long)b * a.nt + t) * 12;
      const double X = Tc[0] * x + Tc[1] * y + Tc[2] * z + Tc[3], Y = Tc[4] * x + Tc[5] * y + Tc[6] * z + Tc[7];
      const double wx = floor(X / a.cell), wy = floor(Y / a.cell);
      if (wx >= x_lo && wx < x_hi && wy >= y_lo && wy < y_hi) {        // on the doubles; a NaN fails
        const long long i = (long long)wx - ox, j = (long long)wy - oy;
        if (i >= 0 && i < a.ex && j >= 0 && j < a.ey)                   // never with an origin an update wrote: the caller's may be anything
          key = (((m * a.nt + t) * a.ex) + (int)i) * a.ey + (int)j;
      }
    }
    bool head;
    const int end = run_end(key, lane, head);
    if (key >= 0 && head) __hip_atomic_fetch_add(a.counts + key, end - lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Launch 3: blockIdx = (tile, turn, map)
__global__ __launch_bounds__(TPB) void k_match_scores(Mat a, int tiles_j) {
  __shared__ int16_t L[HALO_MAX * HALO_MAX];
  __shared__ unsigned short cells[TILE * TILE];
  __shared__ int n_list, n_inside;
  const int tid = threadIdx.x, lane = tid & (CRD_WAVE - 1);
  const int ti = blockIdx.x / tiles_j, tj = blockIdx.x - ti * tiles_j, t = blockIdx.y, m = blockIdx.z;
  const int i0 = ti * TILE, j0 = tj * TILE;                             // the tile's first cell in the count grid
  if (tid == 0) { n_list = 0; n_inside = 0; }
  __syncthreads();
  const int32_t* grid = a.counts + (long long)(m * a.nt + t) * a.ex * a.ey;
  for (int q = tid; q < TILE * TILE; q += TPB) {                        // TILE * TILE is a multiple of TPB: whole waves
    const int li = q / TILE, lj = q - li * TILE, i = i0 + li, j = j0 + lj;
    const bool scan = i < a.ex && j < a.ey && grid[(long long)i * a.ey + j] >= a.min_points;
    const bool inside = scan && i >= a.n_xy && i < a.n_xy + a.nx && j >= a.n_xy && j < a.n_xy + a.ny;
    const unsigned long long word = __ballot(scan), in_word = __ballot(inside);
    int base = 0;
    if (lane == 0 && word) {
      base = atomicAdd(&n_list, __popcll(word));
      if (in_word) atomicAdd(&n_inside, __popcll(in_word));
    }
    base = __shfl(base, 0);
    if (scan) cells[base + __popcll(word & ((1ull << lane) - 1ull))] = (unsigned short)(li << 8 | lj);
  }
  __syncthreads();
  const int n = n_list;
  if (n == 0) return;                                                   // the same in every thread
  if (tid == 0 && t == a.n_theta && n_inside) __hip_atomic_fetch_add(a.n_cells + m, n_inside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // the log-odds under the tile and n_xy cells around it: count-grid cell (i, j) is window cell (i - n_xy, j - n_xy)
  const int side = TILE + 2 * a.n_xy;
  const bool live = a.initialised[m] != 0;
  const long long ox = a.cur[m * 2], oy = a.cur[m * 2 + 1];
  for (int q = tid; q < side * side; q += TPB) {
    const int li = q / side, lj = q - li * side;
    const int wi = i0 + li - 2 * a.n_xy, wj = j0 + lj - 2 * a.n_xy;     // the window cell under count-grid cell (i0 + li - n_xy, ..)
    int v = 0;
    if (live && wi >= 0 && wi < a.nx && wj >= 0 && wj < a.ny) {
      long long sx = (long long)((unsigned long long)ox + (unsigned long long)(long long)wi) % a.nx;
      long long sy = (long long)((unsigned long long)oy + (unsigned long long)(long long)wj) % a.ny;
      sx += sx < 0 ? a.nx : 0;
      sy += sy < 0 ? a.ny : 0;
      v = a.map[((long long)m * a.nx + sx) * a.ny + sy];
    }
    L[q] = (int16_t)v;
  }
  __syncthreads();
  long long* row = a.table + (long long)(m * a.nt + t) * a.ns * a.ns;
  for (int sh = tid; sh < a.ns * a.ns; sh += TPB) {
    const int ix = sh / a.ns, iy = sh - ix * a.ns;                      // dx + n_xy, dy + n_xy: the cell's place in L is (li + ix, lj + iy)
    int sum = 0;                                                        // at most 1024 cells of |log-odds| <= 32767
    for (int k = 0; k < n; ++k) {
      const int c = cells[k];
      sum += L[((c >> 8) + ix) * side + (c & 255) + iy];
    }
    if (sum) __hip_atomic_fetch_add(row + sh, (long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Launch 4: one workgroup per map
__global__ __launch_bounds__(PICK_TPB) void k_match_pick(Mat a) {
  __shared__ MpCandidate best[PICK_TPB];
  __shared__ int bad;
  const int tid = threadIdx.x, m = blockIdx.x, per = a.nt * a.ns * a.ns;
  const long long* table = a.table + (long long)m * per;
  if (tid == 0) bad = 0;
  MpCandidate mine = mp_at(table, tid < per ? tid : 0, a.n_xy);
  for (int i = tid; i < per; i += PICK_TPB) {
    const MpCandidate c = mp_at(table, i, a.n_xy);
    if (mp_better(c, mine, a.n_theta)) mine = c;
    if (a.scores) a.scores[(long long)m * per + i] = c.score;
  }
  best[tid] = mine;
  __syncthreads();
  // a pose or a sensor of a feeding frame that is not finite
  const int b0 = a.M == 1 ? 0 : m, b1 = a.M == 1 ? a.B : m + 1;
  for (int i = tid; i < (b1 - b0) * 15; i += PICK_TPB) {
    const int b = b0 + i / 15, k = i - (i / 15) * 15;
    const double v = k < 12 ? a.Tc[((long long)b * a.nt + a.n_theta) * 12 + k] : a.S[b * 3 + k - 12];
    if (!finite_d(v)) atomicOr(&bad, 1);
  }
  for (int d = PICK_TPB / 2; d > 0; d >>= 1) {
    if (tid < d && mp_better(best[tid + d], best[tid], a.n_theta)) best[tid] = best[tid + d];
    __syncthreads();
  }
  const MpCandidate win = best[0];
  const int centre = (a.n_theta * a.ns + a.n_xy) * a.ns + a.n_xy;
  const int cells = a.n_cells[m];
  int status = (a.initialised[m] == 0 ? MP_UNINITIALISED : 0) | (bad ? MP_NOT_FINITE : 0) | (cells < a.min_cells ? MP_FEW_CELLS : 0) |
               (win.score < a.min_score ? MP_LOW_SCORE : 0);
  if (!(status & MP_KEEPS_PRIOR) && mp_on_border(win, a.n_xy, a.n_theta)) status |= MP_ON_BORDER;
  if (tid == 0) {
    a.pick[m * 3] = win.t - a.n_theta; a.pick[m * 3 + 1] = win.dx; a.pick[m * 3 + 2] = win.dy;
    a.score[m] = win.score;
    a.prior_score[m] = table[centre];
    a.status[m] = status;
  }
  for (int i = tid; i < (b1 - b0) * 12; i += PICK_TPB) {
    const int b = b0 + i / 12, k = i - (i / 12) * 12;
    const double* Tb = a.Tc + (long long)b * a.nt * 12;
    a.pose[(long long)b * 12 + k] = (status & MP_KEEPS_PRIOR) ? Tb[a.n_theta * 12 + k] : mp_shifted_at(Tb + win.t * 12, k, win.dx, win.dy, a.cell);
  }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf
inline long long up16(long long n) { return (n + 15) & ~15ll; }

}  // namespace

extern "C" int crd_match_scan(const float* xyz, const uint8_t* valid, const int32_t* frame_offsets, int32_t rows_per_frame, int32_t B,
                              int32_t n_rows, const double* map_from_points, int32_t t_stride, const double* sensor, int32_t sensor_stride,
                              int32_t M, int32_t nx, int32_t ny, uint64_t cell_f64_bits, uint64_t max_range_f64_bits, uint64_t z_lo_f64_bits,
                              uint64_t z_hi_f64_bits, int32_t min_points, const int16_t* map, const int64_t* cur_origin,
                              const int32_t* initialised, int32_t n_xy, int32_t n_theta, const double* rot, int32_t min_cells,
                              int64_t min_score, void* workspace, int64_t workspace_bytes, double* pose, int32_t* pick, int64_t* score,
                              int64_t* prior_score, int32_t* n_cells, int32_t* status, int64_t* scores, crd_stream_t stream) {
  const char* name = "crd_match_scan";
  CRD_CHECK_ARG(B > 0 && B <= 65535 && n_rows >= 0, "%s: bad argument (B %d, n_rows %d; B is 1 .. 65535)", name, B, n_rows);
  CRD_CHECK_ARG(M == B || M == 1, "%s: bad argument (M %d maps for B %d frames: M is B, one map per frame, or 1, one map for all)", name, M, B);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  CRD_CHECK_ARG((long long)M * nx * ny < 0x80000000ll, "%s: bad argument (M * nx * ny = %lld cells are more than the 32-bit indices hold)", name,
                (long long)M * nx * ny);
  CRD_CHECK_ARG(n_xy >= 0 && n_xy <= MP_MAX_XY, "%s: bad argument (n_xy %d; 0 .. 16)", name, n_xy);
  CRD_CHECK_ARG(n_theta >= 0 && n_theta <= MP_MAX_THETA, "%s: bad argument (n_theta %d; 0 .. 32)", name, n_theta);
  const int nt = 2 * n_theta + 1, ns = 2 * n_xy + 1, ex = nx + 2 * n_xy, ey = ny + 2 * n_xy;
  const long long n_counts = (long long)M * nt * ex * ey, n_table = (long long)M * nt * ns * ns;
  CRD_CHECK_ARG(n_counts < 0x80000000ll, "%s: bad argument (M * (2 n_theta + 1) * (nx + 2 n_xy) * (ny + 2 n_xy) = %lld counts are more than "
                "the 32-bit indices hold)", name, n_counts);
  const double cell = from_bits(cell_f64_bits), max_range = from_bits(max_range_f64_bits), z_lo = from_bits(z_lo_f64_bits);
  const double z_hi = from_bits(z_hi_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(max_range > 0.0 && finite_h(max_range * max_range), "%s: bad argument (max_range %g: positive, with a finite square)", name,
                max_range);
  CRD_CHECK_ARG(z_lo <= z_hi, "%s: bad argument (z_lo %g, z_hi %g: no NaN, z_lo <= z_hi)", name, z_lo, z_hi);
  CRD_CHECK_ARG(t_stride == 0 || t_stride == 12, "%s: bad argument (t_stride %d is neither 0 nor 12)", name, t_stride);
  CRD_CHECK_ARG(sensor_stride == 0 || sensor_stride == 3, "%s: bad argument (sensor_stride %d is neither 0 nor 3)", name, sensor_stride);
  CRD_CHECK_ARG((frame_offsets != nullptr) != (rows_per_frame > 0) && rows_per_frame >= 0,
                "%s: bad argument (frame_offsets %s with rows_per_frame %d: exactly one of the two says which frame owns a row)", name,
                frame_offsets ? "given" : "NULL", rows_per_frame);
  CRD_CHECK_ARG(min_points >= 1, "%s: bad argument (min_points %d)", name, min_points);
  CRD_CHECK_ARG(min_cells >= 0, "%s: bad argument (min_cells %d)", name, min_cells);
  CRD_CHECK_ARG(workspace && map && cur_origin && initialised && rot && pose && pick && score && prior_score && n_cells && status,
                "%s: null pointer (workspace, map, cur_origin, initialised, rot, pose, pick, score, prior_score, n_cells, status)", name);
  CRD_CHECK_ARG(n_rows == 0 || xyz, "%s: null pointer (xyz)", name);
  const long long tc_bytes = up16(96ll * B * nt), s_bytes = up16(24ll * B), count_bytes = up16(4 * n_counts), table_bytes = up16(8 * n_table);
  const long long need = tc_bytes + s_bytes + count_bytes + table_bytes;
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  CRD_CHECK_ARG(aligned_to(xyz, 4) && aligned_to(frame_offsets, 4) && aligned_to(initialised, 4) && aligned_to(pick, 4) && aligned_to(n_cells, 4) &&
                    aligned_to(status, 4) && aligned_to(map, 2) && aligned_to(map_from_points, 8) && aligned_to(sensor, 8) &&
                    aligned_to(cur_origin, 8) && aligned_to(rot, 8) && aligned_to(pose, 8) && aligned_to(score, 8) &&
                    aligned_to(prior_score, 8) && aligned_to(scores, 8),
                "%s: bad argument (xyz, frame_offsets, initialised, pick, n_cells and status must be 4-byte aligned, map 2-byte, "
                "map_from_points, sensor, cur_origin, rot, pose, score, prior_score and scores 8-byte)", name);
  Mat a;
  a.xyz = xyz; a.valid = valid; a.off = frame_offsets; a.T = map_from_points; a.sensor = sensor; a.rot = rot; a.B = B; a.n = n_rows;
  a.rows_per_frame = rows_per_frame; a.t_stride = t_stride; a.s_stride = sensor_stride; a.M = M; a.nx = nx; a.ny = ny;
  a.min_points = min_points; a.n_xy = n_xy; a.n_theta = n_theta; a.min_cells = min_cells; a.nt = nt; a.ns = ns; a.ex = ex; a.ey = ey;
  a.cell = cell; a.max_r2 = max_range * max_range; a.z_lo = z_lo; a.z_hi = z_hi; a.min_score = min_score; a.map = map;
  a.cur = reinterpret_cast<const long long*>(cur_origin); a.initialised = initialised;
  char* ws = reinterpret_cast<char*>(workspace);
  a.Tc = reinterpret_cast<double*>(ws);
  a.S = reinterpret_cast<double*>(ws + tc_bytes);
  a.counts = reinterpret_cast<int32_t*>(ws + tc_bytes + s_bytes);
  a.table = reinterpret_cast<long long*>(ws + tc_bytes + s_bytes + count_bytes);
  a.pose = pose; a.pick = pick; a.n_cells = n_cells; a.status = status; a.score = reinterpret_cast<long long*>(score);
  a.prior_score = reinterpret_cast<long long*>(prior_score); a.scores = reinterpret_cast<long long*>(scores);
  hipStream_t st = as_stream(stream);
  const dim3 block(TPB);
  const int tiles_i = cdiv(ex, TILE), tiles_j = cdiv(ey, TILE);
  hipLaunchKernelGGL(k_match_prepare, dim3(blocks_for(n_counts, TPB, 4096)), block, 0, st, a, n_counts, n_table);
  if (n_rows > 0) hipLaunchKernelGGL(k_match_points, dim3(cdiv(n_rows, TPB)), block, 0, st, a);
  hipLaunchKernelGGL(k_match_scores, dim3(tiles_i * tiles_j, nt, M), block, 0, st, a, tiles_j);
  hipLaunchKernelGGL(k_match_pick, dim3(M), dim3(PICK_TPB), 0, st, a);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
