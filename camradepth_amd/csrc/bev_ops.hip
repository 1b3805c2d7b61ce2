// Bird's-eye-view back end on the device: a point cloud (cloud_ops.hip's compact xyz with frame_offsets, or its organised points with
// valid) -> per-cell grids [B][nx][ny] in the caller's frame: count, highest and lowest point, the row of the highest point, its label,
// occupancy.  The scatter is raster.h's: order-independent 64-bit integer atomics on monotone keys, then the lowest row index among the
// rows that hold the winning key -- here the LARGEST height wins, and a count is added.  Four launches on the caller's stream (clear,
// keys and count, winner, resolve); no workgroup waits for another.  All arithmetic is fp64; a height is rounded to fp32 once.
#include "raster.h"       // frame_of, rigid, finite_d, aligned16, NO_POINT
#include <string.h>

// the results are specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr unsigned EMPTY_F32 = 0x7fc00000u;          // z_max / z_min of a cell without a point: the quiet NaN viz.colorize draws as "bad"

struct Bev {
  const float* xyz;
  const unsigned char *valid, *label;                // each may be NULL
  const int32_t* off;                                // NULL: frame b owns the rows b * rows_per_frame ..
  const double* T;                                   // NULL: the identity
  int B, n, rows_per_frame, t_stride, nx, ny, flip_x, flip_y, min_points;
  double x_min, y_min, cell, z_lo, z_hi;
};

// The monotone key of a height (never NaN, never -0.0): unsigned order of the keys = order of the heights.  No height has key 0 or ~0.
__device__ __forceinline__ unsigned long long key_of(double Z) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(Z);
  return (u >> 63) ? ~u : (u ^ 0x8000000000000000ull);
}
__device__ __forceinline__ double height_of(unsigned long long key) {
  return __longlong_as_double((long long)((key >> 63) ? (key ^ 0x8000000000000000ull) : ~key));
}

// The flat index of row p's cell in the [B][nx][ny] grids and its height Z, or -1: the row is masked out, belongs to no frame, has a
// non-finite coordinate, or lies outside the height band or the grid.
__device__ __forceinline__ int cell_of(const Bev& a, int p, double& Z) {
  if (a.valid && !a.valid[p]) return -1;
  const int b = a.off ? frame_of(a.off, a.B, p) : p / a.rows_per_frame;
  if (b < 0 || b >= a.B) return -1;
  const float* s = a.xyz + (long long)p * 3;
  double X = (double)s[0], Y = (double)s[1];
  Z = (double)s[2];
  if (a.T) rigid(a.T + (long long)b * a.t_stride, (double)s[0], (double)s[1], (double)s[2], X, Y, Z);
  if (!(finite_d(X) && finite_d(Y) && finite_d(Z))) return -1;
  Z = Z + 0.0;                                       // -0.0 -> +0.0: one key per height
  if (!(Z >= a.z_lo && Z <= a.z_hi)) return -1;
  const double qx = floor((X - a.x_min) / a.cell), qy = floor((Y - a.y_min) / a.cell);
  if (!(qx >= 0.0 && qx < (double)a.nx && qy >= 0.0 && qy < (double)a.ny)) return -1;      // on the double: inf and 2^40 cells away fail here
  const int ix = a.flip_x ? a.nx - 1 - (int)qx : (int)qx, iy = a.flip_y ? a.ny - 1 - (int)qy : (int)qy;
  return (b * a.nx + ix) * a.ny + iy;
}

// Pass 0: no point in any cell -- below every height (key_max), above every height (key_min), no winner, nothing counted.
__global__ __launch_bounds__(TPB) void k_bev_clear(int n_cells, unsigned long long* key_max, unsigned long long* key_min, unsigned* winner,
                                                   int32_t* count) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n_cells; i += (long long)gridDim.x * TPB) {
    key_max[i] = 0ull;
    key_min[i] = ~0ull;
    winner[i] = NO_POINT;
    count[i] = 0;
  }
}

// Pass 1: the largest and the smallest key of every cell and the number of its rows.  A cloud in image order puts runs of neighbouring
// rows into one cell (a stretch of road, a wall), and a hot cell serialises its atomics, so each run of equal cells among the
// neighbouring lanes of a wave is folded first -- the keys by a segmented maximum and minimum, the count as the run's length -- and its
// first lane alone goes to memory: integer maximum, minimum and sum, the same result in any grouping.  key_max only rises and key_min
// only falls, so a plain read that already shows a key at or beyond the run's settles it without an atomic (k_zbuf_min_depth's way out).
__global__ __launch_bounds__(TPB) void k_bev_keys(Bev a, unsigned long long* key_max, unsigned long long* key_min, int32_t* count) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & (CRD_WAVE - 1);
  double Z = 0.0;
  const int c = t < a.n ? cell_of(a, (int)t, Z) : -1;            // every lane stays for the wave operations; -1 makes runs of its own
  const int before = __shfl_up(c, 1);
  const unsigned long long heads = __ballot(lane == 0 || before != c);
  const unsigned long long later = lane == CRD_WAVE - 1 ? 0ull : heads >> (lane + 1);
  const int end = later ? lane + __ffsll(later) : CRD_WAVE;      // this lane's run is the lanes [its head, end)
  unsigned long long hi = key_of(Z), lo = hi;
#pragma unroll
  for (int d = 1; d < CRD_WAVE; d <<= 1) {                       // afterwards hi and lo of a head cover its whole run
    const unsigned long long oh = __shfl_down(hi, d), ol = __shfl_down(lo, d);
    if (lane + d < end) {
      hi = oh > hi ? oh : hi;
      lo = ol < lo ? ol : lo;
    }
  }
  if (c < 0 || !((heads >> lane) & 1ull)) return;
  if (__hip_atomic_load(key_max + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < hi)
    __hip_atomic_fetch_max(key_max + c, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (key_min && __hip_atomic_load(key_min + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > lo)
    __hip_atomic_fetch_min(key_min + c, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(count + c, end - lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 2: among the rows at the cell's largest height the lowest row index wins.
__global__ __launch_bounds__(TPB) void k_bev_winner(Bev a, const unsigned long long* key_max, unsigned* winner) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  if (t >= a.n) return;
  const int p = (int)t;
  double Z;
  const int c = cell_of(a, p, Z);
  if (c < 0) return;
  if (key_max[c] != key_of(Z)) return;
  if (__hip_atomic_load(winner + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)p) return;
  __hip_atomic_fetch_min(winner + c, (unsigned)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 3: the keys of every cell into the outputs.  Each optional output may be NULL.
__global__ __launch_bounds__(TPB) void k_bev_resolve(Bev a, int n_cells, const unsigned long long* key_max, const unsigned long long* key_min,
                                                     const unsigned* winner, const int32_t* count, float* z_max, float* z_min,
                                                     int32_t* top_index, unsigned char* top_label, unsigned char* occupancy) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n_cells; i += (long long)gridDim.x * TPB) {
    const int n = count[i];
    const bool any = n > 0;
    const unsigned w = winner[i];
    z_max[i] = any ? (float)height_of(key_max[i]) : __uint_as_float(EMPTY_F32);
    if (z_min) z_min[i] = any ? (float)height_of(key_min[i]) : __uint_as_float(EMPTY_F32);
    if (top_index) top_index[i] = any ? (int32_t)w : -1;
    if (top_label) top_label[i] = (any && w < (unsigned)a.n) ? a.label[w] : (unsigned char)255;
    if (occupancy) occupancy[i] = (unsigned char)(n >= a.min_points);
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf

}  // namespace

extern "C" int crd_bev_grid(const float* xyz, const uint8_t* valid, const uint8_t* label, const int32_t* frame_offsets, int32_t rows_per_frame,
                            int32_t B, int32_t n_rows, const double* grid_from_points, int32_t t_stride, uint64_t x_min_f64_bits,
                            uint64_t y_min_f64_bits, uint64_t cell_f64_bits, int32_t nx, int32_t ny, uint64_t z_lo_f64_bits,
                            uint64_t z_hi_f64_bits, int32_t min_points, int32_t flip_x, int32_t flip_y, void* workspace,
                            int64_t workspace_bytes, int32_t* count, float* z_max, float* z_min, int32_t* top_index, uint8_t* top_label,
                            uint8_t* occupancy, crd_stream_t stream) {
  const char* name = "crd_bev_grid";
  CRD_CHECK_ARG(B > 0 && n_rows >= 0, "%s: bad argument (B %d, n_rows %d)", name, B, n_rows);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a grid of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  const long long n_cells = (long long)B * nx * ny;
  CRD_CHECK_ARG(n_cells < 0x80000000ll, "%s: bad argument (B * nx * ny = %lld cells are more than the 32-bit indices hold)", name, n_cells);
  const double x_min = from_bits(x_min_f64_bits), y_min = from_bits(y_min_f64_bits), cell = from_bits(cell_f64_bits);
  const double z_lo = from_bits(z_lo_f64_bits), z_hi = from_bits(z_hi_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(finite_h(x_min) && finite_h(y_min), "%s: bad argument (x_min %g, y_min %g)", name, x_min, y_min);
  CRD_CHECK_ARG(z_lo == z_lo && z_hi == z_hi && z_lo <= z_hi, "%s: bad argument (z_lo %g, z_hi %g: no NaN, z_lo <= z_hi)", name, z_lo, z_hi);
  CRD_CHECK_ARG(t_stride == 0 || t_stride == 12, "%s: bad argument (t_stride %d is neither 0 nor 12)", name, t_stride);
  CRD_CHECK_ARG((frame_offsets != nullptr) != (rows_per_frame > 0) && rows_per_frame >= 0,
                "%s: bad argument (frame_offsets %s with rows_per_frame %d: exactly one of the two says which frame owns a row)", name,
                frame_offsets ? "given" : "NULL", rows_per_frame);
  CRD_CHECK_ARG(min_points >= 1, "%s: bad argument (min_points %d)", name, min_points);
  CRD_CHECK_ARG(!top_label || label, "%s: bad argument (top_label without label)", name);
  CRD_CHECK_ARG(workspace && count && z_max, "%s: null pointer (workspace, count, z_max)", name);
  CRD_CHECK_ARG(n_rows == 0 || xyz, "%s: null pointer (xyz)", name);
  const long long key_bytes = (8 * n_cells + 15) & ~15ll, need = 2 * key_bytes + ((4 * n_cells + 15) & ~15ll);
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  CRD_CHECK_ARG(aligned4(xyz) && aligned4(frame_offsets) && aligned4(count) && aligned4(z_max) && aligned4(z_min) && aligned4(top_index) &&
                    (reinterpret_cast<uintptr_t>(grid_from_points) & 7) == 0,
                "%s: bad argument (xyz, frame_offsets, count, z_max, z_min and top_index must be 4-byte aligned, grid_from_points 8-byte)", name);
  Bev a;
  a.xyz = xyz; a.valid = valid; a.label = label; a.off = frame_offsets; a.T = grid_from_points; a.B = B; a.n = n_rows;
  a.rows_per_frame = rows_per_frame; a.t_stride = t_stride; a.nx = nx; a.ny = ny; a.flip_x = flip_x != 0; a.flip_y = flip_y != 0;
  a.min_points = min_points; a.x_min = x_min; a.y_min = y_min; a.cell = cell; a.z_lo = z_lo; a.z_hi = z_hi;
  char* ws = reinterpret_cast<char*>(workspace);
  unsigned long long* key_max = reinterpret_cast<unsigned long long*>(ws);
  unsigned long long* key_min = reinterpret_cast<unsigned long long*>(ws + key_bytes);
  unsigned* winner = reinterpret_cast<unsigned*>(ws + 2 * key_bytes);
  hipStream_t st = as_stream(stream);
  const dim3 cells_grid(blocks_for(n_cells, TPB, 2048)), block(TPB);
  hipLaunchKernelGGL(k_bev_clear, cells_grid, block, 0, st, (int)n_cells, key_max, key_min, winner, count);
  if (n_rows > 0) {
    const dim3 rows_grid(cdiv(n_rows, TPB));
    hipLaunchKernelGGL(k_bev_keys, rows_grid, block, 0, st, a, key_max, z_min ? key_min : nullptr, count);
    if (top_index || top_label) hipLaunchKernelGGL(k_bev_winner, rows_grid, block, 0, st, a, (const unsigned long long*)key_max, winner);
  }
  hipLaunchKernelGGL(k_bev_resolve, cells_grid, block, 0, st, a, (int)n_cells, (const unsigned long long*)key_max,
                     (const unsigned long long*)key_min, (const unsigned*)winner, (const int32_t*)count, z_max, z_min, top_index, top_label,
                     occupancy);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
