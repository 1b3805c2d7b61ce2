// Distance field on the device: a state map (occupancy_ops.hip's `state`, or any uint8 map) -> per cell of the window the exact squared
// Euclidean distance, in cells, to the nearest source cell, truncated at a radius R, which cell that is, the clearance in metres and an
// inflated costmap; and a check of K candidate trajectories against that costmap.  The field is separable: launch 1 finds the nearest
// source of every cell inside its own row from the row's source bits (ballots, count-leading / count-trailing zeros), launch 2 scans
// the rows i - R .. i + R of a column outward over those results, held in LDS.  Integer arithmetic and two table look-ups: no float
// operation on the device but the fp64 divide, floor and compare of the path check.  No atomics, no workgroup waits for another.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_field_rows 22 VGPRs, 96 bytes of LDS; k_field_cols 42 VGPRs,
// dynamic LDS of (T + 2R) * 128 bytes (T = 8 .. 64 rows; at R = 255 66304 .. 73472: two workgroups to a CU); k_field_paths 46 VGPRs, no
// LDS.  No scratch, 8 waves per SIMD by the registers.
#include "raster.h"       // finite_d, aligned16
#include <string.h>

// the path check is specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256, WAVES = TPB / CRD_WAVE;
constexpr int MAX_R = 255;
constexpr int MAX_HALO_WORDS = (MAX_R + 63) / 64;                       // 64-bit words of source bits a row search reaches to each side
constexpr int MAX_ROW_WORDS = WAVES + 2 * MAX_HALO_WORDS;
constexpr short NO_SOURCE = 0x7fff;                                     // an LDS entry of launch 2: the row has no source within R
constexpr int MAX_TILE = 64, MIN_TILE = 8;                              // rows of a tile of launch 2
constexpr int SCAN = 8;                                                 // distances of launch 2's scan whose LDS reads are issued together
constexpr int MAX_COL_LDS = (MAX_TILE + 2 * MAX_R) * CRD_WAVE * 2;      // bytes: col_lds(MAX_TILE, MAX_R)

struct Field {
  const unsigned char* state;
  int M, nx, ny, sources, R, unknown_cost;
  const float* clear_table;
  const unsigned char* cost_table;
  int32_t* row_near;                                                    // the workspace
  int32_t *dist2, *nearest;
  float* clearance;                                                     // may be NULL
  unsigned char* cost;                                                  // may be NULL
};

// Launch 1: a workgroup takes 256 consecutive cells of one row.  Its four waves ballot the source predicate of the 4 + 2 * halo words
// of 64 cells around them into LDS (a word outside the row is 0); every thread then finds the nearest set bit at or below its own and
// the nearest above it.  The lower j' of two equal distances is the one found downwards.
__global__ __launch_bounds__(TPB) void k_field_rows(Field a, int halo, int segs, long long n_tiles) {
  __shared__ unsigned long long bits[MAX_ROW_WORDS];
  const int lane = threadIdx.x & (CRD_WAVE - 1), wave = threadIdx.x >> 6;
  const int n_words = WAVES + 2 * halo;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row = tile / segs;                                  // m * nx + i
    const int seg = (int)(tile - row * segs);
    const unsigned char* s = a.state + row * a.ny;
    const int w0 = seg * WAVES - halo;                                  // the row's word that bits[0] holds
    for (int k = wave; k < n_words; k += WAVES) {
      const int j = (w0 + k) * CRD_WAVE + lane;
      bool src = false;
      if (j >= 0 && j < a.ny) {
        const int v = s[j];
        src = v < 8 && ((a.sources >> v) & 1);
      }
      const unsigned long long word = __ballot(src);
      if (lane == 0) bits[k] = word;
    }
    __syncthreads();
    const int j = (seg * WAVES + wave) * CRD_WAVE + lane;
    if (j < a.ny) {
      const int k0 = halo + wave;
      int below = -1, above = -1;                                       // j' <= j and j' > j, -1: none in the words held
      unsigned long long w = bits[k0] & (~0ull >> (CRD_WAVE - 1 - lane));
      for (int k = k0; ; w = bits[--k]) {
        if (w) { below = (w0 + k) * CRD_WAVE + (CRD_WAVE - 1 - __clzll((long long)w)); break; }
        if (k == 0) break;
      }
      w = lane == CRD_WAVE - 1 ? 0ull : bits[k0] & (~0ull << (lane + 1));
      for (int k = k0; ; w = bits[++k]) {
        if (w) { above = (w0 + k) * CRD_WAVE + (__ffsll((long long)w) - 1); break; }
        if (k == n_words - 1) break;
      }
      const int d_below = below >= 0 ? j - below : a.R + 1, d_above = above >= 0 ? above - j : a.R + 1;
      int near = -1;
      if (d_below <= d_above) { if (d_below <= a.R) near = below; } else if (d_above <= a.R) near = above;
      a.row_near[row * a.ny + j] = near;
    }
    __syncthreads();                                                    // bits is written again by the next tile
  }
}

// Launch 2: a workgroup takes T rows of 64 columns, the lanes along j, so every row read is one 256-byte line.  off[s][lane] = j' - j
// of row i0 - R + s (NO_SOURCE without one; rows outside the map are neither written nor read).  A wave takes every fourth row of the
// tile and scans outward from i' = i: upwards a candidate replaces the best so far on t <= best, since its row is lower than every
// row seen, downwards on t < best only; the scan ends once d * d exceeds the best t -- not at equality, where a source straight above
// still wins by its lower row.  A row outside the map or beyond R reads as NO_SOURCE.
__global__ __launch_bounds__(TPB) void k_field_cols(Field a, int T, int row_tiles, int col_tiles, long long n_tiles) {
  extern __shared__ __attribute__((aligned(16))) short off[];
  const int lane = threadIdx.x & (CRD_WAVE - 1), wave = threadIdx.x >> 6;
  const int R = a.R, R2 = R * R, FAR = R2 + 1;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tj = (int)(tile % col_tiles);
    const long long rest = tile / col_tiles;
    const int ti = (int)(rest % row_tiles), m = (int)(rest / row_tiles);
    const int i0 = ti * T, j = tj * CRD_WAVE + lane, lo = i0 - R;
    const int first = lo < 0 ? 0 : lo, end = i0 + T + R < a.nx ? i0 + T + R : a.nx;       // the rows of the map among lo .. lo + T + 2R - 1
    const long long map0 = (long long)m * a.nx;
    for (int i2 = first + wave; i2 < end; i2 += WAVES) {
      short v = NO_SOURCE;
      if (j < a.ny) {
        const int near = a.row_near[(map0 + i2) * a.ny + j];
        if (near >= 0) v = (short)(near - j);                           // |near - j| <= R <= 255
      }
      off[(i2 - lo) * CRD_WAVE + lane] = v;
    }
    __syncthreads();
    const int i_end = i0 + T < a.nx ? i0 + T : a.nx;
    for (int i = i0 + wave; i < i_end; i += WAVES) {
      if (j >= a.ny) continue;
      int best = FAR, best_i = -1, best_off = 0;
      {
        const int v = off[(i - lo) * CRD_WAVE + lane];
        if (v != NO_SOURCE && v * v <= R2) { best = v * v; best_i = i; best_off = v; }
      }
      for (int d0 = 1; d0 <= R && d0 * d0 <= best; d0 += SCAN) {        // SCAN distances at a time: their reads do not wait for each other
        short up[SCAN], down[SCAN];
#pragma unroll
        for (int u = 0; u < SCAN; ++u) {
          const int d = d0 + u;
          up[u] = d <= R && i - d >= first ? off[(i - d - lo) * CRD_WAVE + lane] : NO_SOURCE;
          down[u] = d <= R && i + d < end ? off[(i + d - lo) * CRD_WAVE + lane] : NO_SOURCE;
        }
#pragma unroll
        for (int u = 0; u < SCAN; ++u) {
          const int d = d0 + u;
          if (d * d > best) break;
          int v = up[u], t = d * d + v * v;
          if (v != NO_SOURCE && t <= best && t <= R2) { best = t; best_i = i - d; best_off = v; }
          v = down[u]; t = d * d + v * v;
          if (v != NO_SOURCE && t < best) { best = t; best_i = i + d; best_off = v; }
        }
      }
      const long long idx = (map0 + i) * a.ny + j;
      a.dist2[idx] = best;
      a.nearest[idx] = best_i < 0 ? -1 : best_i * a.ny + (j + best_off);
      if (a.clearance) a.clearance[idx] = a.clear_table[best];
      if (a.cost) {
        int c = a.cost_table[best];
        if (a.unknown_cost > 0 && a.state[idx] == 0 && c < a.unknown_cost) c = a.unknown_cost;
        a.cost[idx] = (unsigned char)c;
      }
    }
    __syncthreads();                                                    // off is written again by the next tile
  }
}

struct Paths {
  const double* xy;
  const int32_t *n_poses, *path_map;                                    // each may be NULL
  int K, P, M, nx, ny, FAR, blocked_at, outside_blocks;
  const long long* origin;
  double cell;
  const unsigned char *state, *cost;
  const int32_t* dist2;
  int32_t *first_blocked, *min_dist2, *n_outside, *n_unknown, *pose_cell;   // pose_cell may be NULL
  unsigned char* max_cost;
};

// One wave per path, the lanes over its poses; integer minimum, maximum and add over the wave, which no order changes.
__global__ __launch_bounds__(TPB) void k_field_paths(Paths a) {
  const int lane = threadIdx.x & (CRD_WAVE - 1);
  const int k = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (k >= a.K) return;                                                 // the whole wave
  int n = a.n_poses ? a.n_poses[k] : a.P;
  n = n < 0 ? 0 : (n > a.P ? a.P : n);
  const int m = a.path_map ? a.path_map[k] : 0;
  const bool has_map = m >= 0 && m < a.M;
  long long ox = 0, oy = 0;
  if (has_map) { ox = a.origin[m * 2]; oy = a.origin[m * 2 + 1]; }
  const double x_lo = (double)ox, x_hi = (double)(long long)((unsigned long long)ox + (unsigned long long)a.nx);
  const double y_lo = (double)oy, y_hi = (double)(long long)((unsigned long long)oy + (unsigned long long)a.ny);
  int first = 0x7fffffff, worst = 0, nearest = a.FAR, outside = 0, unknown = 0;
  for (int p = lane; p < a.P; p += CRD_WAVE) {
    const long long at = (long long)k * a.P + p;
    if (p >= n) {
      if (a.pose_cell) a.pose_cell[at] = -2;
      continue;
    }
    const double X = a.xy[at * 2], Y = a.xy[at * 2 + 1];
    const double wx = floor(X / a.cell), wy = floor(Y / a.cell);
    int c = -1;
    if (has_map && finite_d(X) && finite_d(Y) && wx >= x_lo && wx < x_hi && wy >= y_lo && wy < y_hi) {      // on the doubles
      const long long i = (long long)wx - ox, j = (long long)wy - oy;
      if (i >= 0 && i < a.nx && j >= 0 && j < a.ny) c = (int)i * a.ny + (int)j;     // never false with an origin crd_occupancy_update wrote
    }
    if (a.pose_cell) a.pose_cell[at] = c;
    bool blocked;
    if (c >= 0) {
      const long long idx = (long long)m * a.nx * a.ny + c;
      const int cost = a.cost[idx], d2 = a.dist2[idx];
      worst = cost > worst ? cost : worst;
      nearest = d2 < nearest ? d2 : nearest;
      unknown += a.state[idx] == 0 ? 1 : 0;
      blocked = cost >= a.blocked_at;
    } else {
      ++outside;
      blocked = a.outside_blocks != 0;
    }
    if (blocked && p < first) first = p;
  }
#pragma unroll
  for (int d = CRD_WAVE / 2; d > 0; d >>= 1) {
    const int f = __shfl_xor(first, d), w = __shfl_xor(worst, d), q = __shfl_xor(nearest, d);
    first = f < first ? f : first;
    worst = w > worst ? w : worst;
    nearest = q < nearest ? q : nearest;
    outside += __shfl_xor(outside, d);
    unknown += __shfl_xor(unknown, d);
  }
  if (lane == 0) {
    a.first_blocked[k] = first == 0x7fffffff ? -1 : first;
    a.max_cost[k] = (unsigned char)worst;
    a.min_dist2[k] = nearest;
    a.n_outside[k] = outside;
    a.n_unknown[k] = unknown;
  }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf

inline int col_lds(int T, int R) { return (T + 2 * R) * CRD_WAVE * 2; }   // bytes of launch 2's LDS

// Rows of a tile of launch 2.  Every tile loads a halo of 2R rows, which a higher tile spreads over more cells, but a wave scans its
// rows one after the other, and the scans are what takes the time.  So the tile is the highest that still leaves a workgroup for every
// place the chip has: 256 CUs, on each as many workgroups as its 160 KiB of LDS hold, eight at the most (32 waves).  A small map is cut
// into tiles of 8 rows.  (Measured on 8 x 400 x 400 cells, tiles of 8 rows against tiles of 64: 43.8 against 73.7 us at R 16, 97.2
// against 204.9 us at R 64; tiles of 32 against 64 at R 255: 553 against 705 us.)
inline int tile_rows(int M, int nx, int ny, int R) {
  int T = MAX_TILE;
  for (; T > MIN_TILE; T >>= 1) {
    const int fit = 160 * 1024 / col_lds(T, R), per_cu = fit < 8 ? fit : 8;
    if ((long long)M * cdiv(nx, T) * cdiv(ny, CRD_WAVE) >= 256ll * per_cu) break;
  }
  return T;
}

// what both entries ask of a map and its radius
inline int check_shape(const char* name, int32_t M, int32_t nx, int32_t ny, int32_t max_cells) {
  CRD_CHECK_ARG(M >= 1, "%s: bad argument (M %d maps)", name, M);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  const long long n_cells = (long long)M * nx * ny;
  CRD_CHECK_ARG(n_cells < 0x80000000ll, "%s: bad argument (M * nx * ny = %lld cells are more than the 32-bit indices hold)", name, n_cells);
  CRD_CHECK_ARG(max_cells >= 1 && max_cells <= MAX_R, "%s: bad argument (max_cells %d is not in 1 .. 255)", name, max_cells);
  return CRD_OK;
}

}  // namespace

extern "C" int crd_distance_field(const uint8_t* state, int32_t M, int32_t nx, int32_t ny, int32_t sources, int32_t max_cells,
                                  int32_t unknown_cost, const float* clear_table, const uint8_t* cost_table, void* workspace,
                                  int64_t workspace_bytes, int32_t* dist2, int32_t* nearest, float* clearance, uint8_t* cost,
                                  crd_stream_t stream) {
  const char* name = "crd_distance_field";
  const int rc = check_shape(name, M, nx, ny, max_cells);
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(sources >= 1 && sources <= 255, "%s: bad argument (sources %d is not a mask of the states 0 .. 7, 1 .. 255)", name, sources);
  CRD_CHECK_ARG(unknown_cost >= 0 && unknown_cost <= 255, "%s: bad argument (unknown_cost %d is not in 0 .. 255)", name, unknown_cost);
  CRD_CHECK_ARG(state && clear_table && cost_table && workspace && dist2 && nearest,
                "%s: null pointer (state, clear_table, cost_table, workspace, dist2, nearest)", name);
  const long long n_cells = (long long)M * nx * ny, need = (4 * n_cells + 15) & ~15ll;
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  CRD_CHECK_ARG(aligned_to(clear_table, 4) && aligned_to(dist2, 4) && aligned_to(nearest, 4) && aligned_to(clearance, 4),
                "%s: bad argument (clear_table, dist2, nearest and clearance must be 4-byte aligned)", name);
  Field a;
  a.state = state; a.M = M; a.nx = nx; a.ny = ny; a.sources = sources; a.R = max_cells; a.unknown_cost = unknown_cost;
  a.clear_table = clear_table; a.cost_table = cost_table; a.row_near = reinterpret_cast<int32_t*>(workspace); a.dist2 = dist2;
  a.nearest = nearest; a.clearance = clearance; a.cost = cost;
  hipStream_t st = as_stream(stream);
  const int segs = cdiv(ny, TPB), halo = (max_cells + 63) / 64;
  const long long row_work = (long long)M * nx * segs;
  hipLaunchKernelGGL(k_field_rows, dim3((unsigned)(row_work < 65536 ? row_work : 65536)), dim3(TPB), 0, st, a, halo, segs, row_work);
  const int T = tile_rows(M, nx, ny, max_cells), row_tiles = cdiv(nx, T), col_tiles = cdiv(ny, CRD_WAVE);
  const long long col_work = (long long)M * row_tiles * col_tiles;
  const int lds = col_lds(T, max_cells);
  crd_reserve_lds_once<&k_field_cols>(MAX_COL_LDS, "k_field_cols");
  hipLaunchKernelGGL(k_field_cols, dim3((unsigned)(col_work < 65536 ? col_work : 65536)), dim3(TPB), lds, st, a, T, row_tiles, col_tiles,
                     col_work);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}

extern "C" int crd_field_paths(const double* xy, const int32_t* n_poses, const int32_t* path_map, int32_t K, int32_t P, const int64_t* origin,
                               uint64_t cell_f64_bits, const uint8_t* state, const int32_t* dist2, const uint8_t* cost, int32_t M, int32_t nx,
                               int32_t ny, int32_t max_cells, int32_t blocked_at, int32_t outside_blocks, int32_t* first_blocked,
                               uint8_t* max_cost, int32_t* min_dist2, int32_t* n_outside, int32_t* n_unknown, int32_t* pose_cell,
                               crd_stream_t stream) {
  const char* name = "crd_field_paths";
  const int rc = check_shape(name, M, nx, ny, max_cells);
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(K >= 1 && P >= 1, "%s: bad argument (K %d paths of P %d poses)", name, K, P);
  CRD_CHECK_ARG(blocked_at >= 1 && blocked_at <= 255, "%s: bad argument (blocked_at %d is not in 1 .. 255)", name, blocked_at);
  CRD_CHECK_ARG(outside_blocks == 0 || outside_blocks == 1, "%s: bad argument (outside_blocks %d is neither 0 nor 1)", name, outside_blocks);
  const double cell = from_bits(cell_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(xy && origin && state && dist2 && cost && first_blocked && max_cost && min_dist2 && n_outside && n_unknown,
                "%s: null pointer (xy, origin, state, dist2, cost, first_blocked, max_cost, min_dist2, n_outside, n_unknown)", name);
  CRD_CHECK_ARG(aligned_to(xy, 8) && aligned_to(origin, 8) && aligned_to(n_poses, 4) && aligned_to(path_map, 4) && aligned_to(dist2, 4) &&
                    aligned_to(first_blocked, 4) && aligned_to(min_dist2, 4) && aligned_to(n_outside, 4) && aligned_to(n_unknown, 4) &&
                    aligned_to(pose_cell, 4),
                "%s: bad argument (xy and origin must be 8-byte aligned, n_poses, path_map, dist2, first_blocked, min_dist2, n_outside, "
                "n_unknown and pose_cell 4-byte)", name);
  Paths a;
  a.xy = xy; a.n_poses = n_poses; a.path_map = path_map; a.K = K; a.P = P; a.M = M; a.nx = nx; a.ny = ny; a.FAR = max_cells * max_cells + 1;
  a.blocked_at = blocked_at; a.outside_blocks = outside_blocks; a.origin = reinterpret_cast<const long long*>(origin); a.cell = cell;
  a.state = state; a.cost = cost; a.dist2 = dist2; a.first_blocked = first_blocked; a.min_dist2 = min_dist2; a.n_outside = n_outside;
  a.n_unknown = n_unknown; a.pose_cell = pose_cell; a.max_cost = max_cost;
  hipLaunchKernelGGL(k_field_paths, dim3(cdiv(K, WAVES)), dim3(TPB), 0, as_stream(stream), a);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
