// Navigation field on the device: a costmap (field_ops.hip's `cost`, or any uint8 map) and goal points -> per cell of the window the least
// cost to reach a goal over 8-connected paths of passable cells (chamfer weights 5 and 7 times neutral + cost of the cell left), the
// neighbour to step to, and the paths that follow those steps from K starts.  Integer arithmetic only, no atomics, no workgroup waits
// for another; the only fp64 is the divide, floor and compare that find the cell of a goal or a start, and the cell centres of a path.
//
// The cost-to-go is a Gauss-Seidel relaxation in row sweeps, one wave per map.  A row step takes row i from the row just finished (its
// three neighbours above or below) and then settles the row in itself, left to right and right to left.  Settling is a min-plus scan: a
// cell is the function x -> min(x + A, B) of the value x that arrives from its neighbour (A = 5 * w, B = its own value; a wall is A = B =
// INF), functions compose associatively, so a lane folds its own strip of C columns serially and the 64 lanes combine with four
// DPP row shifts and three row totals read as scalars.  A round is a sweep down and a sweep up; the rounds needed are about the vertical reversals of the worst path, not its length.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_nav_sweep held in registers <1> 30 VGPRs, <2> 33, <4> 46, <8> 140, in
// chunks <8> 58; k_nav_next 28, k_nav_paths 34, k_nav_fill 5; no LDS, no scratch.
#include "raster.h"       // finite_d
#include <string.h>

// the cell of a goal or a start and the centres of a path are specified operation by operation (include/camradepth_hip.h) and compared
// bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int UNREACHED = 0x7fffffff;
constexpr unsigned INF = 0x7fffffffu;                                   // UNREACHED in the scans' unsigned arithmetic: INF + INF fits
constexpr int MAX_CELLS = 1 << 19;                                      // of one map: 3570 * 2^19 < 2^31
constexpr int MAX_STRIP = 8;                                            // columns of a lane: the sweep is built for 1, 2, 4 and 8
constexpr int ON_GOAL = 8, NO_STEP = 255;                               // codes of `next` beside the neighbours 0 .. 7
__constant__ const int DI[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, DJ[8] = {-1, 0, 1, -1, 1, -1, 0, 1};

struct Nav {
  const unsigned char* cost;
  int M, nx, ny;
  const double* goals;
  const int32_t* n_goals;                                               // may be NULL
  int G;
  const long long* origin;
  double cell;
  int neutral, blocked_at, max_rounds;
  int32_t* togo;
  unsigned char* next;                                                  // may be NULL
  int32_t* info;
};

// crd_field_paths' INSIDE rule: i * ny + j of the cell of (X, Y) in the window at (ox, oy), -1 outside it or not finite
__device__ __forceinline__ int window_cell(double X, double Y, double cell, long long ox, long long oy, int nx, int ny) {
  const double x_lo = (double)ox, x_hi = (double)(long long)((unsigned long long)ox + (unsigned long long)nx);
  const double y_lo = (double)oy, y_hi = (double)(long long)((unsigned long long)oy + (unsigned long long)ny);
  const double wx = floor(X / cell), wy = floor(Y / cell);
  if (!(finite_d(X) && finite_d(Y) && wx >= x_lo && wx < x_hi && wy >= y_lo && wy < y_hi)) return -1;       // on the doubles
  const long long i = (long long)wx - ox, j = (long long)wy - oy;
  return i >= 0 && i < nx && j >= 0 && j < ny ? (int)i * ny + (int)j : -1;
}

// Launch 1: togo = UNREACHED everywhere.
__global__ __launch_bounds__(TPB) void k_nav_fill(int32_t* togo, long long n) {
  for (long long t = (long long)blockIdx.x * TPB + threadIdx.x; t < n; t += (long long)gridDim.x * TPB) togo[t] = UNREACHED;
}

// A run of cells as the function x -> min(x + A, B) of the value arriving at its near end, giving the value at its far end.
struct Run { unsigned A, B; };
// `first` is passed through before `then`.  Every operand is at most INF, so no sum leaves 32 bits.
__device__ __forceinline__ Run chain(Run first, Run then) {
  const unsigned A = first.A + then.A, B = first.B + then.A;
  return {A < INF ? A : INF, B < then.B ? B : then.B};
}

// DPP controls (gfx9): row_shr:n moves a value n lanes up inside its row of 16 lanes, row_shl:n down, wave_shr:1 / wave_shl:1 one lane
// over the whole wave.  A lane without a source keeps `old`.
constexpr int ROW_SHL = 0x100, ROW_SHR = 0x110, WAVE_SHL1 = 0x130, WAVE_SHR1 = 0x138;
template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned old, unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ Run dpp_run(Run v) { return {dpp<CTRL>(0u, v.A), dpp<CTRL>(INF, v.B)}; }      // the identity where there is no source
__device__ __forceinline__ Run lane_run(Run v, int l) {
  return {(unsigned)__builtin_amdgcn_readlane((int)v.A, l), (unsigned)__builtin_amdgcn_readlane((int)v.B, l)};
}

// The chain of the runs of the lanes before this one (FWD: the lanes 0 .. lane - 1, lowest first) or behind it (the lanes 63 .. lane + 1,
// highest first); the identity for the first lane.  Four shifted steps inside each row of 16 lanes, then the three row totals that
// matter, read as scalars, in front of them.
template <bool FWD>
__device__ __forceinline__ Run lanes_before(Run mine, int lane) {
  constexpr int SH = FWD ? ROW_SHR : ROW_SHL;
  Run inc = mine;
  inc = chain(dpp_run<SH + 1>(inc), inc);
  inc = chain(dpp_run<SH + 2>(inc), inc);
  inc = chain(dpp_run<SH + 4>(inc), inc);
  inc = chain(dpp_run<SH + 8>(inc), inc);
  const Run t1 = lane_run(inc, FWD ? 15 : 48), t2 = lane_run(inc, FWD ? 31 : 32), t3 = lane_run(inc, FWD ? 47 : 16);
  const Run p2 = chain(t1, t2), p3 = chain(p2, t3);                     // in front of the second, third and fourth row on the way
  const int nth = FWD ? lane >> 4 : 3 - (lane >> 4);                    // this lane's row on the way
  Run rows = {0u, INF};
  if (nth == 1) rows = t1;
  if (nth == 2) rows = p2;
  if (nth == 3) rows = p3;
  return chain(rows, dpp_run<SH + 1>(inc));
}

// The strip of C columns from j0 of a row: step[c] = 5 * w, INF on a wall and beyond the row; value[c] = togo, INF on a wall.
template <int C>
__device__ __forceinline__ void load_strip(const Nav& a, const unsigned char* crow, const int32_t* row, int j0, unsigned (&step)[C],
                                           unsigned (&value)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = j0 + c;
    step[c] = INF; value[c] = INF;
    if (j < a.ny) {
      const int cst = crow[j];
      if (cst < a.blocked_at) { step[c] = 5u * (unsigned)(a.neutral + cst); value[c] = (unsigned)row[j]; }
    }
  }
}

// d from the row just finished: above[q] is that row at the columns j0 - 1 + q, INF on a wall, beyond the row and without a row.
template <int C>
__device__ __forceinline__ void relax(const unsigned (&step)[C], unsigned (&d)[C], const unsigned (&above)[C + 2]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (step[c] == INF) continue;                                       // step / 5 * 7 is exact; a value below INF is at most 3570 * (2^19 - 1)
    const unsigned diag = step[c] / 5u * 7u;
    if (above[c] != INF && above[c] + diag < d[c]) d[c] = above[c] + diag;
    if (above[c + 1] != INF && above[c + 1] + step[c] < d[c]) d[c] = above[c + 1] + step[c];
    if (above[c + 2] != INF && above[c + 2] + diag < d[c]) d[c] = above[c + 2] + diag;
  }
}

// d along the row, left to right (FWD) or right to left, over the strips of all lanes.  carry: the value that arrives from the chunk
// before on the way (INF: none); it leaves as the value of this chunk's last cell.
template <int C, bool FWD>
__device__ __forceinline__ void settle(const unsigned (&step)[C], unsigned (&d)[C], unsigned& carry, int lane) {
  Run mine = {0u, INF};
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int c = FWD ? k : C - 1 - k;
    mine = chain(mine, {step[c], d[c]});
  }
  const Run before = lanes_before<FWD>(mine, lane);
  unsigned x = carry + before.A < before.B ? carry + before.A : before.B;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int c = FWD ? k : C - 1 - k;
    x = x + step[c] < d[c] ? x + step[c] : d[c];
    d[c] = x;
  }
  carry = (unsigned)__builtin_amdgcn_readlane((int)x, FWD ? CRD_WAVE - 1 : 0);
}

// One row step of a row of at most 64 * C cells, lane l holding the columns l * C .. l * C + C - 1: the row just finished is still in
// this wave's registers (prev), its two cells beside the strip come from the neighbour lanes.  step and d arrive loaded (load_strip);
// d leaves as the row's new values, which are stored where they fell.  -> whether this lane lowered a value.
template <int C>
__device__ __forceinline__ bool row_step_held(const unsigned (&step)[C], unsigned (&d)[C], const unsigned (&prev)[C], bool has_prev, int32_t* row,
                                              int lane) {
  unsigned above[C + 2], was[C];
  above[0] = dpp<WAVE_SHR1>(INF, prev[C - 1]);
  above[C + 1] = dpp<WAVE_SHL1>(INF, prev[0]);
#pragma unroll
  for (int c = 0; c < C; ++c) above[c + 1] = prev[c];
#pragma unroll
  for (int q = 0; q < C + 2; ++q) above[q] = has_prev ? above[q] : INF;
#pragma unroll
  for (int c = 0; c < C; ++c) was[c] = d[c];
  relax<C>(step, d, above);
  unsigned carry = INF;
  settle<C, true>(step, d, carry, lane);
  carry = INF;
  settle<C, false>(step, d, carry, lane);
  bool changed = false;
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (d[c] < was[c]) { row[lane * C + c] = (int)d[c]; changed = true; }
  return changed;
}

// One row step of a longer row: row i of the map from row p (-1: none), both in memory, in chunks of 64 * C columns, lane l holding the
// columns l * C .. l * C + C - 1 of a chunk.  The chunk where the first scan ends is the one where the second begins, so it stays in
// registers; the others store the first scan's result and load it again.  -> whether this lane lowered a value.
template <int C>
__device__ __forceinline__ bool row_step_chunked(const Nav& a, const unsigned char* cost, int32_t* togo, int i, int p, int lane) {
  const int ny = a.ny, span = CRD_WAVE * C, n_chunks = (ny + span - 1) / span;
  const unsigned char* crow = cost + i * ny;                            // a map has at most 2^19 cells
  int32_t* row = togo + i * ny;
  const int32_t* prow = p >= 0 ? togo + p * ny : nullptr;
  unsigned step[C], d[C], was[C];
  bool changed = false;
  unsigned carry = INF;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int j0 = ch * span + lane * C;
    load_strip<C>(a, crow, row, j0, step, d);
    unsigned above[C + 2];
#pragma unroll
    for (int q = 0; q < C + 2; ++q) {
      const int j = j0 - 1 + q;
      above[q] = prow && j >= 0 && j < ny ? (unsigned)prow[j] : INF;    // a wall holds UNREACHED
    }
#pragma unroll
    for (int c = 0; c < C; ++c) was[c] = d[c];
    relax<C>(step, d, above);
    settle<C, true>(step, d, carry, lane);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      changed |= d[c] < was[c];
      if (ch < n_chunks - 1 && step[c] != INF) row[j0 + c] = (int)d[c];
    }
  }
  carry = INF;
  for (int ch = n_chunks - 1; ch >= 0; --ch) {
    const int j0 = ch * span + lane * C;
    if (ch < n_chunks - 1) load_strip<C>(a, crow, row, j0, step, d);    // this lane's own stores of the first scan
#pragma unroll
    for (int c = 0; c < C; ++c) was[c] = d[c];
    settle<C, false>(step, d, carry, lane);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      changed |= d[c] < was[c];
      if (step[c] != INF) row[j0 + c] = (int)d[c];
    }
  }
  __threadfence_block();                                                // the next row step reads this row through other lanes
  return changed;
}

// Launch 2: one wave per map.  The goals' cells to 0, then rounds of a sweep down and a sweep up until one changes nothing or
// max_rounds are done; every loop bound is the same for all lanes.  HELD: the row fits one chunk (ny <= 64 * C), so a sweep passes the
// row just finished on in registers and loads the next row's cost and togo, which do not depend on it, before it works on this one.
template <int C, bool HELD>
__global__ __launch_bounds__(CRD_WAVE) void k_nav_sweep(Nav a) {
  const int lane = threadIdx.x, m = blockIdx.x;
  const long long map0 = (long long)m * a.nx * a.ny;
  const unsigned char* cost = a.cost + map0;
  int32_t* togo = a.togo + map0;
  int n = a.n_goals ? a.n_goals[m] : a.G;
  n = n < 0 ? 0 : (n > a.G ? a.G : n);
  const long long ox = a.origin[m * 2], oy = a.origin[m * 2 + 1];
  int used = 0;
  for (int g = lane; g < n; g += CRD_WAVE) {
    const double* xy = a.goals + ((long long)m * a.G + g) * 2;
    const int c = window_cell(xy[0], xy[1], a.cell, ox, oy, a.nx, a.ny);
    if (c >= 0 && cost[c] < a.blocked_at) { togo[c] = 0; ++used; }
  }
#pragma unroll
  for (int d = CRD_WAVE / 2; d > 0; d >>= 1) used += __shfl_xor(used, d);
  __threadfence_block();                                                // the rows are read through other lanes than wrote the goals
  int rounds = 0;
  bool changed;
  do {
    bool mine = false;
    if constexpr (HELD) {
      const int ny = a.ny, j0 = lane * C;
      unsigned step[C], d[C], next_step[C], next_d[C], prev[C];
#pragma unroll
      for (int c = 0; c < C; ++c) { next_step[c] = INF; next_d[c] = INF; prev[c] = INF; }
      load_strip<C>(a, cost, togo, j0, step, d);
      for (int i = 0; i < a.nx; ++i) {                                  // down
        if (i + 1 < a.nx) load_strip<C>(a, cost + (i + 1) * ny, togo + (i + 1) * ny, j0, next_step, next_d);
        mine |= row_step_held<C>(step, d, prev, i > 0, togo + i * ny, lane);
#pragma unroll
        for (int c = 0; c < C; ++c) { prev[c] = d[c]; step[c] = next_step[c]; d[c] = next_d[c]; }
      }
      if (a.nx > 1) load_strip<C>(a, cost + (a.nx - 2) * ny, togo + (a.nx - 2) * ny, j0, step, d);
      for (int i = a.nx - 2; i >= 0; --i) {                             // up: prev is row nx - 1
        if (i > 0) load_strip<C>(a, cost + (i - 1) * ny, togo + (i - 1) * ny, j0, next_step, next_d);
        mine |= row_step_held<C>(step, d, prev, true, togo + i * ny, lane);
#pragma unroll
        for (int c = 0; c < C; ++c) { prev[c] = d[c]; step[c] = next_step[c]; d[c] = next_d[c]; }
      }
    } else {
      for (int i = 0; i < a.nx; ++i) mine |= row_step_chunked<C>(a, cost, togo, i, i - 1, lane);
      for (int i = a.nx - 2; i >= 0; --i) mine |= row_step_chunked<C>(a, cost, togo, i, i + 1, lane);
    }
    changed = __any(mine) != 0;
    ++rounds;
  } while (changed && rounds < a.max_rounds);
  if (lane == 0) {
    int32_t* info = a.info + m * 4;
    info[0] = changed ? 0 : 1; info[1] = rounds; info[2] = used; info[3] = n - used;
  }
}

// Launch 3: the direction map from the final togo, a thread per cell.
__global__ __launch_bounds__(TPB) void k_nav_next(Nav a, long long n_cells) {
  const int per_map = a.nx * a.ny;
  for (long long t = (long long)blockIdx.x * TPB + threadIdx.x; t < n_cells; t += (long long)gridDim.x * TPB) {
    const int here = a.togo[t];
    int code = NO_STEP;
    if (here == 0) code = ON_GOAL;
    else if (here != UNREACHED) {
      const long long map0 = t / per_map * per_map;
      const int c = (int)(t - map0), i = c / a.ny, j = c - i * a.ny;
      const int w = a.neutral + a.cost[t];
      long long best = 0x7fffffffffffffffll;
      for (int k = 0; k < 8; ++k) {                                     // ascending: strictly less keeps the lowest code
        const int i2 = i + DI[k], j2 = j + DJ[k];
        if (i2 < 0 || i2 >= a.nx || j2 < 0 || j2 >= a.ny) continue;
        const int there = a.togo[map0 + i2 * a.ny + j2];
        if (there == UNREACHED) continue;
        const long long v = (long long)there + (DI[k] != 0 && DJ[k] != 0 ? 7 : 5) * w;
        if (v < best) { best = v; code = k; }
      }
    }
    a.next[t] = (unsigned char)code;
  }
}

struct NavPaths {
  const double* starts;
  const int32_t* path_map;                                              // may be NULL
  int K, P, M, nx, ny;
  const long long* origin;
  double cell;
  const int32_t* togo;
  const unsigned char* next;
  int32_t* cells;
  double* xy;                                                           // may be NULL
  int32_t *n_cells, *start_togo, *status;
};

// A path is a pointer chase, one step after the other: one lane per path, the maps in L2.  A code of `next` that is no step (which
// crd_nav_field never leaves on a reached cell) or a step out of the window ends the path as cut.
__global__ __launch_bounds__(CRD_WAVE) void k_nav_paths(NavPaths a) {
  const int k = blockIdx.x * CRD_WAVE + threadIdx.x;
  if (k >= a.K) return;
  const int m = a.path_map ? a.path_map[k] : 0;
  int c = -1, first = UNREACHED, status = 2, n = 0;
  long long ox = 0, oy = 0, map0 = 0;
  if (m >= 0 && m < a.M) {
    ox = a.origin[m * 2]; oy = a.origin[m * 2 + 1];
    map0 = (long long)m * a.nx * a.ny;
    c = window_cell(a.starts[k * 2], a.starts[k * 2 + 1], a.cell, ox, oy, a.nx, a.ny);
  }
  if (c >= 0) {
    first = a.togo[map0 + c];
    status = first == UNREACHED ? 3 : 1;
  }
  int32_t* cells = a.cells + (long long)k * a.P;
  double* xy = a.xy ? a.xy + (long long)k * a.P * 2 : nullptr;
  if (status == 1) {
    while (n < a.P) {
      const int i = c / a.ny, j = c - i * a.ny;
      cells[n] = c;
      if (xy) {
        xy[n * 2] = ((double)(ox + i) + 0.5) * a.cell;
        xy[n * 2 + 1] = ((double)(oy + j) + 0.5) * a.cell;
      }
      ++n;
      const int code = a.next[map0 + c];
      if (code == ON_GOAL) { status = 0; break; }
      if (code > 7) break;
      const int i2 = i + DI[code], j2 = j + DJ[code];
      if (i2 < 0 || i2 >= a.nx || j2 < 0 || j2 >= a.ny) break;
      c = i2 * a.ny + j2;
    }
  }
  for (int p = n; p < a.P; ++p) {
    cells[p] = -1;
    if (xy) { xy[p * 2] = __longlong_as_double(0x7ff8000000000000ll); xy[p * 2 + 1] = __longlong_as_double(0x7ff8000000000000ll); }
  }
  a.n_cells[k] = n;
  a.start_togo[k] = first;
  a.status[k] = status;
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf

// what both entries ask of the maps and the cell
inline int check_shape(const char* name, int32_t M, int32_t nx, int32_t ny, double cell) {
  CRD_CHECK_ARG(M >= 1, "%s: bad argument (M %d maps)", name, M);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  CRD_CHECK_ARG((long long)nx * ny <= MAX_CELLS, "%s: bad argument (nx * ny = %lld cells of one map are more than 2^19, where int32 holds every cost)",
                name, (long long)nx * ny);
  const long long n_cells = (long long)M * nx * ny;
  CRD_CHECK_ARG(n_cells < 0x80000000ll, "%s: bad argument (M * nx * ny = %lld cells are more than the 32-bit indices hold)", name, n_cells);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  return CRD_OK;
}

}  // namespace

extern "C" int crd_nav_field(const uint8_t* cost, int32_t M, int32_t nx, int32_t ny, const double* goals, const int32_t* n_goals, int32_t G,
                             const int64_t* origin, uint64_t cell_f64_bits, int32_t neutral, int32_t blocked_at, int32_t max_rounds,
                             int32_t* togo, uint8_t* next, int32_t* info, crd_stream_t stream) {
  const char* name = "crd_nav_field";
  const int rc = check_shape(name, M, nx, ny, from_bits(cell_f64_bits));
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(G >= 1, "%s: bad argument (G %d goals per map)", name, G);
  CRD_CHECK_ARG(neutral >= 1 && neutral <= 255, "%s: bad argument (neutral %d is not in 1 .. 255)", name, neutral);
  CRD_CHECK_ARG(blocked_at >= 1 && blocked_at <= 255, "%s: bad argument (blocked_at %d is not in 1 .. 255)", name, blocked_at);
  CRD_CHECK_ARG(max_rounds >= 1 && max_rounds <= 4096, "%s: bad argument (max_rounds %d is not in 1 .. 4096)", name, max_rounds);
  CRD_CHECK_ARG(cost && goals && origin && togo && info, "%s: null pointer (cost, goals, origin, togo, info)", name);
  CRD_CHECK_ARG(aligned_to(goals, 8) && aligned_to(origin, 8) && aligned_to(n_goals, 4) && aligned_to(togo, 4) && aligned_to(info, 4),
                "%s: bad argument (goals and origin must be 8-byte aligned, n_goals, togo and info 4-byte)", name);
  Nav a;
  a.cost = cost; a.M = M; a.nx = nx; a.ny = ny; a.goals = goals; a.n_goals = n_goals; a.G = G;
  a.origin = reinterpret_cast<const long long*>(origin); a.cell = from_bits(cell_f64_bits); a.neutral = neutral; a.blocked_at = blocked_at;
  a.max_rounds = max_rounds; a.togo = togo; a.next = next; a.info = info;
  hipStream_t st = as_stream(stream);
  const long long n_cells = (long long)M * nx * ny;
  hipLaunchKernelGGL(k_nav_fill, dim3(blocks_for(n_cells, TPB, 2048)), dim3(TPB), 0, st, togo, n_cells);
  const dim3 grid(M), wave(CRD_WAVE);                                   // the held routes: a row is one chunk of 64 * C columns
  if (ny <= CRD_WAVE) hipLaunchKernelGGL((k_nav_sweep<1, true>), grid, wave, 0, st, a);
  else if (ny <= 2 * CRD_WAVE) hipLaunchKernelGGL((k_nav_sweep<2, true>), grid, wave, 0, st, a);
  else if (ny <= 4 * CRD_WAVE) hipLaunchKernelGGL((k_nav_sweep<4, true>), grid, wave, 0, st, a);
  else if (ny <= MAX_STRIP * CRD_WAVE) hipLaunchKernelGGL((k_nav_sweep<MAX_STRIP, true>), grid, wave, 0, st, a);
  else hipLaunchKernelGGL((k_nav_sweep<MAX_STRIP, false>), grid, wave, 0, st, a);
  if (next) hipLaunchKernelGGL(k_nav_next, dim3(blocks_for(n_cells, TPB, 2048)), dim3(TPB), 0, st, a, n_cells);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}

extern "C" int crd_nav_paths(const double* starts, const int32_t* path_map, int32_t K, int32_t P, const int64_t* origin, uint64_t cell_f64_bits,
                             const int32_t* togo, const uint8_t* next, int32_t M, int32_t nx, int32_t ny, int32_t* cells, double* xy,
                             int32_t* n_cells, int32_t* start_togo, int32_t* status, crd_stream_t stream) {
  const char* name = "crd_nav_paths";
  const int rc = check_shape(name, M, nx, ny, from_bits(cell_f64_bits));
  if (rc != CRD_OK) return rc;
  CRD_CHECK_ARG(K >= 1 && P >= 1, "%s: bad argument (K %d paths of at most P %d cells)", name, K, P);
  CRD_CHECK_ARG((long long)K * P < 0x40000000ll, "%s: bad argument (K * P = %lld cells are more than 2^30)", name, (long long)K * P);
  CRD_CHECK_ARG(starts && origin && togo && next && cells && n_cells && start_togo && status,
                "%s: null pointer (starts, origin, togo, next, cells, n_cells, start_togo, status)", name);
  CRD_CHECK_ARG(aligned_to(starts, 8) && aligned_to(origin, 8) && aligned_to(xy, 8) && aligned_to(path_map, 4) && aligned_to(togo, 4) &&
                    aligned_to(cells, 4) && aligned_to(n_cells, 4) && aligned_to(start_togo, 4) && aligned_to(status, 4),
                "%s: bad argument (starts, origin and xy must be 8-byte aligned, path_map, togo, cells, n_cells, start_togo and status 4-byte)",
                name);
  NavPaths a;
  a.starts = starts; a.path_map = path_map; a.K = K; a.P = P; a.M = M; a.nx = nx; a.ny = ny;
  a.origin = reinterpret_cast<const long long*>(origin); a.cell = from_bits(cell_f64_bits); a.togo = togo; a.next = next; a.cells = cells;
  a.xy = xy; a.n_cells = n_cells; a.start_togo = start_togo; a.status = status;
  hipLaunchKernelGGL(k_nav_paths, dim3(cdiv(K, CRD_WAVE)), dim3(CRD_WAVE), 0, as_stream(stream), a);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
