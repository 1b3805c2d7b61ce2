// Map objects on the device: a state map (occupancy_ops.hip's `state`, or any uint8 map) -> the connected sets of its source cells,
// numbered in the order of their first cells, a label per cell and a table of count, box, edge flag, coordinate sums and centre per
// object (include/camradepth_hip.h, crd_map_objects).  Connected-component labelling by union-find (object_uf.h): inside tiles in LDS,
// then across the tile borders on the global parent table, which is `label` itself.  Eight launches, whatever the map holds:
//   0 k_obj_init     info, the table, sums and centre to their unused values
//   1 k_obj_tile     labels a tile of 16 x 64 cells in LDS: row runs from ballots of the source bits, unions between neighbouring rows,
//                    every cell to its tile root; parent = the root's window index, -1 on a non-source cell; count = the cells of
//                    the tile's piece at its root, 0 elsewhere
//   2 k_obj_merge    one thread per cell next to a tile border: union with its neighbours across the border, corners included with
//                    8-connectivity.  The only launch in which workgroups write what others read: every access to the parent table
//                    is an agent-scope atomic (relaxed load, atomic min), and nothing is concluded from it before the next launch
//   3 k_obj_flatten  every cell to its root (the object's first cell), roots into the workspace; count[root] += the count of every
//                    tile piece that is not the root's own: one atomic per piece
//   4 k_obj_count    per chunk of cells the roots that are kept (count >= min_cells); the small ones into info
//   5 k_obj_number   per chunk: the kept roots of the chunks before it (a sum over at most 1024 counts), then a ballot scan inside the
//                    chunk: the number of every kept root in index order, the table row of those below max_objects
//   6 k_obj_fill     label from the root's number; box, edge flag and sums by integer atomic min / max / or / add: runs of equal
//                    labels among the lanes of a wave folded first, then the runs of a tile per object in LDS, so the row of an
//                    object that covers the map gets seven atomics per tile
//   7 k_obj_centre   the centres from the finished sums (left out with centre == NULL)
// Every output is a function of the partition into objects alone, and only integer atomics touch memory, so the bits are the same
// every run although the parent table between launches 2 and 3 depends on timing.  No workgroup waits for another; every device loop
// is capped (object_uf.h) and a loop that reaches its cap raises info's guard.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_obj_tile 44 VGPRs, 8320 bytes of LDS; k_obj_fill 33 VGPRs,
// 28672 bytes of LDS (five workgroups to a CU); the others 18 to 38 VGPRs, k_obj_count and k_obj_number 16 bytes of LDS.  No scratch.
#include "raster.h"       // aligned16
#include "object_uf.h"
#include <string.h>

// the centre is specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256, WAVES = TPB / CRD_WAVE;
constexpr int TILE_H = 16, TILE_W = CRD_WAVE;                           // rows and columns of a tile of launch 1
constexpr int TILE_CELLS = TILE_H * TILE_W;
constexpr int SLOTS = 1024;                                             // of launch 6's LDS table: twice the runs a tile can hold
constexpr int MAX_CHUNKS = 1024;                                        // of one map in launches 4 and 5
constexpr int NOT_SOURCE = (int)0x80000000;                             // the workspace's root of a non-source cell
constexpr int CODE_OVERFLOW = -70000, CODE_SMALL = -70001;              // a root's entry after launch 5; -(k + 1) for table row k < 65536
constexpr int INT_MAX_ = 0x7fffffff;

struct Obj {
  const unsigned char* state;
  int M, nx, ny, sources, conn8, min_cells, N;
  int n;                                                                // nx * ny
  const long long* origin;
  double cell;
  int32_t *root, *count;                                                // the workspace: int32 [M][n] each
  int32_t *label, *objects, *info;
  long long* sums;
  double* centre;                                                       // may be NULL
};

__device__ __forceinline__ void raise_guard(const Obj& a, int m) {
  __hip_atomic_fetch_or(a.info + m * 4 + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the parent table of a tile in LDS
struct LdsTable {
  int* p;
  __device__ __forceinline__ int load(int x) { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int fetch_min(int x, int v) {
    return __hip_atomic_fetch_min(p + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

// the parent table of one map in memory, as launch 2 sees it
struct AgentTable {
  int32_t* p;
  __device__ __forceinline__ int load(int x) { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int fetch_min(int x, int v) {
    return __hip_atomic_fetch_min(p + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// a parent table that no one writes any more (launch 3)
struct ReadTable {
  const int32_t* p;
  __device__ __forceinline__ int load(int x) { return p[x]; }
};

// Launch 0.  rows = M * N table rows, then the M rows of info.
__global__ __launch_bounds__(TPB) void k_obj_init(Obj a, long long rows) {
  for (long long t = (long long)blockIdx.x * TPB + threadIdx.x; t < rows + a.M; t += (long long)gridDim.x * TPB) {
    if (t >= rows) {
      int32_t* o = a.info + (t - rows) * 4;
      o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0;
      continue;
    }
    int32_t* o = a.objects + t * 8;
    o[0] = -1; o[1] = 0; o[2] = -1; o[3] = -1; o[4] = -1; o[5] = -1; o[6] = 0; o[7] = 0;
    a.sums[t * 2] = 0; a.sums[t * 2 + 1] = 0;
    if (a.centre) {
      a.centre[t * 2] = __longlong_as_double(0x7ff8000000000000ll);
      a.centre[t * 2 + 1] = __longlong_as_double(0x7ff8000000000000ll);
    }
  }
}

// Launch 1: a workgroup takes a tile, a wave every fourth row of it, the lanes along j.  par[r * 64 + lane] starts as the first cell of
// the lane's run of sources in its row (the bit above the highest 0 below the lane), so a row is labelled without a union; a cell
// is then joined with the row above only where that adds something: straight up unless the pair to its left is joined already,
// diagonally only when neither cell between the two is a source.
__global__ __launch_bounds__(TPB) void k_obj_tile(Obj a, int row_tiles, int col_tiles, long long n_tiles) {
  __shared__ int par[TILE_CELLS], cnt[TILE_CELLS];
  __shared__ unsigned long long bits[TILE_H];
  const int lane = threadIdx.x & (CRD_WAVE - 1), wave = threadIdx.x >> 6;
  LdsTable t{par};
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tj = (int)(tile % col_tiles);
    const long long rest = tile / col_tiles;
    const int ti = (int)(rest % row_tiles), m = (int)(rest / row_tiles);
    const int i0 = ti * TILE_H, j = tj * TILE_W + lane;
    const long long map0 = (long long)m * a.n;
    for (int r = wave; r < TILE_H; r += WAVES) {
      const int i = i0 + r;
      bool src = false;
      if (i < a.nx && j < a.ny) {
        const int v = a.state[map0 + (long long)i * a.ny + j];
        src = v < 8 && ((a.sources >> v) & 1);
      }
      const unsigned long long word = __ballot(src);
      if (lane == 0) bits[r] = word;
      const unsigned long long zeros_below = ~word & ((1ull << lane) - 1ull);
      const int start = zeros_below ? CRD_WAVE - __clzll((long long)zeros_below) : 0;
      par[r * TILE_W + lane] = src ? r * TILE_W + start : -1;
      cnt[r * TILE_W + lane] = 0;
    }
    __syncthreads();
    bool capped = false;
    for (int r = wave; r < TILE_H; r += WAVES) {
      if (r == 0) continue;
      const unsigned long long cur = bits[r], up = bits[r - 1];
      if (!((cur >> lane) & 1ull)) continue;
      const int li = r * TILE_W + lane;
      const bool u0 = (up >> lane) & 1ull;
      const bool ul = lane > 0 && ((up >> (lane - 1)) & 1ull), ur = lane < CRD_WAVE - 1 && ((up >> (lane + 1)) & 1ull);
      const bool cl = lane > 0 && ((cur >> (lane - 1)) & 1ull), cr = lane < CRD_WAVE - 1 && ((cur >> (lane + 1)) & 1ull);
      if (u0 && !(ul && cl)) uf_union(t, li, li - TILE_W, TILE_CELLS, capped);
      if (a.conn8 && !u0) {
        if (ul && !cl) uf_union(t, li, li - TILE_W - 1, TILE_CELLS, capped);
        if (ur && !cr) uf_union(t, li, li - TILE_W + 1, TILE_CELLS, capped);
      }
    }
    __syncthreads();
    int roots[TILE_H / WAVES];                                          // of this lane's cell in each of the wave's rows, -1 on a non-source
#pragma unroll
    for (int k = 0; k < TILE_H / WAVES; ++k) {
      const int r = wave + k * WAVES;
      const unsigned long long word = bits[r];
      roots[k] = -1;
      if (!((word >> lane) & 1ull)) continue;
      roots[k] = uf_find(t, r * TILE_W + lane, TILE_CELLS, capped);
      if (lane > 0 && ((word >> (lane - 1)) & 1ull)) continue;           // the first cell of a run adds the run's length
      const unsigned long long above = ~(word >> lane);                 // 0 only for a full row seen from lane 0
      atomicAdd(&cnt[roots[k]], above ? __ffsll((long long)above) - 1 : CRD_WAVE);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TILE_H / WAVES; ++k) {
      const int r = wave + k * WAVES, i = i0 + r;
      if (i >= a.nx || j >= a.ny) continue;
      const long long idx = map0 + (long long)i * a.ny + j;
      const int root = roots[k];
      a.label[idx] = root < 0 ? -1 : (i0 + root / TILE_W) * a.ny + tj * TILE_W + root % TILE_W;
      a.count[idx] = root < 0 ? 0 : cnt[r * TILE_W + lane];             // the cells of the tile's piece at its root, 0 elsewhere
    }
    if (capped) raise_guard(a, m);
    __syncthreads();                                                    // par, cnt and bits are written again by the next tile
  }
}

// Launch 2.  Per map h_items = (row_tiles - 1) * ny cells (i = k * 16, j) under a horizontal border, joined with (i - 1, j) and, with
// 8-connectivity, (i - 1, j - 1) and (i - 1, j + 1); then (col_tiles - 1) * nx cells (i, j = k * 64) right of a vertical border, joined
// with (i, j - 1) and, with 8-connectivity, (i - 1, j - 1) and (i + 1, j - 1).  Every pair of neighbours in different tiles is among
// these, the two diagonals through a point where four tiles meet included; a pair named twice is joined twice, which changes nothing.
__global__ __launch_bounds__(TPB) void k_obj_merge(Obj a, int h_items, int per_map, long long items) {
  for (long long w = (long long)blockIdx.x * TPB + threadIdx.x; w < items; w += (long long)gridDim.x * TPB) {
    const int m = (int)(w / per_map), q = (int)(w - (long long)m * per_map);
    AgentTable t{a.label + (long long)m * a.n};
    int i, j, ni[3], nj[3];
    if (q < h_items) {
      i = (q / a.ny + 1) * TILE_H; j = q % a.ny;
      ni[0] = i - 1; nj[0] = j; ni[1] = i - 1; nj[1] = j - 1; ni[2] = i - 1; nj[2] = j + 1;
    } else {
      const int v = q - h_items;
      j = (v / a.nx + 1) * TILE_W; i = v % a.nx;
      ni[0] = i; nj[0] = j - 1; ni[1] = i - 1; nj[1] = j - 1; ni[2] = i + 1; nj[2] = j - 1;
    }
    if (i >= a.nx || j >= a.ny) continue;                                // never: the borders lie inside the window
    const int c = i * a.ny + j;
    if (t.load(c) < 0) continue;
    bool capped = false;
    const int n_nb = a.conn8 ? 3 : 1;
    for (int k = 0; k < n_nb; ++k) {
      if (ni[k] < 0 || ni[k] >= a.nx || nj[k] < 0 || nj[k] >= a.ny) continue;
      const int d = ni[k] * a.ny + nj[k];
      if (t.load(d) < 0) continue;
      uf_union(t, c, d, a.n, capped);
    }
    if (capped) raise_guard(a, m);
  }
}

// The lanes of a wave hold 64 consecutive cells of one row; v is -1 or a value that cells of one object share.  -> true on the first
// lane of every run of equal v >= 0, with the run's length.
__device__ __forceinline__ bool run_head(int v, int lane, int& len) {
  const int before = __shfl_up(v, 1);
  const bool first = lane == 0 || before != v;
  const unsigned long long heads = __ballot(first);
  const unsigned long long later = lane == CRD_WAVE - 1 ? 0ull : heads >> (lane + 1);
  len = (later ? lane + __ffsll((long long)later) : CRD_WAVE) - lane;
  return first && v >= 0;
}

// Launch 3: a thread per cell.  The parent table is final, so plain loads; the roots go to the workspace.  count is non-zero at the
// root of a tile's piece alone (launch 1): a piece whose root is not the object's adds its cells to the object's root, one atomic per
// piece, not per cell.  Only an object's root is added to and only the others are read, so no read meets an add.
__global__ __launch_bounds__(TPB) void k_obj_flatten(Obj a, long long n_cells) {
  for (long long idx = (long long)blockIdx.x * TPB + threadIdx.x; idx < n_cells; idx += (long long)gridDim.x * TPB) {
    const int m = (int)(idx / a.n), c = (int)(idx - (long long)m * a.n);
    const long long map0 = (long long)m * a.n;
    ReadTable t{a.label + map0};
    bool capped = false;
    if (a.label[idx] < 0) {
      a.root[idx] = NOT_SOURCE;
      continue;
    }
    const int root = uf_find(t, c, a.n, capped);
    a.root[idx] = root;
    if (root != c) {
      const int piece = a.count[idx];
      if (piece > 0) __hip_atomic_fetch_add(a.count + map0 + root, piece, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (capped) raise_guard(a, m);
  }
}

// the sum of v over the workgroup, in every thread; red holds WAVES ints
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
  for (int d = CRD_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();                                                      // red may still be read from the call before
  if ((threadIdx.x & (CRD_WAVE - 1)) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) s += red[k];
  return s;
}

// Launch 4: a workgroup takes a chunk of `chunk` cells of one map.  The kept roots of the chunk go to label at the chunk's first cell:
// the parent table is not needed any more and launch 6 writes label in full.
__global__ __launch_bounds__(TPB) void k_obj_count(Obj a, int chunk, int chunks, long long n_items) {
  __shared__ int red[WAVES];
  for (long long w = blockIdx.x; w < n_items; w += gridDim.x) {
    const int m = (int)(w / chunks), k = (int)(w - (long long)m * chunks);
    const long long map0 = (long long)m * a.n;
    const int c0 = k * chunk, c1 = (long long)c0 + chunk < a.n ? c0 + chunk : a.n;
    int kept = 0, small = 0;
    for (long long c = c0 + threadIdx.x; c < c1; c += TPB) {                // 64 bits: c1 + 255 may pass 2^31
      if (a.root[map0 + c] != (int)c) continue;
      if (a.count[map0 + c] >= a.min_cells) ++kept; else ++small;
    }
    kept = block_sum(kept, red);
    small = block_sum(small, red);
    if (threadIdx.x == 0) {
      a.label[map0 + c0] = kept;
      if (small) __hip_atomic_fetch_add(a.info + m * 4 + 2, small, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Launch 5: the same chunks.  A root's entry in the workspace becomes its code: -(number + 1) with a table row, CODE_OVERFLOW,
// CODE_SMALL.  No other workgroup reads or writes the roots of this chunk in this launch.
__global__ __launch_bounds__(TPB) void k_obj_number(Obj a, int chunk, int chunks, long long n_items) {
  __shared__ int red[WAVES];
  const int lane = threadIdx.x & (CRD_WAVE - 1), wave = threadIdx.x >> 6;
  for (long long w = blockIdx.x; w < n_items; w += gridDim.x) {
    const int m = (int)(w / chunks), k = (int)(w - (long long)m * chunks);
    const long long map0 = (long long)m * a.n;
    int before = 0;
    for (int q = threadIdx.x; q < k; q += TPB) before += a.label[map0 + (long long)q * chunk];
    int next = block_sum(before, red);                                  // the number of this chunk's first kept root
    const int c0 = k * chunk, c1 = (long long)c0 + chunk < a.n ? c0 + chunk : a.n;
    for (long long base = c0; base < c1; base += TPB) {                 // the same trip count in every thread
      const long long c = base + threadIdx.x;
      bool is_root = false, kept = false;
      int cells = 0;
      if (c < c1 && a.root[map0 + c] == (int)c) {
        is_root = true;
        cells = a.count[map0 + c];
        kept = cells >= a.min_cells;
      }
      const unsigned long long word = __ballot(kept);
      __syncthreads();
      if (lane == 0) red[wave] = __popcll(word);
      __syncthreads();
      int number = next + __popcll(word & ((1ull << lane) - 1ull));
      int total = 0;
#pragma unroll
      for (int q = 0; q < WAVES; ++q) {
        if (q < wave) number += red[q];
        total += red[q];
      }
      next += total;
      if (!is_root) continue;
      int code = CODE_SMALL;
      if (kept) {
        code = CODE_OVERFLOW;
        if (number < a.N) {
          code = -(number + 1);
          int32_t* o = a.objects + ((long long)m * a.N + number) * 8;
          o[0] = (int)c; o[1] = cells; o[2] = INT_MAX_; o[3] = -1; o[4] = INT_MAX_; o[5] = -1;      // box: launch 6's atomics
        }
      }
      a.root[map0 + c] = code;
    }
    if (k == chunks - 1 && threadIdx.x == 0) {                          // next: all kept objects of the map
      a.info[m * 4] = next < a.N ? next : a.N;
      a.info[m * 4 + 1] = next < a.N ? 0 : next - a.N;
    }
  }
}

// Launch 6: a workgroup takes a tile of launch 1's tiling, a wave every fourth row of it.  A run of equal labels among the lanes is a
// piece of one row of one object; its first lane finds the object's slot in an LDS table keyed by the label (open addressing from
// label % SLOTS: a tile holds at most 512 runs, the table 1024 slots, and the labels of a tile are mostly consecutive numbers) and
// folds the run into the slot with LDS atomics.  After the tile every slot in use goes to the object's row with one atomic per column
// and is cleared.  So an object that covers the map costs seven atomics per tile, not per run: its row is one hot address.
__global__ __launch_bounds__(TPB) void k_obj_fill(Obj a, int row_tiles, int col_tiles, long long n_tiles) {
  __shared__ int key[SLOTS], lo_i[SLOTS], hi_i[SLOTS], lo_j[SLOTS], hi_j[SLOTS], sum_i[SLOTS], sum_j[SLOTS];
  const int lane = threadIdx.x & (CRD_WAVE - 1), wave = threadIdx.x >> 6;
  for (int q = threadIdx.x; q < SLOTS; q += TPB) {
    key[q] = -1; lo_i[q] = INT_MAX_; hi_i[q] = -1; lo_j[q] = INT_MAX_; hi_j[q] = -1; sum_i[q] = 0; sum_j[q] = 0;
  }
  __syncthreads();
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tj = (int)(tile % col_tiles);
    const long long rest = tile / col_tiles;
    const int ti = (int)(rest % row_tiles), m = (int)(rest / row_tiles);
    const int j = tj * TILE_W + lane;
    const long long map0 = (long long)m * a.n;
    bool capped = false;
    for (int r = wave; r < TILE_H; r += WAVES) {                        // the same trip count in every lane: run_head is a wave operation
      const int i = ti * TILE_H + r;
      int lab = -1;
      if (i < a.nx && j < a.ny) {
        const long long idx = map0 + (long long)i * a.ny + j;
        int code = a.root[idx];
        if (code != NOT_SOURCE) {
          if (code >= 0) code = a.root[map0 + code];                    // the root's code
          if (code == CODE_SMALL) lab = -2;
          else if (code == CODE_OVERFLOW) lab = -3;
          else if (code < 0 && code >= -a.N) lab = -(code + 1);
          else { lab = -3; capped = true; }                             // never: every root was given a code
        }
        a.label[idx] = lab;
      }
      int len;
      if (!run_head(lab, lane, len)) continue;
      int slot = lab & (SLOTS - 1), probe = 0;
      for (; probe < SLOTS; ++probe) {
        const int old = atomicCAS(&key[slot], -1, lab);
        if (old == -1 || old == lab) break;
        slot = (slot + 1) & (SLOTS - 1);
      }
      if (probe == SLOTS) { capped = true; continue; }                  // never: fewer runs than slots
      atomicMin(&lo_i[slot], i); atomicMax(&hi_i[slot], i);
      atomicMin(&lo_j[slot], j); atomicMax(&hi_j[slot], j + len - 1);
      atomicAdd(&sum_i[slot], i * len);                                 // over a tile's 1024 cells at most: below 65535 * 1024 < 2^31
      atomicAdd(&sum_j[slot], j * len + len * (len - 1) / 2);
    }
    if (capped) raise_guard(a, m);
    __syncthreads();
    for (int q = threadIdx.x; q < SLOTS; q += TPB) {
      const int lab = key[q];
      if (lab < 0) continue;
      const int i_lo = lo_i[q], i_hi = hi_i[q], j_lo = lo_j[q], j_hi = hi_j[q];
      int32_t* o = a.objects + ((long long)m * a.N + lab) * 8;
      unsigned long long* s = reinterpret_cast<unsigned long long*>(a.sums) + ((long long)m * a.N + lab) * 2;
      __hip_atomic_fetch_min(o + 2, i_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(o + 3, i_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_min(o + 4, j_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(o + 5, j_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (i_lo == 0 || i_hi == a.nx - 1 || j_lo == 0 || j_hi == a.ny - 1)
        __hip_atomic_fetch_or(o + 6, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(s, (unsigned long long)sum_i[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(s + 1, (unsigned long long)sum_j[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      key[q] = -1; lo_i[q] = INT_MAX_; hi_i[q] = -1; lo_j[q] = INT_MAX_; hi_j[q] = -1; sum_i[q] = 0; sum_j[q] = 0;
    }
    __syncthreads();
  }
}

// Launch 7: one thread per table row in use.
__global__ __launch_bounds__(TPB) void k_obj_centre(Obj a, long long rows) {
  for (long long t = (long long)blockIdx.x * TPB + threadIdx.x; t < rows; t += (long long)gridDim.x * TPB) {
    const int m = (int)(t / a.N), k = (int)(t - (long long)m * a.N);
    if (k >= a.info[m * 4]) continue;
    const double cells = (double)a.objects[t * 8 + 1];
    const double mi = (double)a.sums[t * 2] / cells, mj = (double)a.sums[t * 2 + 1] / cells;
    a.centre[t * 2] = (((double)a.origin[m * 2] + mi) + 0.5) * a.cell;
    a.centre[t * 2 + 1] = (((double)a.origin[m * 2 + 1] + mj) + 0.5) * a.cell;
  }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf
inline unsigned grid_of(long long items) { return (unsigned)(items < 1 ? 1 : (items < 65536 ? items : 65536)); }

}  // namespace

extern "C" int crd_map_objects(const uint8_t* state, int32_t M, int32_t nx, int32_t ny, int32_t sources, int32_t connectivity,
                               int32_t min_cells, int32_t max_objects, const int64_t* origin, uint64_t cell_f64_bits, void* workspace,
                               int64_t workspace_bytes, int32_t* label, int32_t* objects, int64_t* sums, double* centre, int32_t* info,
                               crd_stream_t stream) {
  const char* name = "crd_map_objects";
  CRD_CHECK_ARG(M >= 1, "%s: bad argument (M %d maps)", name, M);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  const long long n_cells = (long long)M * nx * ny;
  CRD_CHECK_ARG(n_cells < 0x80000000ll, "%s: bad argument (M * nx * ny = %lld cells are more than the 32-bit indices hold)", name, n_cells);
  CRD_CHECK_ARG(sources >= 1 && sources <= 255, "%s: bad argument (sources %d is not a mask of the states 0 .. 7, 1 .. 255)", name, sources);
  CRD_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: bad argument (connectivity %d is neither 4 nor 8)", name, connectivity);
  CRD_CHECK_ARG(min_cells >= 1, "%s: bad argument (min_cells %d is below 1)", name, min_cells);
  CRD_CHECK_ARG(max_objects >= 1 && max_objects <= 65535, "%s: bad argument (max_objects %d is not in 1 .. 65535)", name, max_objects);
  const double cell = from_bits(cell_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(state && origin && workspace && label && objects && sums && info,
                "%s: null pointer (state, origin, workspace, label, objects, sums, info)", name);
  const long long need = (8 * n_cells + 15) & ~15ll;
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  CRD_CHECK_ARG(aligned_to(label, 4) && aligned_to(objects, 4) && aligned_to(info, 4) && aligned_to(sums, 8) && aligned_to(centre, 8) &&
                    aligned_to(origin, 8),
                "%s: bad argument (label, objects and info must be 4-byte aligned, sums, centre and origin 8-byte)", name);
  Obj a;
  a.state = state; a.M = M; a.nx = nx; a.ny = ny; a.sources = sources; a.conn8 = connectivity == 8; a.min_cells = min_cells; a.N = max_objects;
  a.n = nx * ny; a.origin = reinterpret_cast<const long long*>(origin); a.cell = cell;
  a.root = reinterpret_cast<int32_t*>(workspace); a.count = a.root + n_cells;
  a.label = label; a.objects = objects; a.info = info; a.sums = reinterpret_cast<long long*>(sums); a.centre = centre;
  hipStream_t st = as_stream(stream);
  const long long rows = (long long)M * max_objects;
  hipLaunchKernelGGL(k_obj_init, dim3(grid_of((rows + M + TPB - 1) / TPB)), dim3(TPB), 0, st, a, rows);
  const int row_tiles = cdiv(nx, TILE_H), col_tiles = cdiv(ny, TILE_W);
  const long long n_tiles = (long long)M * row_tiles * col_tiles;
  hipLaunchKernelGGL(k_obj_tile, dim3(grid_of(n_tiles)), dim3(TPB), 0, st, a, row_tiles, col_tiles, n_tiles);
  const int h_items = (row_tiles - 1) * ny, per_map = h_items + (col_tiles - 1) * nx;      // below 2 * nx * ny / 16
  const long long items = (long long)M * per_map;
  hipLaunchKernelGGL(k_obj_merge, dim3(grid_of((items + TPB - 1) / TPB)), dim3(TPB), 0, st, a, h_items, per_map < 1 ? 1 : per_map, items);
  hipLaunchKernelGGL(k_obj_flatten, dim3(grid_of((n_cells + TPB - 1) / TPB)), dim3(TPB), 0, st, a, n_cells);
  const int chunk = TPB * cdiv(cdiv(a.n, MAX_CHUNKS), TPB), chunks = cdiv(a.n, chunk);
  const long long chunk_items = (long long)M * chunks;
  hipLaunchKernelGGL(k_obj_count, dim3(grid_of(chunk_items)), dim3(TPB), 0, st, a, chunk, chunks, chunk_items);
  hipLaunchKernelGGL(k_obj_number, dim3(grid_of(chunk_items)), dim3(TPB), 0, st, a, chunk, chunks, chunk_items);
  hipLaunchKernelGGL(k_obj_fill, dim3(grid_of(n_tiles)), dim3(TPB), 0, st, a, row_tiles, col_tiles, n_tiles);
  if (centre) hipLaunchKernelGGL(k_obj_centre, dim3(grid_of((rows + TPB - 1) / TPB)), dim3(TPB), 0, st, a, rows);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
