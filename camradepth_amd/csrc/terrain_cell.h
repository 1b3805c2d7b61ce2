// The per-cell rule of the terrain map (terrain_ops.hip, launches 4 and 5), plain integer C++ that compiles for the host as well:
// tests/terrain_cell_host.cpp runs it over every cell of the test cases (include/camradepth_hip.h, crd_terrain_update).
//   tc_fuse    this call's observation (lo, hi) of a cell into its slot (ground, top, weight): the running mean by floor division up
//              to w_max observations, an exponential filter of gain 1 / (w_max + 1) from there on
//   tc_derive  the nine grounds and weights around a cell (row-major 3 x 3, [4] the cell itself, [1] and [7] its neighbours along i,
//              [3] and [5] along j; weight 0: unknown) and its top -> step, slope2, state and hazard
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRD_TC_FN __host__ __device__ __forceinline__
#else
#define CRD_TC_FN inline
#endif

constexpr int TC_UNKNOWN = 0, TC_FREE = 1, TC_OCCUPIED = 2;               // occupancy's codes
constexpr int TC_NO_INFORMATION = 255, TC_LETHAL = 254, TC_FREE_MAX = 253;  // costmap_2d's

struct TcFused {
  int32_t ground, top, weight;
};

struct TcDerived {
  int32_t step;
  int64_t slope2;
  uint8_t state, hazard;
};

// Python's a // b for b > 0
CRD_TC_FN int64_t tc_floordiv(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// w: the slot's weight as it counts (0: never seen, left the window, or the map is new).  A slot of weight 0 holds ground = top = 0.
CRD_TC_FN TcFused tc_fuse(int32_t w, int32_t ground, int32_t top, bool observed, int32_t lo, int32_t hi, int32_t w_max) {
  TcFused r = {w ? ground : 0, w ? top : 0, w};
  if (!observed) return r;
  if (w == 0) {
    r.ground = lo;
    r.top = hi;
  } else {
    r.ground = (int32_t)tc_floordiv((int64_t)w * ground + lo, (int64_t)w + 1);
    r.top = (int32_t)tc_floordiv((int64_t)w * top + hi, (int64_t)w + 1);
  }
  r.weight = w + 1 < w_max ? w + 1 : w_max;
  return r;
}

// The gradient along one axis, in quanta over two cells: central where both neighbours are known, one-sided and doubled where one is
CRD_TC_FN int64_t tc_gradient(int64_t before, bool has_before, int64_t here, int64_t after, bool has_after) {
  if (has_before && has_after) return after - before;
  if (has_after) return 2 * (after - here);
  if (has_before) return 2 * (here - before);
  return 0;
}

CRD_TC_FN TcDerived tc_derive(const int32_t* g, const int32_t* w, int32_t top, int32_t step_max_q, int64_t slope2_max) {
  TcDerived r = {0, 0, (uint8_t)TC_UNKNOWN, (uint8_t)TC_NO_INFORMATION};
  if (w[4] == 0) return r;
  int64_t step = (int64_t)top - g[4];
  for (int k = 0; k < 9; ++k) {
    if (k == 4 || w[k] == 0) continue;
    const int64_t d = (int64_t)g[k] - g[4], a = d < 0 ? -d : d;
    step = a > step ? a : step;
  }
  const int64_t gx = tc_gradient(g[1], w[1] != 0, g[4], g[7], w[7] != 0), gy = tc_gradient(g[3], w[3] != 0, g[4], g[5], w[5] != 0);
  r.step = (int32_t)step;
  r.slope2 = gx * gx + gy * gy;
  if (step > step_max_q || r.slope2 > slope2_max) {
    r.state = (uint8_t)TC_OCCUPIED;
    r.hazard = (uint8_t)TC_LETHAL;
    return r;
  }
  const int64_t hs = tc_floordiv(step * TC_FREE_MAX, step_max_q), hl = tc_floordiv(r.slope2 * TC_FREE_MAX, slope2_max);
  r.state = (uint8_t)TC_FREE;
  r.hazard = (uint8_t)(hs > hl ? hs : hl);
  return r;
}
