// The pick's comparison and the pose composition of match_ops.hip, plain C++ that compiles for the host as well:
// tests/match_pick_host.cpp runs both over the test cases, the candidates in natural and in shuffled order
// (include/camradepth_hip.h, crd_match_scan).
//   mp_better     the strict total order of the candidates (t, dx, dy) of one map: a larger score first; among equals the least
//                 dx * dx + dy * dy, then the least |t - n_theta|, then the least t, dx, dy.  A total order has one least element, so a
//                 reduction by it gives the same pick in every grouping and order.
//   mp_candidate  T'[t]: the pose T turned by (c, s) about the vertical axis of the map frame through S; the centre copies T
//   mp_shifted    T'[t*] moved by whole cells
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRD_MP_FN __host__ __device__ __forceinline__
#else
#define CRD_MP_FN inline
#endif

// each operation rounded to fp64 in the order written: no fused multiply-add, on the device or on the host
#pragma clang fp contract(off)
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

constexpr int MP_MAX_XY = 16, MP_MAX_THETA = 32;
constexpr int MP_UNINITIALISED = 1, MP_NOT_FINITE = 2, MP_FEW_CELLS = 4, MP_LOW_SCORE = 8, MP_ON_BORDER = 16;      // the status bits
constexpr int MP_KEEPS_PRIOR = MP_UNINITIALISED | MP_NOT_FINITE | MP_FEW_CELLS | MP_LOW_SCORE;

// t in 0 .. 2 * n_theta; dx, dy in -n_xy .. n_xy
struct MpCandidate {
  long long score;
  int t, dx, dy;
};

CRD_MP_FN bool mp_better(const MpCandidate& a, const MpCandidate& b, int n_theta) {
  if (a.score != b.score) return a.score > b.score;
  const int ra = a.dx * a.dx + a.dy * a.dy, rb = b.dx * b.dx + b.dy * b.dy;
  if (ra != rb) return ra < rb;
  const int ta = a.t < n_theta ? n_theta - a.t : a.t - n_theta, tb = b.t < n_theta ? n_theta - b.t : b.t - n_theta;
  if (ta != tb) return ta < tb;
  if (a.t != b.t) return a.t < b.t;
  if (a.dx != b.dx) return a.dx < b.dx;
  return a.dy < b.dy;
}

// The candidate of flat index i in the [2 * n_theta + 1][2 * n_xy + 1][2 * n_xy + 1] table
CRD_MP_FN MpCandidate mp_at(const long long* table, int i, int n_xy) {
  const int ns = 2 * n_xy + 1, t = i / (ns * ns), rem = i - t * ns * ns, ix = rem / ns;
  MpCandidate c;
  c.score = table[i]; c.t = t; c.dx = ix - n_xy; c.dy = rem - ix * ns - n_xy;
  return c;
}

CRD_MP_FN bool mp_on_border(const MpCandidate& c, int n_xy, int n_theta) {
  const int ax = c.dx < 0 ? -c.dx : c.dx, ay = c.dy < 0 ? -c.dy : c.dy, at = c.t < n_theta ? n_theta - c.t : c.t - n_theta;
  return (n_xy > 0 && (ax == n_xy || ay == n_xy)) || (n_theta > 0 && at == n_theta);
}

// T, out: row-major [3][4].  S: the point the turn goes through (its x and y are read).
CRD_MP_FN void mp_candidate(const double* T, const double* S, double c, double s, bool centre, double* out) {
  for (int k = 0; k < 12; ++k) out[k] = T[k];
  if (centre) return;
  for (int k = 0; k < 3; ++k) {
    out[k] = c * T[k] - s * T[4 + k];
    out[4 + k] = s * T[k] + c * T[4 + k];
  }
  out[3] = (c * T[3] - s * T[7]) + (S[0] - (c * S[0] - s * S[1]));
  out[7] = (s * T[3] + c * T[7]) + (S[1] - (s * S[0] + c * S[1]));
}

// Entry k of the row-major T'[t*] moved by (dx, dy) cells: the two translations take the shift, the rest is copied
CRD_MP_FN double mp_shifted_at(const double* Tc, int k, int dx, int dy, double cell) {
  if (k == 3) return Tc[3] + (double)dx * cell;
  if (k == 7) return Tc[7] + (double)dy * cell;
  return Tc[k];
}

CRD_MP_FN void mp_shifted(const double* Tc, int dx, int dy, double cell, double* out) {
  for (int k = 0; k < 12; ++k) out[k] = mp_shifted_at(Tc, k, dx, dy, cell);
}
