// The association body of track_ops.hip, plain C++ that compiles for the host as well: tests/tracks_assoc_host.cpp runs it over the
// test cases with its "threads" in natural and in shuffled order.  Greedy assignment of object rows to track slots by ROUNDS of mutual
// best choices (include/camradepth_hip.h, crd_track_objects).  The state of a round, one entry per slot t and per row k:
//   trk_obj[t]   TA_NOT (the slot is free: it takes no part), TA_OPEN (live, not taken yet) or the row k that took it
//   obj_trk[k]   TA_NOT (the row is no candidate), TA_OPEN, or the slot t it took
//   obj_pick[k]  the choice of an open row in this round: TA_NONE (no open slot within the gate) or a slot;  trk_pick[t] likewise
// A round is three phases with a barrier behind each of the last two: ta_object_pick for every row and ta_track_pick for every slot
// (they read the state and write their own pick only), then ta_take for every row (it reads the picks and writes obj_trk[k] and, for
// the one row a slot picked back, trk_obj[t]).  So no phase has two writers of one word or a reader of a word written in that phase,
// and the order of the threads inside a phase changes nothing.
// Every open row and slot scans anew in every round.  Keeping a pick that is still open (the open set only shrinks, so it stays the
// least) gives the same bits and was measured: no gain, since a wave scans as long as one of its lanes does ("Object tracks").
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRD_TA_FN __host__ __device__ __forceinline__
#else
#define CRD_TA_FN inline
#endif

// each operation rounded to fp64 in the order written: no fused multiply-add, on the device or on the host
#pragma clang fp contract(off)
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

constexpr int TA_NOT = -2, TA_OPEN = -1;                                // trk_obj, obj_trk
constexpr int TA_NONE = -1;                                             // obj_pick, trk_pick

#if defined(__clang__)
#define CRD_TA_UNROLL _Pragma("unroll 8")
#else
#define CRD_TA_UNROLL
#endif

// the squared distance of a centre z and a prediction p
CRD_TA_FN double ta_d2(double zx, double zy, double px, double py) {
  const double dx = zx - px, dy = zy - py;
  return (dx * dx) + (dy * dy);
}

// Row k picks its least (d2, t) over the open slots with d2 <= gate2.  A NaN compares false: no candidate.
CRD_TA_FN void ta_object_pick(int k, int T, const double* zx, const double* zy, const double* px, const double* py, double gate2,
                              const int* trk_obj, const int* obj_trk, int* obj_pick) {
  if (obj_trk[k] != TA_OPEN) return;
  const double x = zx[k], y = zy[k];
  int best = TA_NONE;
  double best_d2 = 0.0;
  // Ascending t: a strict < keeps the lowest slot among equal d2.  No branch in the body, so that the loads of several slots are in
  // flight at once: with a branch on trk_obj[t] every step waited for two LDS round trips ("Object tracks").
  CRD_TA_UNROLL
  for (int t = 0; t < T; ++t) {
    const double d2 = ta_d2(x, y, px[t], py[t]);
    const bool better = (trk_obj[t] == TA_OPEN) & (d2 <= gate2) & ((best == TA_NONE) | (d2 < best_d2));
    best = better ? t : best;
    best_d2 = better ? d2 : best_d2;
  }
  obj_pick[k] = best;
}

// Slot t picks its least (d2, k) over the open rows k < n with d2 <= gate2.
CRD_TA_FN void ta_track_pick(int t, int n, const double* zx, const double* zy, const double* px, const double* py, double gate2,
                             const int* trk_obj, const int* obj_trk, int* trk_pick) {
  if (trk_obj[t] != TA_OPEN) return;
  const double x = px[t], y = py[t];
  int best = TA_NONE;
  double best_d2 = 0.0;
  CRD_TA_UNROLL
  for (int k = 0; k < n; ++k) {
    const double d2 = ta_d2(zx[k], zy[k], x, y);
    const bool better = (obj_trk[k] == TA_OPEN) & (d2 <= gate2) & ((best == TA_NONE) | (d2 < best_d2));
    best = better ? k : best;
    best_d2 = better ? d2 : best_d2;
  }
  trk_pick[t] = best;
}

// Row k takes the slot it picked when the slot picked it back.  -> whether it did.
CRD_TA_FN bool ta_take(int k, const int* obj_pick, const int* trk_pick, int* trk_obj, int* obj_trk) {
  if (obj_trk[k] != TA_OPEN) return false;
  const int t = obj_pick[k];
  if (t < 0 || trk_pick[t] != k) return false;
  obj_trk[k] = t;
  trk_obj[t] = k;
  return true;
}
