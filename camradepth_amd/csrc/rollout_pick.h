// The score and the pick's comparison of rollout_ops.hip, plain C++ that compiles for the host as well: tests/rollout_pick_host.cpp
// runs both over records in natural and in shuffled order (include/camradepth_hip.h, crd_plan_rollouts).
//   rp_score   the int64 score of candidate k = iv * n_w + iw from its integers, each weight multiplying its own term
//   rp_better  the strict total order of the candidates of one map: a valid one before an invalid one; among valid ones the least
//              score, then the least |iw - c|, then the larger iv, then the least k; invalid ones by k.  A total order has one least
//              element, so a reduction by it gives the same pick in every grouping and order.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRD_RP_FN __host__ __device__ __forceinline__
#else
#define CRD_RP_FN inline
#endif

constexpr int RP_MAX_V = 64, RP_MAX_W = 129, RP_MAX_K = 4096, RP_MAX_P = 256, RP_MAX_T = 1024, RP_MAX_WEIGHT = 32767;
constexpr int RP_UNREACHED = 0x7fffffff;                                       // crd_nav_field's
constexpr int RP_NOT_FINITE = 1, RP_NO_CANDIDATE = 2;                          // the status bits
constexpr int RP_ADMISSIBLE = 1, RP_CLEAR_STATIC = 2, RP_CLEAR = 4, RP_VALID = 8;      // the flags of a record

// One candidate's record, 32 bytes: what launch 1 writes and launch 2 reads
struct RpRecord {
  long long score;
  int32_t first_blocked, first_track, max_cost, end_togo, sum_cost, flags;
};

struct RpWeights {
  int togo, max_cost, sum_cost, slow, turn;                                    // each 0 .. 32767
};

struct RpCandidate {
  long long score;
  int k, valid, turn, iv;                                                      // |iw - c| and iv of k, divided out once
};

CRD_RP_FN int rp_turn(int k, int n_w) {
  const int iw = k % n_w, c = (n_w - 1) / 2;
  return iw < c ? c - iw : iw - c;
}

// has_togo: a cost-to-go was given; without one its term is left out whatever end_togo holds.  Every term is below 2^47.
CRD_RP_FN long long rp_score(const RpWeights& w, int has_togo, int end_togo, int max_cost, int sum_cost, int k, int n_v, int n_w) {
  const int iv = k / n_w;
  long long s = has_togo ? (long long)w.togo * end_togo : 0ll;
  s += (long long)w.max_cost * max_cost;
  s += (long long)w.sum_cost * sum_cost;
  s += (long long)w.slow * (n_v - 1 - iv);
  s += (long long)w.turn * rp_turn(k, n_w);
  return s;
}

CRD_RP_FN bool rp_better(const RpCandidate& a, const RpCandidate& b) {
  if (a.valid != b.valid) return a.valid > b.valid;
  if (a.valid) {
    if (a.score != b.score) return a.score < b.score;
    if (a.turn != b.turn) return a.turn < b.turn;
    if (a.iv != b.iv) return a.iv > b.iv;
  }
  return a.k < b.k;
}

CRD_RP_FN RpCandidate rp_at(const RpRecord* records, int k, int n_w) {
  RpCandidate c;
  c.score = records[k].score; c.k = k; c.valid = (records[k].flags & RP_VALID) ? 1 : 0; c.turn = rp_turn(k, n_w); c.iv = k / n_w;
  return c;
}
