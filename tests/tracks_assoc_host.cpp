// Host build of the association body of camradepth_amd/csrc/track_ops.hip (track_assoc.h) for tests/test_tracks_ref_cpu.py: the same
// ta_object_pick, ta_track_pick and ta_take over plain arrays, a round's phases run "thread" by "thread" in natural or in shuffled
// order, as the kernel runs them between its barriers.  Built by the test as a shared library (c++ -shared); with
// tests/tracks_assoc_main.cpp a stand-alone program, which is the form a sanitizer goes on.
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

#include "track_assoc.h"

namespace {

uint64_t next_random(uint64_t& s) {                                      // xorshift64
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  return s;
}

std::vector<int> order_of(int n, uint64_t& s, bool shuffled) {
  std::vector<int> v(n);
  std::iota(v.begin(), v.end(), 0);
  if (shuffled)
    for (std::size_t k = v.size(); k > 1; --k) std::swap(v[k - 1], v[next_random(s) % k]);
  return v;
}

}  // namespace

// px, py [T]: the predictions; live [T]: non-zero on a live slot.  zx, zy [N]: the centres; candidate [N]: non-zero on a candidate row
// (all of them below n).  seed 0: the threads of every phase in natural order; otherwise shuffled by it, anew for every phase.
// -> trk_obj [T], obj_trk [N] (TA_NOT, TA_OPEN or the partner), *rounds; returns the guard (1: left by the cap).
extern "C" int ta_associate(int T, int N, int n, const double* px, const double* py, const uint8_t* live, const double* zx, const double* zy,
                            const uint8_t* candidate, double gate2, int cap, uint64_t seed, int32_t* trk_obj, int32_t* obj_trk,
                            int32_t* rounds) {
  std::vector<int> obj_pick(N, TA_NONE), trk_pick(T, TA_NONE);
  for (int t = 0; t < T; ++t) trk_obj[t] = live[t] ? TA_OPEN : TA_NOT;
  for (int k = 0; k < N; ++k) obj_trk[k] = candidate[k] ? TA_OPEN : TA_NOT;
  uint64_t s = seed;
  int done = 0;
  bool any = true;
  while (done < cap) {
    for (int k : order_of(N, s, seed != 0)) ta_object_pick(k, T, zx, zy, px, py, gate2, trk_obj, obj_trk, obj_pick.data());
    for (int t : order_of(T, s, seed != 0)) ta_track_pick(t, n, zx, zy, px, py, gate2, trk_obj, obj_trk, trk_pick.data());
    any = false;
    for (int k : order_of(N, s, seed != 0)) any |= ta_take(k, obj_pick.data(), trk_pick.data(), trk_obj, obj_trk);
    ++done;
    if (!any) break;
  }
  *rounds = done;
  return any ? 1 : 0;
}
