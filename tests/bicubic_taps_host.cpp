// Host build of camradepth_amd/csrc/bicubic_taps.h for tests/test_bicubic_taps_cpu.py: the 2n x n forward matrix of the bicubic x2
// from the forward taps, and the checks of the transpose's folded weights against its columns.  Built by the test as a shared library
// (c++ -shared) and, with the main below, as a stand-alone program, which is the form a sanitizer goes on.  Every value is a
// multiple of 1/256, so the comparisons are equalities.
#include <cstdio>
#include <vector>

#include "bicubic_taps.h"

// F [2n][n], row-major: F[o][i] = the sum, in tap order, of the taps of output o that the clamping puts on input i
extern "C" void bt_matrix(int n, float* F) {
  for (int k = 0; k < 2 * n * n; ++k) F[k] = 0.f;
  for (int o = 0; o < 2 * n; ++o)
    for (int t = 0; t < BT_TAPS; ++t) F[o * n + bt_fwd_index(o, n, t)] += bt_fwd_weight(o, t);
}

// -> the number of failed checks for maps of n inputs
extern "C" int bt_check(int n) {
  std::vector<float> F(2 * (size_t)n * n);
  bt_matrix(n, F.data());
  int bad = 0;
  for (int o = 0; o < 2 * n; ++o) {                                       // every output row sums to one
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += F[o * n + i];
    bad += s != 1.f;
    for (int t = 0; t < BT_TAPS; ++t) bad += bt_fwd_index(o, n, t) < 0 || bt_fwd_index(o, n, t) >= n;
  }
  // the folded weights are the matrix's columns, zero outside the map; the predicate excludes no weight that is not zero, and
  // admits at most BT_BWD_TAPS consecutive outputs from 2i + BT_BWD_FIRST
  for (int i = -3; i < n + 3; ++i) {
    int admitted = 0;
    for (int o = -8; o < 2 * n + 8; ++o) {
      const bool inside = i >= 0 && i < n && o >= 0 && o < 2 * n;
      const float want = inside ? F[o * n + i] : 0.f;
      const bool may = bt_bwd_may_be_nonzero(i, n, o);
      bad += bt_bwd_weight(i, n, o) != want;
      bad += want != 0.f && !may;
      bad += may && (o < 2 * i + BT_BWD_FIRST || o >= 2 * i + BT_BWD_FIRST + BT_BWD_TAPS || !inside);
      admitted += may;
    }
    bad += admitted > BT_BWD_TAPS;
  }
  return bad;
}

int main() {
  int bad = 0;
  for (int n = 1; n <= 12; ++n) {
    const int b = bt_check(n);
    if (b) std::printf("n = %d: %d checks failed\n", n, b);
    bad += b;
  }
  std::printf("n = 1 .. 12: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
