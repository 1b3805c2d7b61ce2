// Host build of camradepth_amd/csrc/match_pick.h for tests/test_match_pick_cpu.py: the pick of k_match_pick as a reduction by
// mp_better over the candidates in natural or in shuffled order, folded in pairs as the kernel's tree does, and the pose composition of
// k_match_prepare and k_match_pick.  Built by the test as a shared library (c++ -shared) and, with the main below, as a stand-alone
// program, which is the form a sanitizer goes on.  The program reads problems from the file named on the command line; numbers
// separated by white space, doubles as C99 hex floats:
//   the number of tables, then per table   n_xy n_theta | NT * NS * NS scores | t dx dy (expected)
//   the number of poses, then per pose     12 x T | Sx Sy | c s | centre dx dy | cell | 12 x expected
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

#include "match_pick.h"

namespace {

uint64_t next_random(uint64_t& s) {                                      // xorshift64
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  return s;
}

}  // namespace

// table [2 n_theta + 1][2 n_xy + 1][2 n_xy + 1]; seed 0: the candidates in natural order, otherwise shuffled by it.  pick: (t, dx, dy).
extern "C" long long mp_pick(const long long* table, int n_xy, int n_theta, uint64_t seed, int32_t* pick) {
  const int ns = 2 * n_xy + 1, per = (2 * n_theta + 1) * ns * ns;
  std::vector<int> order(per);
  std::iota(order.begin(), order.end(), 0);
  uint64_t s = seed;
  if (seed)
    for (std::size_t k = order.size(); k > 1; --k) std::swap(order[k - 1], order[next_random(s) % k]);
  std::vector<MpCandidate> best;
  for (int i : order) best.push_back(mp_at(table, i, n_xy));
  while (best.size() > 1) {                                              // the tree: pairs at a distance of half the length
    const std::size_t half = (best.size() + 1) / 2;
    for (std::size_t k = 0; k + half < best.size(); ++k)
      if (mp_better(best[k + half], best[k], n_theta)) best[k] = best[k + half];
    best.resize(half);
  }
  pick[0] = best[0].t; pick[1] = best[0].dx; pick[2] = best[0].dy;
  return best[0].score;
}

// out [12]: T'[t] of T about S by (c, s), then moved by (dx, dy) cells
extern "C" void mp_pose(const double* T, const double* S, double c, double s, int centre, int dx, int dy, double cell, double* candidate,
                        double* out) {
  mp_candidate(T, S, c, s, centre != 0, candidate);
  mp_shifted(candidate, dx, dy, cell, out);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s problems.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  int tables = 0, poses = 0, bad = 0;
  bool ok = std::fscanf(f, "%d", &tables) == 1 && tables >= 1;
  for (int p = 0; ok && p < tables; ++p) {
    int n_xy, n_theta, want[3];
    ok = std::fscanf(f, "%d %d", &n_xy, &n_theta) == 2 && n_xy >= 0 && n_xy <= MP_MAX_XY && n_theta >= 0 && n_theta <= MP_MAX_THETA;
    if (!ok) break;
    const int ns = 2 * n_xy + 1, per = (2 * n_theta + 1) * ns * ns;
    std::vector<long long> table(per);
    for (int i = 0; i < per; ++i) ok &= std::fscanf(f, "%lld", &table[i]) == 1;
    ok &= std::fscanf(f, "%d %d %d", &want[0], &want[1], &want[2]) == 3;
    if (!ok) break;
    const uint64_t seeds[3] = {0, 1, 0x9E3779B97F4A7C15ull};
    for (uint64_t seed : seeds) {
      int32_t got[3];
      mp_pick(table.data(), n_xy, n_theta, seed, got);
      if (got[0] != want[0] || got[1] != want[1] || got[2] != want[2]) {
        std::printf("table %d, seed %llu: pick (%d, %d, %d), want (%d, %d, %d)\n", p, (unsigned long long)seed, got[0], got[1], got[2], want[0],
                    want[1], want[2]);
        ++bad;
      }
    }
  }
  ok = ok && std::fscanf(f, "%d", &poses) == 1 && poses >= 1;
  for (int p = 0; ok && p < poses; ++p) {
    double T[12], S[2], c, s, cell, want[12], candidate[12], got[12];
    int centre, dx, dy;
    for (double& v : T) ok &= std::fscanf(f, "%la", &v) == 1;
    ok &= std::fscanf(f, "%la %la %la %la %d %d %d %la", &S[0], &S[1], &c, &s, &centre, &dx, &dy, &cell) == 8;
    for (double& v : want) ok &= std::fscanf(f, "%la", &v) == 1;
    if (!ok) break;
    mp_pose(T, S, c, s, centre, dx, dy, cell, candidate, got);
    if (std::memcmp(got, want, sizeof got) != 0) {
      std::printf("pose %d differs\n", p);
      ++bad;
    }
  }
  std::fclose(f);
  if (!ok) {
    std::printf("malformed file\n");
    return 2;
  }
  std::printf("%d tables, %d poses: %s\n", tables, poses, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
