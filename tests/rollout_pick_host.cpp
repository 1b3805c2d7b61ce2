// Host build of camradepth_amd/csrc/rollout_pick.h for tests/test_rollout_pick_cpu.py: the score of a record by rp_score and the pick of
// k_rollout_pick as a reduction by rp_better over the records in natural or in shuffled order, folded in pairs as the kernel's tree
// does.  Built by the test as a shared library (c++ -shared) and, with the main below, as a stand-alone program, which is the form a
// sanitizer goes on.  The program reads problems from the file named on the command line, integers separated by white space:
//   the number of problems, then per problem   K n_v n_w | togo max_cost sum_cost slow turn (the weights) | has_togo |
//                                              K x (end_togo max_cost sum_cost flags score) | the expected k, -1 without a valid one
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <utility>
#include <vector>

#include "rollout_pick.h"

namespace {

uint64_t next_random(uint64_t& s) {                                      // xorshift64
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  return s;
}

}  // namespace

// values [K][4]: end_togo, max_cost, sum_cost, flags of every record; weights [5]; scores [K] out.  seed 0: the records in natural
// order, otherwise shuffled by it.  -> the picked k, or -1 when the least record is not valid.
extern "C" int rp_pick(const int32_t* values, int K, int n_v, int n_w, const int32_t* weights, int has_togo, uint64_t seed, long long* scores) {
  RpWeights w;
  w.togo = weights[0]; w.max_cost = weights[1]; w.sum_cost = weights[2]; w.slow = weights[3]; w.turn = weights[4];
  std::vector<RpRecord> records(K);
  for (int k = 0; k < K; ++k) {
    const int32_t* v = values + 4 * k;
    RpRecord r = {};
    r.end_togo = v[0]; r.max_cost = v[1]; r.sum_cost = v[2]; r.flags = v[3];
    r.score = rp_score(w, has_togo, r.end_togo, r.max_cost, r.sum_cost, k, n_v, n_w);
    records[k] = r;
    scores[k] = r.score;
  }
  std::vector<int> order(K);
  std::iota(order.begin(), order.end(), 0);
  uint64_t s = seed;
  if (seed)
    for (std::size_t k = order.size(); k > 1; --k) std::swap(order[k - 1], order[next_random(s) % k]);
  std::vector<RpCandidate> best;
  for (int k : order) best.push_back(rp_at(records.data(), k, n_w));
  while (best.size() > 1) {                                              // the tree: pairs at a distance of half the length
    const std::size_t half = (best.size() + 1) / 2;
    for (std::size_t k = 0; k + half < best.size(); ++k)
      if (rp_better(best[k + half], best[k])) best[k] = best[k + half];
    best.resize(half);
  }
  return best[0].valid ? best[0].k : -1;
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
  int problems = 0, bad = 0;
  bool ok = std::fscanf(f, "%d", &problems) == 1 && problems >= 1;
  for (int p = 0; ok && p < problems; ++p) {
    int K, n_v, n_w, has_togo, want;
    int32_t weights[5];
    ok = std::fscanf(f, "%d %d %d", &K, &n_v, &n_w) == 3 && n_v >= 1 && n_v <= RP_MAX_V && n_w >= 1 && n_w <= RP_MAX_W && K == n_v * n_w &&
         K <= RP_MAX_K;
    if (!ok) break;
    for (int32_t& w : weights) ok &= std::fscanf(f, "%d", &w) == 1 && w >= 0 && w <= RP_MAX_WEIGHT;
    ok &= std::fscanf(f, "%d", &has_togo) == 1;
    std::vector<int32_t> values(4 * (std::size_t)K);
    std::vector<long long> want_scores(K), scores(K);
    for (int k = 0; ok && k < K; ++k)
      ok &= std::fscanf(f, "%d %d %d %d %lld", &values[4 * k], &values[4 * k + 1], &values[4 * k + 2], &values[4 * k + 3], &want_scores[k]) == 5;
    ok &= std::fscanf(f, "%d", &want) == 1;
    if (!ok) break;
    const uint64_t seeds[3] = {0, 1, 0x9E3779B97F4A7C15ull};
    for (uint64_t seed : seeds) {
      const int got = rp_pick(values.data(), K, n_v, n_w, weights, has_togo, seed, scores.data());
      if (got != want || scores != want_scores) {
        std::printf("problem %d, seed %llu: pick %d, want %d%s\n", p, (unsigned long long)seed, got, want,
                    scores != want_scores ? "; the scores differ" : "");
        ++bad;
      }
    }
  }
  std::fclose(f);
  if (!ok) {
    std::printf("malformed file\n");
    return 2;
  }
  std::printf("%d problems: %s\n", problems, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
