// Stand-alone form of tests/tracks_assoc_host.cpp for a sanitizer build (-fsanitize=address,undefined): reads association problems
// from the file named on the command line, runs ta_associate in natural and in two shuffled orders and compares with the expected
// assignment in the file.  tests/test_tracks_ref_cpu.py writes the file from its cases.  Format, numbers separated by white space,
// doubles as C99 hex floats: the number of problems, then per problem
//   T N n cap gate2 | T x (live px py) | N x (candidate zx zy) | T x trk_obj | N x obj_trk | rounds guard
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int ta_associate(int T, int N, int n, const double* px, const double* py, const uint8_t* live, const double* zx, const double* zy,
                            const uint8_t* candidate, double gate2, int cap, uint64_t seed, int32_t* trk_obj, int32_t* obj_trk,
                            int32_t* rounds);

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
  if (std::fscanf(f, "%d", &problems) != 1) problems = -1;
  for (int p = 0; p < problems; ++p) {
    int T, N, n, cap;
    double gate2;
    if (std::fscanf(f, "%d %d %d %d %la", &T, &N, &n, &cap, &gate2) != 5 || T < 0 || N < 0 || T > 4096 || N > 4096) { bad = -1; break; }
    std::vector<double> px(T), py(T), zx(N), zy(N);
    std::vector<uint8_t> live(T), candidate(N);
    std::vector<int32_t> want_t(T), want_k(N), got_t(T), got_k(N);
    bool ok = true;
    int flag;
    for (int t = 0; t < T; ++t) { ok &= std::fscanf(f, "%d %la %la", &flag, &px[t], &py[t]) == 3; live[t] = flag != 0; }
    for (int k = 0; k < N; ++k) { ok &= std::fscanf(f, "%d %la %la", &flag, &zx[k], &zy[k]) == 3; candidate[k] = flag != 0; }
    for (int t = 0; t < T; ++t) ok &= std::fscanf(f, "%d", &want_t[t]) == 1;
    for (int k = 0; k < N; ++k) ok &= std::fscanf(f, "%d", &want_k[k]) == 1;
    int want_rounds, want_guard;
    ok &= std::fscanf(f, "%d %d", &want_rounds, &want_guard) == 2;
    if (!ok) { bad = -1; break; }
    const uint64_t seeds[3] = {0, 1, 0x9E3779B97F4A7C15ull};
    for (uint64_t seed : seeds) {
      int32_t rounds = -1;
      const int guard = ta_associate(T, N, n, px.data(), py.data(), live.data(), zx.data(), zy.data(), candidate.data(), gate2, cap, seed,
                                     got_t.data(), got_k.data(), &rounds);
      if (guard != want_guard || rounds != want_rounds || got_t != want_t || got_k != want_k) {
        std::printf("problem %d, seed %llu: rounds %d (want %d), guard %d (want %d), assignment %s\n", p, (unsigned long long)seed, rounds,
                    want_rounds, guard, want_guard, got_t == want_t && got_k == want_k ? "equal" : "differs");
        ++bad;
      }
    }
  }
  std::fclose(f);
  if (bad < 0 || problems < 1) {
    std::printf("malformed file\n");
    return 2;
  }
  std::printf("%d problems: %s\n", problems, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
