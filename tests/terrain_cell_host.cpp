// Host build of camradepth_amd/csrc/terrain_cell.h for tests/test_terrain_cell_cpu.py: launch 4's rule (tc_fuse) over the cells of a
// window and launch 5's (tc_derive) with the nine grounds and weights gathered from the window as k_ter_derive gathers them.  Built by
// the test as a shared library (c++ -shared) and, with the main below, as a stand-alone program, which is the form a sanitizer goes
// on.  The program reads windows from the file named on the command line; integers separated by white space:
//   the number of windows, then per window   nx ny min_points w_max step_max_q slope2_max
//   and per cell, in window order            w ground top n lo hi | ground top w step slope2 state hazard (expected)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "terrain_cell.h"

// Every cell of a window: what the slot counts as (w, ground, top) and this call's observation (n, lo, hi) -> the fused triple
extern "C" void tch_fuse(int cells, const int32_t* w, const int32_t* ground, const int32_t* top, const int32_t* n, const int32_t* lo,
                         const int32_t* hi, int min_points, int w_max, int32_t* out_ground, int32_t* out_top, int32_t* out_w) {
  for (int c = 0; c < cells; ++c) {
    const TcFused f = tc_fuse(w[c], ground[c], top[c], n[c] >= min_points, lo[c], hi[c], w_max);
    out_ground[c] = f.ground;
    out_top[c] = f.top;
    out_w[c] = f.weight;
  }
}

// Every cell of a window [nx][ny] of fused triples -> step, slope2, state, hazard; a neighbour outside the window has weight 0
extern "C" void tch_derive(int nx, int ny, const int32_t* ground, const int32_t* top, const int32_t* w, int32_t step_max_q,
                           int64_t slope2_max, int32_t* step, int64_t* slope2, uint8_t* state, uint8_t* hazard) {
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j) {
      int32_t g9[9], w9[9];
      for (int k = 0; k < 9; ++k) {
        const int a = i + k / 3 - 1, b = j + k % 3 - 1;
        const bool in = a >= 0 && a < nx && b >= 0 && b < ny;
        g9[k] = in ? ground[a * ny + b] : 0;
        w9[k] = in ? w[a * ny + b] : 0;
      }
      const int c = i * ny + j;
      const TcDerived d = tc_derive(g9, w9, w9[4] ? top[c] : 0, step_max_q, slope2_max);
      step[c] = d.step;
      slope2[c] = d.slope2;
      state[c] = d.state;
      hazard[c] = d.hazard;
    }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s windows.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  int windows = 0, bad = 0;
  long long cells_seen = 0;
  bool ok = std::fscanf(f, "%d", &windows) == 1 && windows >= 1;
  for (int p = 0; ok && p < windows; ++p) {
    int nx, ny, min_points, w_max, step_max_q;
    long long slope2_max;
    ok = std::fscanf(f, "%d %d %d %d %d %lld", &nx, &ny, &min_points, &w_max, &step_max_q, &slope2_max) == 6 && nx >= 1 && ny >= 1 &&
         nx <= 65535 && ny <= 65535;
    if (!ok) break;
    const int cells = nx * ny;
    std::vector<int32_t> in[6], want[3], want_step(cells), got[3], step(cells);
    std::vector<int64_t> want_slope2(cells), slope2(cells);
    std::vector<int> want_state(cells), want_hazard(cells);
    std::vector<uint8_t> state(cells), hazard(cells);
    for (auto& v : in) v.resize(cells);
    for (auto& v : want) v.resize(cells);
    for (auto& v : got) v.resize(cells);
    for (int c = 0; ok && c < cells; ++c) {
      for (auto& v : in) ok &= std::fscanf(f, "%d", &v[c]) == 1;
      for (auto& v : want) ok &= std::fscanf(f, "%d", &v[c]) == 1;
      long long s2;
      ok &= std::fscanf(f, "%d %lld %d %d", &want_step[c], &s2, &want_state[c], &want_hazard[c]) == 4;
      want_slope2[c] = s2;
    }
    if (!ok) break;
    tch_fuse(cells, in[0].data(), in[1].data(), in[2].data(), in[3].data(), in[4].data(), in[5].data(), min_points, w_max, got[0].data(),
             got[1].data(), got[2].data());
    tch_derive(nx, ny, got[0].data(), got[1].data(), got[2].data(), step_max_q, slope2_max, step.data(), slope2.data(), state.data(),
               hazard.data());
    for (int c = 0; c < cells; ++c) {
      const bool same = got[0][c] == want[0][c] && got[1][c] == want[1][c] && got[2][c] == want[2][c] && step[c] == want_step[c] &&
                        slope2[c] == want_slope2[c] && state[c] == want_state[c] && hazard[c] == want_hazard[c];
      if (!same) {
        if (bad < 10) std::printf("window %d, cell %d differs\n", p, c);
        ++bad;
      }
    }
    cells_seen += cells;
  }
  std::fclose(f);
  if (!ok) {
    std::printf("malformed file\n");
    return 2;
  }
  std::printf("%d windows, %lld cells: %s\n", windows, cells_seen, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
