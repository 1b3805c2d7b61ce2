// Host build of the union-find body of camradepth_amd/csrc/object_ops.hip (object_uf.h) for tests/test_objects_ref_cpu.py: the same
// uf_find and uf_union over a plain array, driven over every pair of neighbouring source cells in natural or in shuffled order.
// Built by the test as a shared library (c++ -shared); with -DUF_MAIN a stand-alone program that checks random maps against a flood
// fill, which is the form a sanitizer goes on.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "object_uf.h"

namespace {

struct HostTable {
  int32_t* p;
  int load(int x) { return p[x]; }
  int fetch_min(int x, int v) {
    const int old = p[x];
    if (v < old) p[x] = v;
    return old;
  }
};

uint64_t next_random(uint64_t& s) {                                      // xorshift64
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  return s;
}

}  // namespace

// src: nx * ny bytes, non-zero on a source cell.  root: the root of every source cell after all unions, -1 on the others.  seed 0: the
// pairs in raster order; otherwise shuffled by it, and every second pair with its two cells swapped.  Returns 1 when a loop was capped.
extern "C" int uf_partition(const uint8_t* src, int nx, int ny, int connectivity, uint64_t seed, int32_t* root) {
  const int n = nx * ny;
  std::vector<int32_t> parent(n);
  for (int c = 0; c < n; ++c) parent[c] = src[c] ? c : -1;
  std::vector<std::pair<int, int>> pairs;
  const int di[4] = {0, 1, 1, 1}, dj[4] = {1, 0, -1, 1};
  const int n_dirs = connectivity == 8 ? 4 : 2;
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < n_dirs; ++k) {
        const int a = i + di[k], b = j + dj[k];
        if (a >= nx || b < 0 || b >= ny || !src[i * ny + j] || !src[a * ny + b]) continue;
        pairs.emplace_back(i * ny + j, a * ny + b);
      }
  if (seed) {
    uint64_t s = seed;
    for (size_t k = pairs.size(); k > 1; --k) std::swap(pairs[k - 1], pairs[next_random(s) % k]);
    for (size_t k = 0; k < pairs.size(); k += 2) std::swap(pairs[k].first, pairs[k].second);
  }
  HostTable t{parent.data()};
  bool capped = false;
  for (const auto& pr : pairs) uf_union(t, pr.first, pr.second, n, capped);
  for (int c = 0; c < n; ++c) root[c] = src[c] ? uf_find(t, c, n, capped) : -1;
  return capped ? 1 : 0;
}

#ifdef UF_MAIN
int main() {
  uint64_t s = 12345;
  int bad = 0;
  for (int trial = 0; trial < 60; ++trial) {
    const int nx = 1 + (int)(next_random(s) % 40), ny = 1 + (int)(next_random(s) % 90), conn = trial % 2 ? 8 : 4;
    const unsigned density = 20 + (unsigned)(next_random(s) % 60);
    std::vector<uint8_t> src(nx * ny);
    for (auto& v : src) v = next_random(s) % 100 < density;
    std::vector<int32_t> want(nx * ny, -1), natural(nx * ny), shuffled(nx * ny);
    for (int c = 0; c < nx * ny; ++c) {                                  // flood fill from every first cell, in index order
      if (!src[c] || want[c] >= 0) continue;
      std::vector<int> stack{c};
      want[c] = c;
      while (!stack.empty()) {
        const int x = stack.back();
        stack.pop_back();
        for (int a = -1; a <= 1; ++a)
          for (int b = -1; b <= 1; ++b) {
            if ((a == 0 && b == 0) || (conn == 4 && a != 0 && b != 0)) continue;
            const int i = x / ny + a, j = x % ny + b;
            if (i < 0 || i >= nx || j < 0 || j >= ny || !src[i * ny + j] || want[i * ny + j] >= 0) continue;
            want[i * ny + j] = c;
            stack.push_back(i * ny + j);
          }
      }
    }
    const int c1 = uf_partition(src.data(), nx, ny, conn, 0, natural.data());
    const int c2 = uf_partition(src.data(), nx, ny, conn, 77 + trial, shuffled.data());
    if (c1 || c2 || natural != want || shuffled != want) {
      std::printf("trial %d (%d x %d, %d-connected): capped %d %d, wrong\n", trial, nx, ny, conn, c1, c2);
      ++bad;
    }
  }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
