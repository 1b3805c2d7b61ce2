// The union-find body of object_ops.hip, plain C++ that compiles for the host as well: tests/objects_uf_host.cpp runs it over the test
// cases in natural and in shuffled order.  A TABLE gives load(x), the parent of cell x read so that a value another thread has just
// written is seen sooner or later, and fetch_min(x, v), parent[x] = min(parent[x], v) as ONE atomic operation that returns the value
// before it.  Nothing else touches the table while unions run, so these hold at all times:
//   parent[x] <= x              a root is the lowest cell of its tree, the tree's FIRST CELL; a chain of parents strictly falls
//   a link is only ever lowered   fetch_min puts min(old, v) there; whichever of old and v lost its place is joined to the other by
//                               the retry below, so no connection is lost
// No call waits for another thread: a find or a union that loses a race goes on from the value the atomic returned.  Every loop has a
// hard cap (a chain of falling indices has at most `cap` = cells steps, a union lowers a link at every retry); a loop that reaches it
// leaves and sets `capped`, which the caller reports.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRD_UF_FN __host__ __device__ __forceinline__
#else
#define CRD_UF_FN inline
#endif

// the root of x: follows the parents until a cell is its own
template <class Table>
CRD_UF_FN int uf_find(Table& t, int x, int cap, bool& capped) {
  for (int step = 0; step <= cap; ++step) {
    const int p = t.load(x);
    if (p == x) return x;
    x = p;
  }
  capped = true;
  return x;
}

// joins the sets of a and b: the larger root is hung under the smaller
template <class Table>
CRD_UF_FN void uf_union(Table& t, int a, int b, int cap, bool& capped) {
  for (int retry = 0; retry <= cap; ++retry) {
    a = uf_find(t, a, cap, capped);
    b = uf_find(t, b, cap, capped);
    if (a == b || capped) return;
    if (a < b) { const int s = a; a = b; b = s; }                       // a: the larger root, b: the smaller
    const int old = t.fetch_min(a, b);
    if (old == a) return;                                               // a was still a root and now hangs under b
    // a had been hung under old < a meanwhile.  parent[a] is now min(old, b): one of the two lost its link to a, so join them.
    a = old;
  }
  capped = true;
}
