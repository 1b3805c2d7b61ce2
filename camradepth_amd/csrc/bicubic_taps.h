// The taps of the bicubic x2 kernels (bicubic.hip), plain C++ that compiles for the host as well: tests/bicubic_taps_host.cpp builds
// the forward matrix from the forward taps and checks the transpose's folded weights against its columns.
//   PyTorch upsample_bicubic2d, A = -0.75, scale 2, align_corners=False: output o of 2n reads four clamped inputs,
//     odd  o = 2k + 1: inputs k - 1 .. k + 2 with BT_WO,      even o = 2k: inputs k - 2 .. k + 1 with BT_WE
//   bt_fwd_index / bt_fwd_weight   tap t of output o: the clamped input index and its weight
//   bt_bwd_weight                  B[o][i], the weight of output o in the transpose's sum for input i: the taps of o that the clamping
//                                  folds onto i, added in tap order
//   bt_bwd_may_be_nonzero          B[o][i] can differ from zero only for o in [2i - 3, 2i + 4] (and inside the map): the clamping moves
//                                  a tap onto the first or the last input only from outputs that read that input anyway, so the
//                                  folded border rows have the interior's eight candidates
// Every weight is a multiple of 1/256 and every folded sum of them too: all of this is exact in fp32.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRD_BT_FN __host__ __device__ __forceinline__
#else
#define CRD_BT_FN inline
#endif

constexpr int BT_TAPS = 4;            // taps of an output
constexpr int BT_BWD_TAPS = 8;        // candidate outputs of an input: o = 2i - 3 + k, k = 0 .. 7
constexpr int BT_BWD_FIRST = -3;

CRD_BT_FN float bt_wo(int t) { return t == 0 ? -0.10546875f : t == 1 ? 0.87890625f : t == 2 ? 0.26171875f : -0.03515625f; }
CRD_BT_FN float bt_we(int t) { return t == 0 ? -0.03515625f : t == 1 ? 0.26171875f : t == 2 ? 0.87890625f : -0.10546875f; }

CRD_BT_FN int bt_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

CRD_BT_FN int bt_fwd_index(int o, int n, int t) {
  const int k = o >> 1;
  return bt_clamp(((o & 1) ? k - 1 : k - 2) + t, n);
}
CRD_BT_FN float bt_fwd_weight(int o, int t) { return (o & 1) ? bt_wo(t) : bt_we(t); }

CRD_BT_FN bool bt_bwd_may_be_nonzero(int i, int n, int o) {
  return i >= 0 && i < n && o >= 0 && o < 2 * n && o >= 2 * i + BT_BWD_FIRST && o < 2 * i + BT_BWD_FIRST + BT_BWD_TAPS;
}

// zero for an input or an output outside the map: the kernels read such a tap from a clamped address
CRD_BT_FN float bt_bwd_weight(int i, int n, int o) {
  float acc = 0.f;
  if (!bt_bwd_may_be_nonzero(i, n, o)) return acc;
  for (int t = 0; t < BT_TAPS; ++t)
    if (bt_fwd_index(o, n, t) == i) acc += bt_fwd_weight(o, t);
  return acc;
}
