// Register-path skeleton of the pointwise MFMA GEMMs whose A rows are transformed on their way into LDS: k_gngemm_reg (gngemm.hip,
// GroupNorm apply in the operand load) and k_gnbwd_gemm (xfgemm.hip, GroupNorm-backward apply).  Both operands go by buffer_load to
// registers two K-slabs ahead and by ds_write into a two-stage XOR-swizzled LDS tile; 4 waves, a (WM TM 32) x (WN TN 32) tile per
// workgroup.  Shared here: the slab's MFMAs, the accumulator start, the per-thread constants, the weight rows' offsets and loads, the rules
// of the pipelined K loop and the host-side LDS sizing / tile rule.  A kernel keeps what is its own: its coefficient table, the A-operand
// loads and their transform (its load_slab / store_slab lambdas), its prologue, its grid order -- and its copy of the K loop (below).
#pragma once
#include "conv_common.h"

namespace crdk {

constexpr int BK = 64;                       // K elements per slab: 8 granules of 8 bf16 per tile row
constexpr unsigned OOB = 0x80000000u;        // a buffer offset past every range: the load returns zeros, the store is dropped
typedef __attribute__((ext_vector_type(4))) unsigned u32x4r;

template <int TM, int TN, int WM, int WN>
__device__ __forceinline__ void mfma_slab(const bf16_t* sa, const bf16_t* sb, f32x16 (&acc)[TM][TN], int wm, int wn, int l) {
#pragma unroll
  for (int ks = 0; ks < BK / 16; ++ks) {
    bf16x8 af[TM], bfr[TN];
    const int gi2 = ks * 2 + (l >> 5);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = (wm * TM + i) * 32 + (l & 31);
      af[i] = *reinterpret_cast<const bf16x8*>(&sa[row * BK + ((gi2 ^ ((row >> 1) & 7)) << 3)]);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = (wn * TN + j) * 32 + (l & 31);
      bfr[j] = *reinterpret_cast<const bf16x8*>(&sb[row * BK + ((gi2 ^ ((row >> 1) & 7)) << 3)]);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
  }
}

// the accumulators start at the bias of their column (lane l holds column l & 31 of every 32 x 32 tile)
template <int TM, int TN, int WN>
__device__ __forceinline__ void init_acc(const ConvK& a, f32x16 (&acc)[TM][TN], int b, int n0, int wn, int l) {
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + (wn * TN + j) * 32 + (l & 31);
    const float bias_v = (a.bias && col < a.Cout) ? a.bias[(long long)b * a.bias_bstride + col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = bias_v;
  }
}

// A thread's share of every slab is 16 bytes of the rows r0 + 32 i of the A and of the B tile; LDS slot l & 7 of a row takes K granule g
// (k_igemm's XOR swizzle, applied on the source side: a thread's rows are 32 apart, so g is the same for all of them).
struct RegLane { int r0, g; };
__device__ __forceinline__ RegLane reg_lane(int wv, int l) {
  const int r0 = 8 * wv + (l >> 3);
  return {r0, (l & 7) ^ ((r0 >> 1) & 7)};
}

// Weight half of a slab.  Byte offsets of the thread's weight rows with the row's validity folded in: a row past Cout starts out of range
// and stays there whatever the K loop adds, so the loads are unconditional (THE K LOOP, below).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t reg_weight_rsrc(const ConvK& a) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, a.Cout * a.Ktot * 2, 0x00020000);
}
template <int B_IT>
__device__ __forceinline__ void reg_weight_offsets(const ConvK& a, int n0, int r0, unsigned (&woff)[B_IT]) {
#pragma unroll
  for (int j = 0; j < B_IT; ++j) {
    const int ng = n0 + r0 + 32 * j;
    woff[j] = ng < a.Cout ? (unsigned)(ng * a.Ktot * 2) : OOB;
  }
}
// kf: the thread's first K element of the slab (kt BK + 8 g); km: OOB on the K tail and on slabs past the end, else 0
template <int B_IT>
__device__ __forceinline__ void reg_load_weights(const __amdgpu_buffer_rsrc_t rw, const unsigned (&woff)[B_IT], int kf, unsigned km, u32x4r (&w)[B_IT]) {
#pragma unroll
  for (int j = 0; j < B_IT; ++j) w[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, (woff[j] + (unsigned)(kf * 2)) | km, 0, 0);
}

// THE K LOOP of both kernels (written out in each; the last paragraph says why).  On entry slabs 0 and 1 are in flight in registers -- load_slab(0, r0s);
// load_slab(1, r1s) at the head of the kernel, before anything is waited for -- and the kernel's table is on its way to LDS.
// load_slab(kt, regs) requests slab kt, store_slab(kt, stage, regs) transforms it into LDS stage `stage`:
//   lds_barrier(); store_slab(0, 0, r0s); load_slab(2, r0s); lds_barrier();                      the table, then slab 0
//   for (kt = 0; kt + 2 <= nK; kt += 2) {
//     store_slab(kt + 1, 1, r1s); load_slab(kt + 3, r1s); mfma_slab(stage 0); lds_barrier();
//     store_slab(kt + 2, 0, r0s); load_slab(kt + 4, r0s); mfma_slab(stage 1); lds_barrier();
//   }
//   if (kt < nK) { mfma_slab(stage 0); lds_barrier(); }                                           odd slab count: single-slab tail
// Steady state: two slabs per trip and NO CONDITIONAL MEMORY OPERATION in it.  A load or store under a branch -- even a wave-uniform one such
// as `if (kt + 3 < nK) load_slab(...)`, or `if (store_xn && ok)` around the store of the transformed operand, or an offset written as
// `ok ? computed : OOB` inside the loop, which the compiler turns into an exec-mask branch around the load (two loads into the same
// registers on two paths) -- makes the number of requests in flight depend on the path.  The compiler's wait insertion then assumes the
// path that issued fewer, and every use of a slab's registers also drains the YOUNGER slab's requests (s_waitcnt vmcnt(5..0) in the ISA
// where vmcnt(12..9) was meant): the two-slab prefetch is one slab deep.  So every load and store of load_slab / store_slab is
// unconditional: rows, K granules and whole slabs that do not exist carry out-of-range offsets (OOB folded into LOOP-INVARIANT offsets:
// zeros in, nothing out).  The barriers are lds_barrier() (common.h): __syncthreads() would wait for every register load in flight.
// The loop and the weight tile's ds_write are NOT functions of this header: as a __forceinline__ template over the two lambdas the loop
// left k_gngemm_reg as it was but moved registers and vmcnt immediates in three k_gnbwd_gemm instances (<2,0,0>: 204 -> 208 VGPRs), and
// the weight store as a helper did the same to five k_gngemm_reg instances (+4 VGPRs, vmcnt(3) -> vmcnt(4)).  A change to the loop
// is made in gngemm.hip and xfgemm.hip both.

// ---- host side ----
template <int BM, int BN>
constexpr size_t epilogue_bytes() { return (size_t)BM * (BN + 8) * 4 + 256 * 16 * 4 + 2048; }   // fp32 staging tile + folds behind it
// Dynamic LDS in front of the kernel's table: the two stages of both tiles, aliased by conv_epilogue's staging area (-> ConvK::lds_bytes)
template <int BM, int BN>
constexpr size_t reg_gemm_tile_bytes() {
  size_t tiles = (size_t)2 * (BM + BN) * BK * 2;
  if (tiles < epilogue_bytes<BM, BN>()) tiles = epilogue_bytes<BM, BN>();
  return (tiles + 255) / 256 * 256;
}
constexpr int REG_GEMM_LDS_MAX = 160 * 1024;          // tiles + table must fit; reserved once per kernel whatever the launch needs
// 64 x 64 tiles when 64 x 128 ones would not cover the chip (as crd_conv_igemm chooses)
inline bool reg_gemm_small_tiles(const ConvK& k, int B) {
  const long long big_tiles = (long long)cdiv(k.OHW, 64) * cdiv(k.Cout, 128) * B;
  return k.Cout <= 64 || big_tiles < 256;
}

}  // namespace crdk
