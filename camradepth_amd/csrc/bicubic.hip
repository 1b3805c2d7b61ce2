// Bicubic x2 of the decoder and its transpose for gfx950, as row-walking kernels: a thread owns one (column, 8-channel granule) of
// the INPUT-sized map and walks down the rows of its band, so every row is loaded and passed horizontally once per band instead of
// once per output row that needs it.  Consecutive lanes hold consecutive granules of a pixel (whole pixel rows, any C % 8 == 0: no
// channel windows, so C = 136 idles nothing), neighbouring columns share their loads through L1.  The taps are bicubic_taps.h.
//   forward    ring of the even / odd horizontal sums of four input rows; per input row five clamped 16-byte loads (requested one
//              row ahead), one horizontal pass, 2 x 2 outputs.  Order of operations per output as in the one-thread-per-pixel
//              form it replaces (horizontal t = 0 .. 3, then vertical t = 0 .. 3): bit-identical results.
//   transpose  dx = By^T (dy Bx): per dy row eight loads from clamped addresses (one row ahead) and one horizontal pass with the
//              thread's folded column weights, then added into the four pending dx rows the dy row belongs to with the band's
//              folded row weights (a table in LDS, written once); a dx row is stored when its last dy row has been added.
//              One kernel for every map size, H, W >= 1.
// A band of R rows re-reads 4 (forward) or 6 (transpose) halo rows; R halves from 8 while the grid would not cover the chip
// (tiling); on a grid smaller still the forward runs one thread per input pixel with all five rows requested at once.
#include "common.h"
#include "bicubic_taps.h"

namespace {

constexpr int TPB = 256;
constexpr int BAND_MAX = 16;                                  // (BAND_MAX + 3) * 8 row weights are written by one pass of the workgroup
typedef __attribute__((ext_vector_type(2))) float f32x2;

__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
// Ordering points for the compiler (empty asm statements keep their order): every sum of a row is complete at finish(), and
// nothing of a loaded row is unpacked before hold()
__device__ __forceinline__ void finish(float (&a)[8], float (&b)[8]) {
  asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                    "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]));
}
__device__ __forceinline__ void hold(uint4 (&r)[5]) {
  asm volatile("" : "+v"(r[0].x), "+v"(r[0].y), "+v"(r[0].z), "+v"(r[0].w), "+v"(r[1].x), "+v"(r[1].y), "+v"(r[1].z), "+v"(r[1].w),
                    "+v"(r[2].x), "+v"(r[2].y), "+v"(r[2].z), "+v"(r[2].w), "+v"(r[3].x), "+v"(r[3].y), "+v"(r[3].z), "+v"(r[3].w),
                    "+v"(r[4].x), "+v"(r[4].y), "+v"(r[4].z), "+v"(r[4].w));
}

// F8 = 1: the output is the e4m3 copy (y = bytes, y_ld in bytes) of the bf16 result, scaled by inv_scale; 2: that and the
// bf16 result itself (y2).  BURST: the form for grids too small to cover the chip with bands -- one thread per (input pixel, granule)
// over a flat grid, the five input rows requested at once (one memory latency per thread instead of three), one step, no loop
template <int F8, bool BURST>
__global__ __launch_bounds__(TPB) void k_bicubic_rows(const bf16_t* x, int x_ld, int H, int W, int C, void* y, int y_ld, float inv_scale,
                                                      void* y2, int y2_ld, int R) {
  const int b = blockIdx.z;
  const int CG = C >> 3;
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= (BURST ? H : 1) * W * CG) return;
  const int pix = i / CG, cg = i - pix * CG;
  const int k0 = BURST ? pix / W : blockIdx.y * R, k1 = k0 + R < H ? k0 + R : H;
  const int m = BURST ? pix - k0 * W : pix;
  const int OW = 2 * W;
  const bf16_t* xb = x + (long long)b * H * W * x_ld + cg * 8;
  int cxo[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) cxo[c] = bt_clamp(m - 2 + c, W) * x_ld;
  auto request = [&](int row, uint4 (&r)[5]) {
    const bf16_t* p = xb + (long long)bt_clamp(row, H) * W * x_ld;
#pragma unroll
    for (int c = 0; c < 5; ++c) r[c] = ld16(p + cxo[c]);
  };
  auto horizontal = [&](const uint4 (&r)[5], float (&he)[8], float (&ho)[8]) {
    float v[5][8];
#pragma unroll
    for (int c = 0; c < 5; ++c) unpack8(r[c], v[c]);
#pragma unroll
    for (int j = 0; j < 8; ++j) { he[j] = 0.f; ho[j] = 0.f; }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) { he[j] += bt_we(t) * v[t][j]; ho[j] += bt_wo(t) * v[t + 1][j]; }
  };
  // slot (row - k0 + 2) & 3 of the ring holds the horizontal sums of input row `row`
  float he[4][8], ho[4][8];
  uint4 raw[2][5];
  if (BURST) {
    uint4 r0[5], r1[5], r2[5];
    request(k0 - 2, r0); request(k0 - 1, r1); request(k0, r2); request(k0 + 1, raw[0]); request(k0 + 2, raw[1]);
    horizontal(r0, he[0], ho[0]); horizontal(r1, he[1], ho[1]); horizontal(r2, he[2], ho[2]); horizontal(raw[0], he[3], ho[3]);
  } else {
    // the first four rows, three requests in flight, one row's pass at a time (finish() / hold()): left to the compiler, the four
    // passes were interleaved with every unpacked operand alive (221 registers: two waves per SIMD; the loop needs under 150)
    uint4 r2[5];
    request(k0 - 2, raw[0]); request(k0 - 1, raw[1]); request(k0, r2);
    horizontal(raw[0], he[0], ho[0]); finish(he[0], ho[0]); request(k0 + 1, raw[0]);
    hold(raw[1]); horizontal(raw[1], he[1], ho[1]); finish(he[1], ho[1]); request(k0 + 2, raw[1]);
    hold(r2); horizontal(r2, he[2], ho[2]); finish(he[2], ho[2]);
    hold(raw[0]); horizontal(raw[0], he[3], ho[3]); finish(he[3], ho[3]);
  }
  // output row 2k + oy from the sums of its four input rows, in tap order
  auto emit = [&](int k, int oy, const float (&e0)[8], const float (&e1)[8], const float (&e2)[8], const float (&e3)[8],
                  const float (&o0)[8], const float (&o1)[8], const float (&o2)[8], const float (&o3)[8]) {
#pragma unroll
    for (int ox = 0; ox < 2; ++ox) {
      float out[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float wy = oy ? bt_wo(t) : bt_we(t);
        const float(&hr)[8] = ox ? (t == 0 ? o0 : t == 1 ? o1 : t == 2 ? o2 : o3) : (t == 0 ? e0 : t == 1 ? e1 : t == 2 ? e2 : e3);
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] += wy * hr[j];
      }
      const long long opix = (long long)b * 2 * H * OW + (long long)(2 * k + oy) * OW + 2 * m + ox;
      if (F8) store8_fp8(y, opix * y_ld + cg * 8, out, inv_scale);
      else store8_bf16(y, opix * y_ld + cg * 8, out);
      if (F8 == 2) store8_bf16(y2, opix * y2_ld + cg * 8, out);
    }
  };
  if (BURST) {
    emit(k0, 0, he[0], he[1], he[2], he[3], ho[0], ho[1], ho[2], ho[3]);
    horizontal(raw[1], he[0], ho[0]);
    emit(k0, 1, he[1], he[2], he[3], he[0], ho[1], ho[2], ho[3], ho[0]);
    return;
  }
  for (int k = k0; k < k1; k += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (k + u < k1) {                                       // (the same in every lane)
        // rows k+u-2 .. k+u+1 are in slots u .. u+3 (mod 4), row k+u+2 is in raw[(u + 1) & 1]: ask for the row after it first
        request(k + u + 3, raw[u & 1]);
        emit(k + u, 0, he[u & 3], he[(u + 1) & 3], he[(u + 2) & 3], he[(u + 3) & 3], ho[u & 3], ho[(u + 1) & 3], ho[(u + 2) & 3],
             ho[(u + 3) & 3]);
        horizontal(raw[(u + 1) & 1], he[u & 3], ho[u & 3]);   // row k+u+2 takes the slot of row k+u-2
        emit(k + u, 1, he[(u + 1) & 3], he[(u + 2) & 3], he[(u + 3) & 3], he[u & 3], ho[(u + 1) & 3], ho[(u + 2) & 3], ho[(u + 3) & 3],
             ho[u & 3]);
      }
    }
  }
}

// Step s of a band that starts at input row i0 is j = i0 - 3 + s: it adds the dy rows 2j + 3 and 2j + 4, which both belong to the
// input rows j .. j + 3 (a row outside the map has weight zero), and completes dx row j.  swy[s][0 .. 3] / [4 .. 7] are the weights of
// the two dy rows for those four input rows.  The dy row after the one in use is in flight (four in flight: no faster on any level).
__global__ __launch_bounds__(TPB) void k_bicubic_bwd_rows(const bf16_t* dy, int dy_ld, int H, int W, int C, bf16_t* dx, int dx_ld,
                                                          int accumulate, int R) {
  __shared__ __attribute__((aligned(16))) float swy[(BAND_MAX + 3) * 8];
  const int b = blockIdx.z;
  const int CG = C >> 3;
  const int i0 = blockIdx.y * R, i1 = i0 + R < H ? i0 + R : H;
  const int nsteps = i1 - i0 + 3;
  if ((int)threadIdx.x < nsteps * 8) {
    const int s = threadIdx.x >> 3, q = threadIdx.x & 7;
    const int j = i0 - 3 + s;
    swy[threadIdx.x] = bt_bwd_weight(j + (q & 3), H, 2 * j + 3 + (q >> 2));
  }
  __syncthreads();
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= W * CG) return;
  const int ix = i / CG, cg = i - ix * CG;
  const int OH = 2 * H, OW = 2 * W;
  const bf16_t* db = dy + (long long)b * OH * OW * dy_ld + cg * 8;
  float wx[BT_BWD_TAPS];
  int cxo[BT_BWD_TAPS];
#pragma unroll
  for (int c = 0; c < BT_BWD_TAPS; ++c) {
    const int o = 2 * ix + BT_BWD_FIRST + c;
    wx[c] = bt_bwd_weight(ix, W, o);
    cxo[c] = bt_clamp(o, OW) * dy_ld;
  }
  auto request = [&](int oy, uint4 (&r)[BT_BWD_TAPS]) {
    const bf16_t* p = db + (long long)bt_clamp(oy, OH) * OW * dy_ld;
#pragma unroll
    for (int c = 0; c < BT_BWD_TAPS; ++c) r[c] = ld16(p + cxo[c]);
  };
  f32x2 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[a][q] = f32x2{0.f, 0.f};
  // one dy row: horizontal pass, then into the pending rows a0 .. a3 with the weights w
  auto add_row = [&](const uint4 (&r)[BT_BWD_TAPS], const float4 w, f32x2 (&a0)[4], f32x2 (&a1)[4], f32x2 (&a2)[4], f32x2 (&a3)[4]) {
    f32x2 h[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q] = f32x2{0.f, 0.f};
#pragma unroll
    for (int c = 0; c < BT_BWD_TAPS; ++c) {
      const f32x2 wc = f32x2{wx[c], wx[c]};
      h[0] = __builtin_elementwise_fma(f32x2{bf_lo(r[c].x), bf_hi(r[c].x)}, wc, h[0]);
      h[1] = __builtin_elementwise_fma(f32x2{bf_lo(r[c].y), bf_hi(r[c].y)}, wc, h[1]);
      h[2] = __builtin_elementwise_fma(f32x2{bf_lo(r[c].z), bf_hi(r[c].z)}, wc, h[2]);
      h[3] = __builtin_elementwise_fma(f32x2{bf_lo(r[c].w), bf_hi(r[c].w)}, wc, h[3]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a0[q] = __builtin_elementwise_fma(h[q], f32x2{w.x, w.x}, a0[q]);
      a1[q] = __builtin_elementwise_fma(h[q], f32x2{w.y, w.y}, a1[q]);
      a2[q] = __builtin_elementwise_fma(h[q], f32x2{w.z, w.z}, a2[q]);
      a3[q] = __builtin_elementwise_fma(h[q], f32x2{w.w, w.w}, a3[q]);
    }
  };
  uint4 raw[2][BT_BWD_TAPS];
  request(2 * i0 - 3, raw[0]);
  const float4* sw4 = reinterpret_cast<const float4*>(swy);
  for (int s0 = 0; s0 < nsteps; s0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = s0 + u;
      if (s < nsteps) {                                       // (the same in every lane, like every branch below)
        // input row j + a is pending in acc[(u + a) & 3]
        const int j = i0 - 3 + s, oa = 2 * j + 3;
        request(oa + 1, raw[1]);
        const bool done = j >= i0;
        const long long off = ((long long)b * H * W + (long long)(done ? j : 0) * W + ix) * dx_ld + cg * 8;
        uint4 old = make_uint4(0, 0, 0, 0);
        if (done && accumulate) old = ld16(dx + off);
        const float4 wa = sw4[2 * s], wb = sw4[2 * s + 1];
        if ((unsigned)oa < (unsigned)OH) add_row(raw[0], wa, acc[u & 3], acc[(u + 1) & 3], acc[(u + 2) & 3], acc[(u + 3) & 3]);
        request(oa + 2, raw[0]);
        if ((unsigned)(oa + 1) < (unsigned)OH) add_row(raw[1], wb, acc[u & 3], acc[(u + 1) & 3], acc[(u + 2) & 3], acc[(u + 3) & 3]);
        if (done) {
          f32x2(&a)[4] = acc[u & 3];
          uint4 o;
          o.x = pack_bf2(a[0][0] + bf_lo(old.x), a[0][1] + bf_hi(old.x)); o.y = pack_bf2(a[1][0] + bf_lo(old.y), a[1][1] + bf_hi(old.y));
          o.z = pack_bf2(a[2][0] + bf_lo(old.z), a[2][1] + bf_hi(old.z)); o.w = pack_bf2(a[3][0] + bf_lo(old.w), a[3][1] + bf_hi(old.w));
          *reinterpret_cast<uint4*>(dx + off) = o;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[u & 3][q] = f32x2{0.f, 0.f};           // from the next step on: input row j + 4
      }
    }
  }
}

// Band height: eight rows, halved down to two while the grid would have fewer workgroups than the chip has CUs.  A grid that is
// smaller even then is a small map, whose launch time is one thread's chain of loads and arithmetic: the forward runs its BURST form.
// (Measured on the five levels of the 8 x 256 x 416 plan: bands of 16 rows, workgroups of 64 or 128 threads and bands of one row for
// the transpose were slower or equal; developer builds read CRD_BICUBIC_BAND.)
struct Tiling { int gx, rows; bool small; };
inline Tiling tiling(int H, int W, int CG, int B) {
  Tiling t;
  t.gx = cdiv((long long)W * CG, TPB);
  t.rows = 8;
  while (t.rows > 2 && (long long)cdiv(H, t.rows) * t.gx * B < 256) t.rows >>= 1;
  t.small = (long long)cdiv(H, t.rows) * t.gx * B < 256;
  const int forced = crd_dev_int("CRD_BICUBIC_BAND", 0);
  if (forced > 0) { t.rows = forced < BAND_MAX ? forced : BAND_MAX; t.small = false; }
  return t;
}

template <int F8>
void launch_rows(const void* x, int x_ld, int x_coff, int B, int H, int W, int C, void* y, int y_ld, float inv_scale, void* y2, int y2_ld,
                 crd_stream_t stream) {
  const Tiling t = tiling(H, W, C / 8, B);
  const bf16_t* xp = reinterpret_cast<const bf16_t*>(x) + x_coff;
  if (t.small)
    hipLaunchKernelGGL((k_bicubic_rows<F8, true>), dim3(cdiv((long long)H * W * (C / 8), TPB), 1, B), dim3(TPB), 0, as_stream(stream), xp, x_ld,
                       H, W, C, y, y_ld, inv_scale, y2, y2_ld, 1);
  else
    hipLaunchKernelGGL((k_bicubic_rows<F8, false>), dim3(t.gx, cdiv(H, t.rows), B), dim3(TPB), 0, as_stream(stream), xp, x_ld, H, W, C, y,
                       y_ld, inv_scale, y2, y2_ld, t.rows);
}

}  // namespace

extern "C" int crd_bicubic2x(const void* x, int32_t x_ld, int32_t x_coff, int32_t B, int32_t H, int32_t W, int32_t C, void* y,
                             int32_t y_ld, int32_t y_coff, crd_stream_t stream) {
  CRD_CHECK_ARG(x && y, "crd_bicubic2x: null pointer");
  CRD_CHECK_ARG(C % 8 == 0 && x_ld % 8 == 0 && x_coff % 8 == 0 && y_ld % 8 == 0 && y_coff % 8 == 0, "crd_bicubic2x: alignment");
  CRD_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "crd_bicubic2x: empty map");
  launch_rows<0>(x, x_ld, x_coff, B, H, W, C, reinterpret_cast<bf16_t*>(y) + y_coff, y_ld, 1.f, nullptr, 0, stream);
  CRD_LAUNCH_CHECK("crd_bicubic2x");
  return CRD_OK;
}

extern "C" int crd_bicubic2x_fp8(const void* x, int32_t x_ld, int32_t x_coff, int32_t B, int32_t H, int32_t W, int32_t C, void* y_fp8,
                                 int32_t y_ld, int32_t y_coff, float y_scale, void* y_bf16, int32_t yb_ld, int32_t yb_coff,
                                 crd_stream_t stream) {
  CRD_CHECK_ARG(x && y_fp8 && y_scale > 0.f, "crd_bicubic2x_fp8: null pointer / bad scale");
  CRD_CHECK_ARG(C % 8 == 0 && x_ld % 8 == 0 && x_coff % 8 == 0 && y_ld % 8 == 0 && y_coff % 8 == 0 && yb_ld % 8 == 0 && yb_coff % 8 == 0,
                "crd_bicubic2x_fp8: alignment");
  CRD_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "crd_bicubic2x_fp8: empty map");
  unsigned char* y8 = reinterpret_cast<unsigned char*>(y_fp8) + y_coff;
  if (y_bf16) launch_rows<2>(x, x_ld, x_coff, B, H, W, C, y8, y_ld, 1.f / y_scale, reinterpret_cast<bf16_t*>(y_bf16) + yb_coff, yb_ld, stream);
  else launch_rows<1>(x, x_ld, x_coff, B, H, W, C, y8, y_ld, 1.f / y_scale, nullptr, 0, stream);
  CRD_LAUNCH_CHECK("crd_bicubic2x_fp8");
  return CRD_OK;
}

extern "C" int crd_bicubic2x_bwd(const void* dy, int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                                 void* dx, int32_t dx_ld, int32_t dx_coff, int32_t accumulate, crd_stream_t stream) {
  CRD_CHECK_ARG(dy && dx, "crd_bicubic2x_bwd: null pointer");
  CRD_CHECK_ARG(C % 8 == 0 && dy_ld % 8 == 0 && dy_coff % 8 == 0 && dx_ld % 8 == 0 && dx_coff % 8 == 0, "crd_bicubic2x_bwd: alignment");
  CRD_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "crd_bicubic2x_bwd: empty map");
  const Tiling t = tiling(H, W, C / 8, B);
  hipLaunchKernelGGL(k_bicubic_bwd_rows, dim3(t.gx, cdiv(H, t.rows), B), dim3(TPB), 0, as_stream(stream),
                     reinterpret_cast<const bf16_t*>(dy) + dy_coff, dy_ld, H, W, C, reinterpret_cast<bf16_t*>(dx) + dx_coff, dx_ld,
                     accumulate, t.rows);
  CRD_LAUNCH_CHECK("crd_bicubic2x_bwd");
  return CRD_OK;
}
