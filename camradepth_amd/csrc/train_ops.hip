// Training-step kernels for gfx950: the multi-tensor diffGradNorm optimizer, the table-driven weight pack / gradient unpack between
// the reference's parameter layout and the bf16 [Cout][tap][Cin] layout the MFMA kernels read, crd_swap_f32 and the dropout
// masks.  All are HBM-bound streaming kernels.  (The losses are in losses.hip, the evaluation metrics in eval_ops.hip.)
#include <math.h>
#include "common.h"

namespace {

constexpr int TPB = 256;

// ---- diffGradNorm (src/models/diffGradNorm.py:73-110) -------------------------------------------
constexpr int OPT_CHUNK = 4096;  // elements per workgroup

// hp (device, optional): [beta1, beta2, eps, weight_decay, step_size] -- lets a captured HIP graph follow the
// per-iteration OneCycleLR schedule without re-capture
// GATED (skip_nonfinite): the same pass also tests every gradient element for NaN / inf and ORs the verdict into gate[0] -- one
// word per accumulation window; an OR does not depend on the order of the workgroups.
// CLIP (max_grad_norm): three more parts per workgroup, rows of norm_sq `ps` floats apart: [1] sum g^2 (the global norm's), and
// with weight decay [2] sum g.p and [3] sum p^2, so that k_dgn_scalar can form ||c g + wd p||^2 once the coefficient c is known
// without a second pass.  Row 0 stays the sum of (g + wd p)^2, the same operations in the same order as without CLIP.
template <bool GATED, bool CLIP = false>
__global__ __launch_bounds__(TPB) void k_dgn_norm(const float* p, const float* g, const long long* seg_off, const int* blk2seg,
                                                  const int* blk2chunk, float wd, const float* hp, float* norm_sq,
                                                  const unsigned char* active, int* gate, long long ps = 0) {
  if (hp) wd = hp[3];
  const int t = blk2seg[blockIdx.x];
  // A skipped tensor (`p.grad is None`, diffGradNorm.py:54-55) has NO gradient storage behind its segment when the gradients are used in
  // place (optim.diffGradNorm with separately allocated tensors: g = the first active gradient's pointer minus its offset): reading its
  // segment walked past the end of that allocation -- a memory access fault whenever it was the last block of an allocator segment
  // (round 6: the full GPU suite hit it once; round 1-5's k_dgn_update already skipped such tensors, this kernel did not).
  if (active && !active[t]) {
    if (threadIdx.x == 0) {
      norm_sq[blockIdx.x] = 0.f;
      if (CLIP) norm_sq[blockIdx.x + ps] = norm_sq[blockIdx.x + 2 * ps] = norm_sq[blockIdx.x + 3 * ps] = 0.f;
    }
    return;
  }
  const long long beg = seg_off[2 * t] + (long long)blk2chunk[blockIdx.x] * OPT_CHUNK;
  long long end = beg + OPT_CHUNK;
  if (end > seg_off[2 * t + 1]) end = seg_off[2 * t + 1];
  float s = 0.f, sg = 0.f, sgp = 0.f, spp = 0.f;
  bool bad = false;
  if (CLIP) {
    // explicit fmaf: the contractions the compiler makes of the loop below (g + wd p, s + gv^2), which it no longer makes once the
    // loop carries three more sums -- row 0 must keep the bits of norm_sq without CLIP
    for (long long i = beg + threadIdx.x; i < end; i += TPB) {
      float gv = g[i];
      if (GATED) bad |= !isfinite(gv);
      sg = fmaf(gv, gv, sg);
      if (wd != 0.f) {
        const float pv = p[i];
        sgp = fmaf(gv, pv, sgp);
        spp = fmaf(pv, pv, spp);
        gv = fmaf(wd, pv, gv);
      }
      s = fmaf(gv, gv, s);
    }
  } else {
    for (long long i = beg + threadIdx.x; i < end; i += TPB) {
      float gv = g[i];
      if (GATED) bad |= !isfinite(gv);
      if (wd != 0.f) gv += wd * p[i];
      s += gv * gv;
    }
  }
  if (GATED && bad) atomicOr(gate, 1);                     // rare path
  s = wave_sum(s);
  __shared__ float sm[4][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[0][w] = s;
  if (CLIP) {
    sg = wave_sum(sg); sgp = wave_sum(sgp); spp = wave_sum(spp);
    if ((threadIdx.x & 63) == 0) { sm[1][w] = sg; sm[2][w] = sgp; sm[3][w] = spp; }
  }
  __syncthreads();
  if (threadIdx.x == 0) norm_sq[blockIdx.x] = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3];     // this workgroup's part (plain store)
  if (CLIP && threadIdx.x < 3) {
    const int r = threadIdx.x + 1;
    norm_sq[blockIdx.x + r * ps] = sm[r][0] + sm[r][1] + sm[r][2] + sm[r][3];
  }
}

// max_grad_norm: torch.nn.utils.clip_grad_norm_'s total and coefficient from the sum g^2 parts of every workgroup (row 1 of
// k_dgn_norm<., true>; frozen tensors wrote 0).  One workgroup adds them in a FIXED order with an fp64 accumulator (lane-strided,
// then a tree in LDS): the same bits on every run, no float atomics.  clip[0] = total = ||g|| (fp32), clip[1] = coef =
// min(1, max_norm / (total + 1e-6)) formed as torch forms it in fp32 (max_norm * reciprocal(total + 1e-6), then clamp(max=1):
// a NaN total gives a NaN coefficient, as torch's with error_if_nonfinite=False).
__global__ __launch_bounds__(256) void k_grad_norm_total(const float* sq, int n, float max_norm, float* clip) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)sq[i];
  __shared__ double sm[256];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(sm[0]);
    float c = (1.f / (total + 1e-6f)) * max_norm;
    if (c > 1.f) c = 1.f;
    clip[0] = total;
    clip[1] = c;
  }
}

// c * g rounded on its own, as torch's in-place g.mul_(coef) leaves it, never fused with the weight-decay term that follows
__device__ __forceinline__ float clip_mul(float g, float c) {
#pragma clang fp contract(off)
  return g * c;
}

// per tensor: ||g||^2 = its workgroups' parts added in a FIXED order (lane-strided, then the butterfly), so the e > n
// branch below sees the same norm on every run; e <- 0.95 e + 0.05 n ; factor = e > n ? e/(n+1e-8) : 1.
// One wave per tensor.  The tensor's first workgroup is found by a 64-ary search in blk2seg (non-decreasing): two or
// three dependent loads for the ~6000 workgroups of the model.
// Gated commit (skip_nonfinite): gate = int32[8] on the device, [0] a gradient element was not finite (k_dgn_norm<true>), [1] a crd_sum_t
// partial was dropped during the window's backward (crd_nonfinite_capture), [2] committed optimizer steps, [3] skipped steps, [4] the last
// window's verdict, [5] the bits of this step's step_size.  The first wave of the scalar kernel takes the decision and keeps the
// counters; the update kernel (launched behind it) only reads.  Bias corrections: the host's step_size (hp[4], or the argument) as long
// as the device count of this step equals the host's (nothing skipped yet: the same bits as the ungated path), otherwise computed here in
// fp64 from the fp64 copies of lr / beta1 / beta2 the host leaves in hp[8..13] (hp[14]: the host's step number as an int32).
struct DgnGateHost { float step_size; int host_step; };
__device__ __forceinline__ void dgn_gate_decide(int* gate, const float* hp, DgnGateHost h) {
  const int bad = (gate[0] | gate[1]) ? 1 : 0;
  gate[4] = bad;
  if (bad) { gate[3] += 1; return; }
  const int n = gate[2] + 1;
  gate[2] = n;
  float ss = h.step_size;
  if (hp) {
    ss = hp[4];
    const int host_n = reinterpret_cast<const int*>(hp)[14];
    if (n != host_n) {
      const double* d = reinterpret_cast<const double*>(hp + 8);
      const double bc1 = 1.0 - pow(d[1], (double)n), bc2 = 1.0 - pow(d[2], (double)n);
      ss = (float)(d[0] * sqrt(bc2) / (bc1 + 1e-8));
    }
  }
  gate[5] = __float_as_int(ss);
}

// CLIP: the tensor's norm is that of c g + wd p, c = clip[1] (k_grad_norm_total).  With c == 1 it is row 0 of the parts, the
// bits of the path without clipping; otherwise c^2 sum g^2 + 2 c wd sum g.p + wd^2 sum p^2 from rows 1-3, each row added in the
// order row 0 is, combined in fp64.
template <bool GATED, bool CLIP = false>
__global__ __launch_bounds__(256) void k_dgn_scalar(float* exp_grad_norm, const float* norm_part, float* factor, const unsigned char* active,
                                                    int n, const long long* seg_off, const int* blk2seg, int n_blocks, int* gate,
                                                    const float* hp, DgnGateHost gh, float wd = 0.f, const float* clip = nullptr,
                                                    long long ps = 0) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (GATED) {
    const bool bad = gate[0] | gate[1];                    // (dgn_gate_decide does not write these two words)
    if (blockIdx.x == 0 && threadIdx.x == 0) dgn_gate_decide(gate, hp, gh);
    if (bad) return;                                       // skipped step: exp_grad_norm and factor stay as they are
  }
  if (t >= n) return;
  if (active && !active[t]) { if (lane == 0) factor[t] = 1.f; return; }
  int lo = 0, len = n_blocks;                      // the first workgroup of tensor t lies in [lo, lo + len]
  while (len > 0) {
    const int stride = (len + 63) >> 6;
    const int pos = lo + lane * stride;
    const bool less = pos < lo + len && blk2seg[pos] < t;
    const int k = __popcll(__ballot(less));        // blk2seg is sorted: the probes below t are the first k lanes
    if (k == 0) break;
    const int end = lo + len;
    lo += (k - 1) * stride + 1;
    len = min(stride - 1, end - lo);
  }
  const int cnt = (int)((seg_off[2 * t + 1] - seg_off[2 * t] + OPT_CHUNK - 1) / OPT_CHUNK);
  float s = 0.f;
  const float c = CLIP ? clip[1] : 1.f;
  if (!CLIP || c == 1.f) {
    for (int i = lane; i < cnt; i += 64) s += norm_part[lo + i];
    s = wave_sum(s);
  } else {
    if (hp) wd = hp[3];
    float a = 0.f, b = 0.f, q = 0.f;
    for (int i = lane; i < cnt; i += 64) {
      a += norm_part[ps + lo + i];
      b += norm_part[2 * ps + lo + i];
      q += norm_part[3 * ps + lo + i];
    }
    a = wave_sum(a); b = wave_sum(b); q = wave_sum(q);
    const double cd = c, wdd = wd;
    s = (float)(cd * cd * a + 2.0 * cd * wdd * b + wdd * wdd * q);
    if (s < 0.f) s = 0.f;                                  // rounding of a near-cancellation (a NaN stays NaN)
  }
  if (lane == 0) {
    const float nrm = sqrtf(s);
    const float e = 0.95f * exp_grad_norm[t] + 0.05f * nrm;
    factor[t] = e > nrm ? e / (nrm + 1e-8f) : 1.f;
    exp_grad_norm[t] = e;
  }
}

// ema_decay: the weight of step n of the parameters' exponential moving average, w_n = 1 - d_n, d_n = min(decay, (1 + n) / (10 + n))
// with the warm-up (timm's rule), else decay.  ONE fp32 expression for the host (ungated paths: it knows n) and the device (gated
// commit: only the device knows how many steps were committed), so that every path forms the same bits.
__host__ __device__ __forceinline__ float dgn_ema_weight(float decay, int warmup, int n) {
  const float d = warmup ? fminf(decay, (float)(1 + n) / (float)(10 + n)) : decay;
  return 1.0f - d;
}
// e: the EMA buffer (layout of p).  w: w_n of this step (hp[5] when hp is given).  Gated: decay / warmup / base (hp[6], int32 at hp[15] /
// hp[7] when hp is given), base = gate[2] when the EMA was created or restored: n = committed steps since then.
struct DgnEma { float* e; float w; float decay; int warmup; int base; };

// CLIP: g <- c g (c = clip[1]) before the weight decay is added; c == 1 leaves every bit as it is
// EMA: e <- fmaf(w_n, p_new - e, e) on the value about to be stored (in a register: one more load and store per element, same
// lane -> address map as p, so the stream coalesces as p's does); frozen tensors and skipped windows return above it
template <bool GATED, bool CLIP = false, bool EMA = false>
__global__ __launch_bounds__(TPB) void k_dgn_update(float* p, const float* g, float* m, float* v, float* pg, const float* factor,
                                                    const long long* seg_off, const int* blk2seg, const int* blk2chunk,
                                                    const unsigned char* active, float beta1, float beta2, float eps, float wd,
                                                    float step_size, const float* hp, const int* gate, const float* clip = nullptr,
                                                    DgnEma ea = DgnEma{}) {
  if (hp) { beta1 = hp[0]; beta2 = hp[1]; eps = hp[2]; wd = hp[3]; step_size = hp[4]; }
  if (GATED) {
    if (gate[4]) return;                                   // the window saw a non-finite gradient: nothing is written
    step_size = __int_as_float(gate[5]);
  }
  float ew = 0.f;
  if (EMA) {
    ew = hp ? hp[5] : ea.w;
    if (GATED) {                                           // (gate[2]: this step included, k_dgn_scalar counted it)
      const int* hi = reinterpret_cast<const int*>(hp);
      ew = hp ? dgn_ema_weight(hp[6], hi[15], gate[2] - hi[7]) : dgn_ema_weight(ea.decay, ea.warmup, gate[2] - ea.base);
    }
  }
  const int t = blk2seg[blockIdx.x];
  if (active && !active[t]) return;
  const long long beg = seg_off[2 * t] + (long long)blk2chunk[blockIdx.x] * OPT_CHUNK;
  long long end = beg + OPT_CHUNK;
  if (end > seg_off[2 * t + 1]) end = seg_off[2 * t + 1];
  const float f = factor[t];
  const float c = CLIP ? clip[1] : 1.f;
  for (long long i = beg + threadIdx.x; i < end; i += TPB) {
    float gv = g[i];
    const float pv = p[i];
    if (CLIP) {                                            // (fmaf: the contraction of the line below, see k_dgn_norm)
      gv = clip_mul(gv, c);
      if (wd != 0.f) gv = fmaf(wd, pv, gv);
    } else if (wd != 0.f) {
      gv += wd * pv;
    }
    const float g1 = gv * f;
    const float mv = beta1 * m[i] + (1.f - beta1) * g1;
    const float vv = beta2 * v[i] + (1.f - beta2) * gv * gv;
    const float dfc = 1.f / (1.f + expf(-fabsf(pg[i] - gv)));
    m[i] = mv; v[i] = vv; pg[i] = gv;
    const float pn = pv - step_size * (mv * dfc) / (sqrtf(vv) + eps);
    p[i] = pn;
    if (EMA) {
      const float ev = ea.e[i];
      ea.e[i] = fmaf(ew, pn - ev, ev);
    }
  }
}

// crd_swap_f32: a[i] <-> b[i].  `head` leading and the trailing elements one by one, nvec float4 pairs between them (16-byte loads
// and stores: the host picked head so that both are aligned there, or nvec = 0).  Every element belongs to exactly one lane.
__global__ __launch_bounds__(TPB) void k_swap_f32(float* a, float* b, long long n, long long head, long long nvec) {
  const long long tid = (long long)blockIdx.x * TPB + threadIdx.x, stride = (long long)gridDim.x * TPB;
  float4* a4 = reinterpret_cast<float4*>(a + head);
  float4* b4 = reinterpret_cast<float4*>(b + head);
  for (long long i = tid; i < nvec; i += stride) {
    const float4 x = a4[i], y = b4[i];
    a4[i] = y; b4[i] = x;
  }
  const long long tail0 = head + 4 * nvec, rem = head + (n - tail0);
  for (long long i = tid; i < rem; i += stride) {
    const long long j = i < head ? i : tail0 + (i - head);
    const float x = a[j], y = b[j];
    a[j] = y; b[j] = x;
  }
}

// ---- weight pack / gradient unpack ------------------------------------------------------------------
// One pass over the fp32 parameters: a workgroup stages a tile of 16 output channels x CI_T internal input channels x all
// taps in LDS (source reads run along the reference layout [co][ci][tap], so they are contiguous and every parameter is
// fetched ONCE), then writes the tile in each requested packed order with the destination's fastest index on the lanes.
// (The previous kernel walked every destination form separately and gathered the source with a `taps`-float stride per
// lane: 728 MB of fetches per step for 88 MB of parameters.)
constexpr int WP_CO = 16, WP_ELEMS = 512;
__global__ __launch_bounds__(TPB) void k_weight_pack(const crd_pack_entry* tab) {
  __shared__ float tile[WP_CO * WP_ELEMS];
  const crd_pack_entry e = tab[blockIdx.y];
  int ci_t = (WP_ELEMS / e.taps) & ~7;
  if (ci_t < 8) ci_t = 8;                                   // taps <= 64: 8 channels x 64 taps = 512
  if (ci_t > 64) ci_t = 64;
  const int n_ci = (e.Cin_pad + ci_t - 1) / ci_t, n_co = (e.Cout_pad + WP_CO - 1) / WP_CO;
  const int per_co = ci_t * e.taps;                         // <= WP_ELEMS
  for (int tl = blockIdx.x; tl < n_ci * n_co; tl += gridDim.x) {
    const int co0 = (tl / n_ci) * WP_CO, ci0 = (tl % n_ci) * ci_t;
    __syncthreads();                                        // the previous tile has been written out
    for (int i = threadIdx.x; i < WP_CO * per_co; i += TPB) {
      const int co = co0 + i / per_co, r = i % per_co;
      const int ci = ci0 + r / e.taps, tap = r % e.taps;
      float v = 0.f;
      if (co < e.Cout && ci < e.Cin_pad) {
        const int cr = e.cmap ? e.cmap[ci] : (ci < e.Cin_ref ? ci : -1);
        if (cr >= 0) v = e.src[((long long)co * e.Cin_ref + cr) * e.taps + tap];
      }
      tile[i] = v;
    }
    __syncthreads();
    if (e.dst_fwd) {                                        // [co][tap][ci]: ci on the lanes
      for (int i = threadIdx.x; i < WP_CO * per_co; i += TPB) {
        const int cl = i % ci_t, r = i / ci_t;
        const int tap = r % e.taps, col = r / e.taps;
        const int co = co0 + col, ci = ci0 + cl;
        if (co < e.Cout && ci < e.Cin_pad) {
          const float v = tile[col * per_co + cl * e.taps + tap];
          const long long o = ((long long)co * e.taps + tap) * e.Cin_pad + ci;
          if (e.dst_f32) reinterpret_cast<float*>(e.dst_fwd)[o] = e.dst_f32 == 2 ? bf_round(v) : v;
          else reinterpret_cast<bf16_t*>(e.dst_fwd)[o] = f2bf(v);
        }
      }
    }
    if (e.dst_dgrad || e.dst_scatter) {                     // [ci][tap][co_pad] / [tap][ci][co_pad]: co on the lanes
      for (int i = threadIdx.x; i < WP_CO * per_co; i += TPB) {
        const int col = i % WP_CO, r = i / WP_CO;
        const int tap = r % e.taps, cl = r / e.taps;
        const int co = co0 + col, ci = ci0 + cl;
        if (co < e.Cout_pad && ci < e.Cin_pad) {
          const bf16_t q = f2bf(tile[col * per_co + cl * e.taps + tap]);      // zero beyond Cout (never loaded)
          if (e.dst_dgrad) {
            if (e.dgrad_ld == 0) reinterpret_cast<bf16_t*>(e.dst_dgrad)[((long long)ci * e.taps + tap) * e.Cout_pad + co] = q;
            else {                                             // K-concatenated form: a row range of this layer's input channels
              const int rr = ci - e.dgrad_row0;
              if (rr >= 0 && rr < e.dgrad_rows)
                reinterpret_cast<bf16_t*>(e.dst_dgrad)[((long long)rr * e.taps + tap) * e.dgrad_ld + e.dgrad_coff + co] = q;
            }
          }
          if (e.dst_scatter) reinterpret_cast<bf16_t*>(e.dst_scatter)[((long long)tap * e.Cin_pad + ci) * e.Cout_pad + co] = q;
        }
      }
    }
  }
}

// Copies of a replicated accumulator are added in index order (fixed: reproducible); fixed-point sources (src_sum) are
// added as integers and converted once.
__global__ __launch_bounds__(TPB) void k_wgrad_unpack(const crd_unpack_entry* tab, int accumulate) {
  const crd_unpack_entry e = tab[blockIdx.y];
  const long long n = (long long)e.Cout * e.taps * e.Cin_pad;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
    const int ci = (int)(i % e.Cin_pad);
    const long long r = i / e.Cin_pad;
    const int tap = (int)(r % e.taps), co = (int)(r / e.taps);
    const int cr = e.cmap ? e.cmap[ci] : (ci < e.Cin_ref ? ci : -1);
    if (cr < 0) continue;
    float* d = e.dst + ((long long)co * e.Cin_ref + cr) * e.taps + tap;
    float v;
    if (e.src_sum) {
      const crd_sum_t* src = reinterpret_cast<const crd_sum_t*>(e.src);
      long long q = src[i], q1 = 0, q2 = 0, q3 = 0;          // independent chains keep several loads in flight
      int rp = 1;
      for (; rp + 3 <= e.replicas; rp += 3) {
        q1 += src[(long long)rp * e.replica_stride + i];
        q2 += src[(long long)(rp + 1) * e.replica_stride + i];
        q3 += src[(long long)(rp + 2) * e.replica_stride + i];
      }
      for (; rp < e.replicas; ++rp) q += src[(long long)rp * e.replica_stride + i];
      v = (float)(q + q1 + q2 + q3) * (1.f / GRAD_ONE);
    } else {
      const float* src = reinterpret_cast<const float*>(e.src);
      float v1 = 0.f, v2 = 0.f, v3 = 0.f;
      v = src[i];
      int rp = 1;
      for (; rp + 3 <= e.replicas; rp += 3) {
        v1 += src[(long long)rp * e.replica_stride + i];
        v2 += src[(long long)(rp + 1) * e.replica_stride + i];
        v3 += src[(long long)(rp + 2) * e.replica_stride + i];
      }
      for (; rp < e.replicas; ++rp) v += src[(long long)rp * e.replica_stride + i];
      v += (v1 + v2) + v3;
    }
    *d = accumulate ? *d + v : v;
  }
}

// out[r][c] = u(r,c) < keep[r] ? 1/keep[r] : 0 with a counter-based hash RNG; *counter advances once per launch,
// so a captured graph draws fresh masks on every replay.
__global__ __launch_bounds__(TPB) void k_dropout_masks(float* out, const float* keep, int rows, int cols, unsigned long long seed,
                                                       unsigned long long* counter) {
  const unsigned long long epoch = *counter;
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    const int r = (int)(i / cols);
    const float kp = keep[r];
    const unsigned long long h = splitmix64(splitmix64(seed ^ (epoch * 0xD1342543DE82EF95ull)) + (unsigned long long)i);
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
    out[i] = u < kp ? 1.0f / kp : 0.0f;
  }
}
__global__ void k_counter_inc(unsigned long long* counter) { *counter += 1; }

}  // namespace

// ---- diffGradNorm: crd_dgn_desc (include/camradepth_hip.h).  The switches are gate / clip / ema != NULL; the kernels take them as
// template flags, and dgn_norm / dgn_commit below are the only places that map the one onto the other. ----
template <bool GATED, bool CLIP>
static void dgn_norm_launch(const crd_dgn_desc& d, hipStream_t st) {
  hipLaunchKernelGGL((k_dgn_norm<GATED, CLIP>), dim3(d.n_blocks), dim3(TPB), 0, st, d.p, d.g, reinterpret_cast<const long long*>(d.seg_off),
                     d.blk2seg, d.blk2chunk, d.weight_decay, d.hp_dev, d.parts, d.active, d.gate, (long long)d.parts_stride);
}
static void dgn_norm(const crd_dgn_desc& d, hipStream_t st) {
  switch ((d.gate ? 2 : 0) | (d.clip ? 1 : 0)) {
    case 0: dgn_norm_launch<false, false>(d, st); break;
    case 1: dgn_norm_launch<false, true>(d, st); break;
    case 2: dgn_norm_launch<true, false>(d, st); break;
    default: dgn_norm_launch<true, true>(d, st); break;
  }
}

// [total + coefficient,] the per-tensor scalars, the update.  Arguments an instantiation does not read (gate, clip, the EMA,
// hp in the plain scalar kernel) are passed as they are in the descriptor.
template <bool GATED, bool CLIP, bool EMA>
static void dgn_commit_launch(const crd_dgn_desc& d, float step_size, const DgnEma& ea, hipStream_t st) {
  const long long* so = reinterpret_cast<const long long*>(d.seg_off);
  const long long ps = d.parts_stride;
  if (CLIP) hipLaunchKernelGGL(k_grad_norm_total, dim3(1), dim3(256), 0, st, d.parts + ps, d.n_blocks, d.max_norm, d.clip);
  hipLaunchKernelGGL((k_dgn_scalar<GATED, CLIP>), dim3(cdiv(d.n_tensors, 4)), dim3(256), 0, st, d.exp_grad_norm, d.parts, d.factor, d.active,
                     d.n_tensors, so, d.blk2seg, d.n_blocks, d.gate, d.hp_dev, DgnGateHost{step_size, d.step}, d.weight_decay,
                     (const float*)d.clip, ps);
  hipLaunchKernelGGL((k_dgn_update<GATED, CLIP, EMA>), dim3(d.n_blocks), dim3(TPB), 0, st, d.p, d.g, d.exp_avg, d.exp_avg_sq, d.prev_grad,
                     d.factor, so, d.blk2seg, d.blk2chunk, d.active, d.beta1, d.beta2, d.eps, d.weight_decay, step_size, d.hp_dev,
                     (const int*)d.gate, (const float*)d.clip, ea);
}
static void dgn_commit(const crd_dgn_desc& d, hipStream_t st) {
  const double bc1 = 1.0 - pow((double)d.beta1, (double)d.step), bc2 = 1.0 - pow((double)d.beta2, (double)d.step);
  const float step_size = (float)((double)d.lr * sqrt(bc2) / (bc1 + 1e-8));
  // without a gate the host forms w_n (read when hp_dev is NULL); with one the device forms it from its own count and the base
  DgnEma ea{};
  if (d.ema) ea = DgnEma{d.ema, d.gate ? 0.f : dgn_ema_weight(d.ema_decay, d.ema_warmup, d.ema_n), d.ema_decay, d.ema_warmup,
                         d.gate ? d.ema_base : 0};
  switch ((d.gate ? 4 : 0) | (d.clip ? 2 : 0) | (d.ema ? 1 : 0)) {
    case 0: dgn_commit_launch<false, false, false>(d, step_size, ea, st); break;
    case 1: dgn_commit_launch<false, false, true>(d, step_size, ea, st); break;
    case 2: dgn_commit_launch<false, true, false>(d, step_size, ea, st); break;
    case 3: dgn_commit_launch<false, true, true>(d, step_size, ea, st); break;
    case 4: dgn_commit_launch<true, false, false>(d, step_size, ea, st); break;
    case 5: dgn_commit_launch<true, false, true>(d, step_size, ea, st); break;
    case 6: dgn_commit_launch<true, true, false>(d, step_size, ea, st); break;
    default: dgn_commit_launch<true, true, true>(d, step_size, ea, st); break;
  }
}

// The argument checks of all three entry points, before any launch.  commit = false: the norm pass alone, which reads nothing more
// than what the first two checks cover.
static int dgn_check(const char* who, const crd_dgn_desc* d, bool commit) {
  CRD_CHECK_ARG(d, "%s: null descriptor", who);
  CRD_CHECK_ARG(d->p && d->g && d->parts && d->seg_off && d->blk2seg && d->blk2chunk && d->n_blocks > 0,
                "%s: bad argument (p, g, parts or a table is null, or n_blocks <= 0)", who);
  if (d->clip) CRD_CHECK_ARG(d->parts_stride >= d->n_blocks, "%s: bad argument (clip: parts_stride < n_blocks)", who);
  if (!commit) return CRD_OK;
  CRD_CHECK_ARG(d->exp_avg && d->exp_avg_sq && d->prev_grad && d->exp_grad_norm && d->factor && d->n_tensors > 0 && d->step >= 1,
                "%s: bad argument (an optimizer-state buffer is null, n_tensors <= 0 or step < 1)", who);
  if (d->clip) {
    CRD_CHECK_ARG(d->max_norm > 0.f, "%s: bad argument (clip: max_norm must be > 0)", who);
    // k_grad_norm_total adds row 1 over n_blocks: a commit over a slice of the blocks would clip with a partial norm
    CRD_CHECK_ARG(d->parts_stride == d->n_blocks, "%s: bad argument (clip: the commit takes all blocks, parts_stride == n_blocks)", who);
  }
  if (d->ema) {
    CRD_CHECK_ARG(d->ema_decay >= 0.f && d->ema_decay < 1.f, "%s: bad argument (ema: 0 <= ema_decay < 1)", who);
    if (d->gate) CRD_CHECK_ARG(d->ema_base >= 0, "%s: bad argument (ema with a gate: ema_base < 0)", who);
    else CRD_CHECK_ARG(d->ema_n >= (d->hp_dev ? 0 : 1), "%s: bad argument (ema without a gate: ema_n < 1)", who);
  }
  return CRD_OK;
}

extern "C" int crd_diffgradnorm_norm(const crd_dgn_desc* d, crd_stream_t stream) {
  if (int rc = dgn_check("crd_diffgradnorm_norm", d, false)) return rc;
  dgn_norm(*d, as_stream(stream));
  CRD_LAUNCH_CHECK("crd_diffgradnorm_norm");
  return CRD_OK;
}

extern "C" int crd_diffgradnorm_commit(const crd_dgn_desc* d, crd_stream_t stream) {
  if (int rc = dgn_check("crd_diffgradnorm_commit", d, true)) return rc;
  dgn_commit(*d, as_stream(stream));
  CRD_LAUNCH_CHECK("crd_diffgradnorm_commit");
  return CRD_OK;
}

extern "C" int crd_diffgradnorm_step(const crd_dgn_desc* d, crd_stream_t stream) {
  if (int rc = dgn_check("crd_diffgradnorm_step", d, true)) return rc;
  dgn_norm(*d, as_stream(stream));
  dgn_commit(*d, as_stream(stream));
  CRD_LAUNCH_CHECK("crd_diffgradnorm_step");
  return CRD_OK;
}

extern "C" int crd_swap_f32(float* a, float* b, int64_t n, crd_stream_t stream) {
  CRD_CHECK_ARG(n >= 0 && (n == 0 || (a && b)) && ((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0 &&
                    (n == 0 || a + n <= b || b + n <= a),
                "crd_swap_f32: bad argument (two non-overlapping fp32 buffers)");
  if (n == 0) return CRD_OK;
  long long head = (long long)(((16 - ((uintptr_t)a & 15)) & 15) / 4), nvec = 0;      // elements up to a's first 16-byte boundary
  if (head > n) head = n;
  if ((((uintptr_t)(b + head)) & 15) == 0) nvec = (n - head) / 4;
  else head = 0;                                                                      // a and b misaligned differently: one by one
  const long long work = nvec > n - 4 * nvec ? nvec : n - 4 * nvec;
  hipLaunchKernelGGL(k_swap_f32, dim3(blocks_for(work, TPB, 4096)), dim3(TPB), 0, as_stream(stream), a, b, (long long)n, head, nvec);
  CRD_LAUNCH_CHECK("crd_swap_f32");
  return CRD_OK;
}

extern "C" int crd_dropout_masks(float* out, const float* keep, int32_t rows, int32_t cols, uint64_t seed, uint64_t* counter,
                                 crd_stream_t stream) {
  CRD_CHECK_ARG(out && keep && counter && rows > 0 && cols > 0, "crd_dropout_masks: bad argument");
  hipLaunchKernelGGL(k_dropout_masks, dim3(blocks_for((long long)rows * cols, TPB, 64)), dim3(TPB), 0, as_stream(stream), out, keep, rows,
                     cols, (unsigned long long)seed, reinterpret_cast<unsigned long long*>(counter));
  hipLaunchKernelGGL(k_counter_inc, dim3(1), dim3(1), 0, as_stream(stream), reinterpret_cast<unsigned long long*>(counter));
  CRD_LAUNCH_CHECK("crd_dropout_masks");
  return CRD_OK;
}

extern "C" int crd_weight_pack(const crd_pack_entry* table_dev, int32_t n, int64_t max_elems, crd_stream_t stream) {
  CRD_CHECK_ARG(table_dev && n > 0 && max_elems > 0, "crd_weight_pack: bad argument");
  long long tiles = (max_elems + WP_CO * WP_ELEMS - 1) / (WP_CO * WP_ELEMS) * 2;      // padded tiles: about twice the dense count
  if (tiles < 1) tiles = 1;
  if (tiles > 96) tiles = 96;
  hipLaunchKernelGGL(k_weight_pack, dim3((unsigned)tiles, n), dim3(TPB), 0, as_stream(stream), table_dev);
  CRD_LAUNCH_CHECK("crd_weight_pack");
  return CRD_OK;
}

extern "C" int crd_wgrad_unpack(const crd_unpack_entry* table_dev, int32_t n, int64_t max_elems, int32_t accumulate,
                                crd_stream_t stream) {
  CRD_CHECK_ARG(table_dev && n > 0 && max_elems > 0, "crd_wgrad_unpack: bad argument");
  hipLaunchKernelGGL(k_wgrad_unpack, dim3(blocks_for(max_elems, TPB, 2048), n), dim3(TPB), 0, as_stream(stream), table_dev, accumulate);
  CRD_LAUNCH_CHECK("crd_wgrad_unpack");
  return CRD_OK;
}
