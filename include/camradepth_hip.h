/*
 * camradepth_hip.h -- C ABI of libcamradepth_hip.so (gfx950 / MI355X).
 *
 * The reference (TUMFTM/CamRaDepth) has no FFI or operator registry: its hot path is PyTorch ATen
 * calls made from Python modules.  This header is therefore the boundary a maintainer would bind
 * with ctypes to replace those calls.  Every entry point cites the reference code it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless named host_*.  The library never allocates, frees or
 *     synchronises; the caller owns every buffer and passes the HIP stream to enqueue on.
 *   - Return value: 0 = ok, negative = error (CRD_E_*); crd_last_error() gives a message
 *     (thread-local).  No exceptions cross the ABI.
 *   - Activations are "pixel-major" (NHWC): element (b,y,x,c) of a tensor lives at
 *     base[((b*H + y)*W + x)*ld + coff + c]; `ld` is the channel stride of the underlying buffer,
 *     so a producer can write into a channel slice of a wider buffer (this is how torch.cat of the
 *     reference disappears).  bf16 tensors need ld, coff and C to be multiples of 8 (16-byte rows).
 *   - The encoder's [B,C,N] tensors of the reference are the same layout with H*W = N.
 */
#ifndef CAMRADEPTH_HIP_H
#define CAMRADEPTH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* crd_stream_t; /* hipStream_t */

#define CRD_OK 0
#define CRD_E_INVALID (-1)     /* bad argument (null pointer, misaligned stride, ...) */
#define CRD_E_UNSUPPORTED (-2) /* shape outside what the kernels implement */
#define CRD_E_LAUNCH (-3)      /* HIP launch failure */

/* Order-independent sums.  Every accumulator that several workgroups add into -- GroupNorm statistics, per-channel sums,
 * loss / metric sums, the reduce sums of the GroupNorm backward, weight- and bias-gradient accumulators -- is a 64-bit
 * FIXED-POINT integer added to with integer atomics: integer addition is associative, so the result does not depend on
 * the order in which the workgroups arrive and two runs on the same inputs are bit-identical (fp32 atomics are not:
 * VERDICT r2 measured 1-3 % run-to-run spread downstream of them).  value = acc * 2^-FRAC_BITS.
 *   CRD_STAT_FRAC_BITS (20): forward statistics and loss sums -- range +-8.8e12, every partial rounded to 2^-21
 *     (<= 1e-9 absolute on a mean / mean square of >= 64 elements, against GroupNorm's eps = 1e-5);
 *   CRD_GRAD_FRAC_BITS (44): gradient-magnitude sums -- range +-5.2e5, partials rounded to 2^-45 (2.8e-14; operands are
 *     bf16, i.e. 4e-3 relative, and diffGradNorm's eps = 1e-8 swamps gradients below 1e-9).
 * Buffers of this type are zeroed by the caller (all-zero bits = 0.0). */
typedef int64_t crd_sum_t;
#define CRD_STAT_FRAC_BITS 20
#define CRD_GRAD_FRAC_BITS 44
/* NaN, infinity and magnitudes outside the range cannot be represented in a crd_sum_t.  A partial sum that is not finite, or
 * whose scaled magnitude reaches 2^62, adds NOTHING to its accumulator and raises a sticky device-side flag instead (a run
 * that has diverged would otherwise report a finite, too-small loss where the reference reports NaN, and bias / GroupNorm
 * gradients of 0 next to NaN weight gradients).  crd_nonfinite_status(reset, stream) runs its query ON `stream` -- behind every
 * kernel the caller enqueued there -- and waits for that stream; returns 1 if any such partial was dropped since the flag was last
 * cleared (0 if none, negative on error) and clears it when reset != 0.  reset == 2: clear only -- enqueued on `stream`, nothing is read
 * back, no wait, returns 0 (the eager model forward opens a step with it).  (Work on OTHER streams is ordered by the caller.)
 * TrainStep.losses(), the loss modules and camradepth_amd.lib.stat_checked() report NaN when it is set.  Sums whose TOTAL
 * leaves the range while every partial stays inside it still wrap (|statistic sum| > 8.8e12, |gradient sum| > 5.2e5). */
int crd_nonfinite_status(int32_t reset, crd_stream_t stream);
/* Device-side capture of the same flags (skip_nonfinite): ONE 64-thread launch on `stream`, no host read, legal inside a captured
 * graph.  ORs every translation unit's flag into a carry word and clears the flags; window_flag (optional, device int32) is ORed
 * with the result as well.  crd_nonfinite_status() ORs the carry word into what it reports and clears it with the flags, so what
 * the host sees is unchanged.  A training step calls it at the start of its backward (window_flag = NULL: what the forward's loss
 * sums dropped does not count) and at the end (window_flag = the window's verdict word). */
int crd_nonfinite_capture(int32_t* window_flag, crd_stream_t stream);

const char* crd_last_error(void);
#define CRD_ABI_VERSION 13       /* bumped whenever a struct layout or signature changes: the binding refuses a stale library */
int crd_version(void);          /* CRD_ABI_VERSION of the library that was built */
const char* crd_arch(void);     /* "gfx950" */

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on MFMA (bf16 in, fp32 accumulate).
 * Replaces torch conv1d/conv2d on the hot path: OverlapPatchEmbed.proj
 * (src/models/simplified_attention.py:158,185), Attention_MaxPool.{q,k,proj,sr} (:59-68,92-102),
 * Mlp.{fc1,fc2} (:17,20,35,41), ConvLayer conv (src/utils/utils.py:211,225), Depth_Activation
 * convs (utils.py:282-289) and the seg head convs (src/models/CamRaDepth.py:88-94), and -- with
 * gather_mode 1 / out_mode 1 -- their data gradients (autograd of the same calls).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x;      /* bf16 activations, pixel-major */
  int32_t x_ld, x_coff;
  int32_t B, IH, IW, Cin;       /* Cin multiple of 8 (pad channels must carry zero weights) */
  const void* w;      /* bf16 weights [Cout][KH*KW][Cin], tap index = ky*KW + kx */
  int32_t Cout, KH, KW, stride, pad;
  int32_t OH, OW;               /* output grid */
  int32_t gather_mode;          /* 0: y[oy,ox] += w[ky,kx] x[oy*s-p+ky, ox*s-p+kx]   (forward)
                                   1: y[iy,ix] += w[ky,kx] x[(iy+p-ky)/s, (ix+p-kx)/s] (data gradient) */
  void* y;            /* output, pixel-major */
  int32_t y_ld, y_coff;
  int32_t y_f32;                /* 0: bf16 output, 1: fp32 output */
  int32_t out_mode;             /* 0: y[b,oy,ox,n]; 1: patch scatter: n=(ky*pk+kx)*pc+c ->
                                   y[b, oy*pk+ky, ox*pk+kx, c] (data gradient of a k=s conv) */
  int32_t patch_k, patch_c;
  const float* bias;  /* [Cout] or NULL; element (b, co) is bias[b*bias_bstride + co] */
  int32_t bias_bstride;         /* 0: shared by all images; >0: one bias row per image */
  int32_t act;                  /* 0 none, 1 sigmoid */
  const float* res;   /* fp32, same indexing as y (ld = res_ld): y = res + res_scale[b]*v, or NULL */
  int32_t res_ld;
  const float* res_scale; /* [B] or NULL (=1) */
  int32_t accumulate;           /* 1: y += v (read-modify-write in y's dtype) */
  crd_sum_t* stats;   /* [B][Cout/16][2] += (sum, sum of squares) of the ROUNDED outputs (CRD_STAT_FRAC_BITS), or NULL */
  float* stats_partial;           /* optional scratch: per-tile partial sums are written here with plain stores and
                                     folded into `stats` by a small second kernel (avoids contended atomics) */
  int64_t stats_partial_capacity; /* floats available in stats_partial; needs B*ceil(OH*OW/64)*(Cout/16)*2 */
  /* Optional (red_x != NULL; bf16 output, no residual, Cout > 160, not the 3x3 halo shapes): this launch produces the dy
   * of a GroupNorm (+GELU) backward -- e.g. the data gradient of Mlp.fc2 feeding Mlp.norm2 -- and also computes that
   * backward's reduce phase: red_x is the GroupNorm's raw input (bf16, or fp32 with red_x_f32) laid out like y (pixel-major, red_x_ld channels per
   * pixel, same pixel grid), red_stats its g16 sums, red_gmul its slabs per group, red_act 1 for GELU; red_r is the
   * buffer crd_gn_bwd_reduce would fill (crd_sum_t [B*Cout*2 + B*(Cout/(16*red_gmul))*2], zeroed by the caller).  Only
   * crd_gn_bwd_apply remains to be called. */
  const void* red_x;
  int32_t red_x_ld, red_gmul, red_act, red_x_f32;   /* red_x_f32 = 1: red_x holds fp32 (the encoder's residual stream) */
  const crd_sum_t* red_stats;
  const float* red_gamma;
  const float* red_beta;
  crd_sum_t* red_r;            /* CRD_GRAD_FRAC_BITS */
  crd_sum_t* chan_sums;               /* optional, with stats and an fp32 or residual output: per-channel (sum, sumsq) of the
                                     stored output, crd_sum_t [B][Cout][2] (CRD_STAT_FRAC_BITS) (what crd_gn_stats'
                                     chan_sums would hold for the output tensor) */
} crd_conv_desc;

int crd_conv_igemm(const crd_conv_desc* d, crd_stream_t stream);
/* Which kernel crd_conv_igemm(d) would launch right now, as a NUL-terminated label (host arithmetic only: nothing is launched, no
 * device memory is read, no launch counter moves).  Runs the argument checks of crd_conv_igemm first: same status, same
 * crd_last_error(); a label that does not fit `capacity` bytes is CRD_E_INVALID.  The launch and this query share one decision
 * function and the kernels' own epilogue-branch conditions, and the crd_tune_* switches apply to both.
 *   hand-offs to another kernel family:  "conv3x3_halo", "conv3x3p", "pw_narrow", "pw_wide_plain" (their tile choice is not named)
 *   the generic kernel:  "k_igemm<WM,WN,TM,TN,MODE=m,NST=n,KG=g>/<epilogue>[+partials|+atomics]"
 *     tile = 32 WM TM rows x 32 WN TN columns; MODE 0 forward gather, 1 data gradient of a stride-1 layer, 2 strided data gradient;
 *     NST LDS stages; KG > 1 split-K groups inside the workgroup; epilogue = rege (register epilogue), vec (bf16, 16-byte stores
 *     through LDS), vecf (fp32 through LDS) or scalar (per lane); with d->stats, how the GroupNorm sums leave the workgroups:
 *     per-tile partial rows + a finalize launch, or atomics (also when stats_partial_capacity is too small for the chosen tile).
 * The tests pin the route of every case they mean to run through this (tests/test_conv_routes_cpu.py). */
int crd_conv_igemm_route(const crd_conv_desc* d, char* label, int32_t capacity);

/* The same convolution with a GroupNorm (+ exact GELU) applied to its INPUT while the A operand is loaded:
 *   y = epilogue( W * act( GroupNorm(x) ) ),   GroupNorm(x)[b,p,c] = (x - mean[b,g]) * rstd[b,g] * gamma[c] + beta[c]
 * -- nn.GroupNorm followed by Conv1d / Conv2d in Block / Attention_MaxPool / Mlp (simplified_attention.py:34-43 Mlp.norm2 +
 * GELU + fc2, :96-100 attn.sr behind Block.norm1 and attn.k behind attn.norm, :142-145 fc1 behind Block.norm2) without
 * the pass that would store the normalised tensor first.  d->x is the RAW tensor (fp32 when x_f32, else bf16); statistics
 * as raw sums per 16-channel slab, crd_sum_t [B][Cin/16][2] (what crd_gn_stats / a producer's `stats` epilogue leave), a
 * group being `gmul` consecutive slabs.  xn != NULL: act(GroupNorm(x)) is also stored as bf16 [B][IH*IW][xn_ld] (the
 * operand a later weight-gradient call needs).  Pointwise (1x1) and non-overlapping patch convolutions only
 * (KH == KW == stride, pad 0, gather_mode 0, out_mode 0); every epilogue option of crd_conv_desc except red_x and
 * stats_partial. */
typedef struct {
  int32_t x_f32;            /* d->x holds fp32 (1) or bf16 (0) */
  int32_t gmul;             /* 16-channel slabs per group */
  const crd_sum_t* stats;   /* [B][Cin/16][2] */
  const float* gamma;       /* [Cin] */
  const float* beta;        /* [Cin] */
  int32_t act;              /* 0 none, 1 exact GELU (after the affine) */
  int32_t xn_ld;
  void* xn;                 /* optional bf16 output */
} crd_gn_input;
int crd_gn_conv(const crd_conv_desc* d, const crd_gn_input* n, crd_stream_t stream);
/* Two crd_gn_conv problems of the same batch in ONE launch (round 6): attn.q and the attn.sr patch convolution of a Block, which both
 * read Block.norm1(x) (src/models/simplified_attention.py:96-100).  Both read the fp32 residual stream behind a GroupNorm without
 * activation and both take the 64 x 64 tiles; every option of crd_gn_conv applies to each (bias, output sums, n->xn). */
int crd_gn_conv2(const crd_conv_desc* d0, const crd_gn_input* n0, const crd_conv_desc* d1, const crd_gn_input* n1, crd_stream_t stream);
/* Backward twin of crd_gn_conv (round 6): the APPLY phase of a GroupNorm (+ exact GELU) backward folded into the A-operand load of
 * the pointwise data-gradient GEMM that consumes the gradient (csrc/xfgemm.hip).  d->x holds dy of the GroupNorm (bf16
 * [B][P][x_ld] + x_coff, Cin = the GroupNorm's channels); the GEMM multiplies d->w with
 *   dx = (gamma * g - S1 - xhat * S2) * rstd,  g = dy * mask * act'(xhat * gamma + beta)
 * -- what crd_gn_bwd_apply(x = gx, dy, stats, r) stores -- and the descriptor's epilogue options apply to the product (bias,
 * accumulate, out_mode = 1 patch scatter, stats, the fused reduce red_*).  Replaces crd_gn_bwd_apply + crd_conv_igemm in the backward
 * chain of an encoder Block: Mlp.norm1 in front of fc1's data gradient, attn.norm in front of the sr patch scatter (the autograd of
 * src/models/simplified_attention.py:38-41,96-100).  KH = KW = stride = 1, pad 0; bf16 output. */
typedef struct {
  const void* gx; int32_t gx_f32, gx_ld;   /* the GroupNorm's INPUT [B][P][gx_ld] from channel 0, bf16 or fp32 */
  int32_t gmul, act;                       /* group = gmul 16-channel slabs; act = 1: exact GELU behind the GroupNorm */
  const crd_sum_t* stats;                  /* forward slab sums of gx [B][Cin/16][2] */
  const float* gamma; const float* beta;   /* [Cin] */
  const float* mask;                       /* Dropout2d mask [B][Cin] or NULL */
  const crd_sum_t* r;                      /* crd_gn_bwd_reduce's sums: [B][Cin][2] then [B][Cin/(16 gmul)][2] */
  void* dx; int32_t dx_ld;                 /* optional: dx stored as bf16 [B][P][dx_ld] (what the weight gradients read), or NULL */
  float* dgamma; float* dbeta;             /* optional (both or neither): += the GroupNorm's parameter gradients */
} crd_gn_bwd_input;
int crd_gn_bwd_conv(const crd_conv_desc* d, const crd_gn_bwd_input* n, crd_stream_t stream);
/* 1 when crd_conv_igemm / crd_gn_conv send a 1x1 layer of this shape (input channels, output channels, pixels per sample) to the
 * narrow streaming kernel (round 5, csrc/pw_narrow.hip: Mlp.fc2 and the data gradient of Mlp.fc1 at encoder stages 1-2,
 * simplified_attention.py:17,20,35,41 -- hidden 512 / 1024 -> 64 / 128 channels): the weights of a workgroup's 16-column
 * slices live in registers, the hidden tensor streams through LDS once.  With crd_gn_conv (act = 1) Mlp.norm2 + the exact GELU
 * are applied to the rows on their way in and crd_gn_input.xn receives the activated tensor: callers use this to decide whether
 * the separate crd_gn_apply pass over the hidden tensor can be dropped. */
int crd_pw_narrow_supported(int32_t Cin, int32_t Cout, int32_t pixels);
/* Tuning / test knob of that kernel: on = 0 / 1 switches it off / on (2: on, and also for the K = 1024 launches without a GroupNorm
 * in front, which the generic tiles serve faster -- benchmarks only) for launches recorded from now on (returns the previous
 * setting; plans built before keep what they chose); on < 0: returns the number of launches that took the narrow kernel so far
 * (modulo 2^31) -- the tests use it to assert that the native kernel ran and not the generic tiles behind it. */
int crd_tune_pw_narrow(int32_t on);
/* Tuning knob of the 3x3 halo kernel: launches whose 128-column tiling would give fewer than `workgroups` workgroups use
 * 64- or 32-column tiles instead (default 512; 0 disables; < 0 restores the default).  Returns the previous value.
 * Not needed for correctness -- the tests use it to reach every tile configuration with small inputs. */
int crd_tune_conv3x3_small_grid(int workgroups);
/* Round 5: the 64 x 64-tile launches of crd_conv_igemm with a bf16 output in the plain layout (+ bias, sigmoid, accumulate, GroupNorm
 * sums, the fused GroupNorm-backward reduce) use a REGISTER epilogue (csrc/conv_common.h: conv_epilogue_reg -- swapped MFMA operands,
 * 16-byte stores straight from the accumulators, the epilogue's inputs prefetched at kernel start) instead of the LDS-staged one.
 * on = 0 / 1 switches it off / on for the following launches (returns the previous setting); on < 0 returns the number of launches
 * that took it so far (modulo 2^31).  Same results up to the summation order of the fused reduce's fp32 partials. */
int crd_tune_igemm_reg_epilogue(int32_t on);

/* ---- fp8 (OCP e4m3) inference path of the decoder's 3x3 ConvLayers (BASELINE.json config 5) ------------------------------
 * y = bf16( x_scale * w_scales[co] * sum_k x8[k] * w8[co][k] ) on the block-scaled MFMA (all block scales 2^0) at twice the
 * bf16 matrix rate.  d as for crd_conv_igemm with x = fp8 activations [B][IH*IW][x_ld] (1 byte per channel, Cin / x_ld /
 * x_coff multiples of 16) and w = fp8 weights [Cout][9][Cin]; 3x3 / stride 1 / pad 1 forward, plain bf16 output, optional
 * GroupNorm sums (stats + a stats_partial buffer of B x ceil(W/32) x ceil(H/16) x 4 x Cout/16 x 2 floats).  No reference
 * counterpart: the reference computes these convolutions under fp16 autocast (runner.py:191). */
int crd_conv3x3_fp8(const crd_conv_desc* d, const float* w_scales, float x_scale, crd_stream_t stream);
/* amax[0] = max(amax[0], max |x|) over channels [coff, coff + C) of a pixel-major bf16 tensor (atomic max on the float's
 * bits: amax must hold a non-negative float, e.g. 0).  Calibration of x_scale = amax / 448. */
int crd_amax_bf16(const void* x, int64_t rows, int32_t ld, int32_t coff, int32_t C, float* amax, crd_stream_t stream);
/* y[r][y_coff + c] = e4m3(clamp(x[r][coff + c] / scale, +-448)), round to nearest even; C, y_ld, y_coff multiples of 8 */
int crd_quant_fp8(const void* x, int64_t rows, int32_t ld, int32_t coff, int32_t C, void* y, int32_t y_ld, int32_t y_coff,
                  float scale, crd_stream_t stream);
/* Producers that write the e4m3 copy directly (what crd_quant_fp8 would make of their bf16 output: e4m3(bf16(v) / y_scale)):
 * GroupNorm(+GELU) of a ConvLayer (utils.py:210-228) and the decoder's 2x bicubic upsample (utils.py:249-257).  Arguments as
 * crd_gn_apply / crd_bicubic2x with y an fp8 tensor (y_ld, y_coff in bytes = channels).  y_bf16 (optional, NULL = none):
 * the bf16 output itself as well -- a training step keeps it for the backward pass. */
int crd_gn_apply_fp8(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                     int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask, void* y_fp8, int32_t y_ld,
                     int32_t y_coff, float y_scale, void* y_bf16, int32_t yb_ld, int32_t yb_coff, crd_stream_t stream);
int crd_bicubic2x_fp8(const void* x, int32_t x_ld, int32_t x_coff, int32_t B, int32_t H, int32_t W, int32_t C, void* y_fp8,
                      int32_t y_ld, int32_t y_coff, float y_scale, void* y_bf16, int32_t yb_ld, int32_t yb_coff, crd_stream_t stream);
/* per output channel: scales[co] = max |w[co]| / 448 (1 for an all-zero row), w_fp8[co][tap][c] = e4m3(w[co][tap][c] / scales[co])
 * for c < Cin and 0 for Cin <= c < Cin_out (crd_conv3x3_fp8 wants Cin_out % 16 == 0); w_bf16 is the packed forward weight
 * [Cout][taps][Cin] */
int crd_weight_quant_fp8(const void* w_bf16, int32_t Cout, int32_t taps, int32_t Cin, int32_t Cin_out, void* w_fp8, float* scales,
                         crd_stream_t stream);

/* ---- fp8 DATA GRADIENTS of the same ConvLayers (round 5; config 5 as a training step) ----------------------------------------
 * dx[b,iy,ix,ci] (+)= bf16( *x_scale_dev * w_scales[ci] * sum_{ky,kx,co} dy8[b, iy+1-ky, ix+1-kx, co] * w8[ci][ky*3+kx][co] ):
 * the autograd of crd_conv3x3_fp8's convolution w.r.t. its input (utils.py:211 under autograd), with dy = the GroupNorm
 * backward's output quantised to e4m3 (crd_gn_bwd_apply_fp8) and w8 = the packed data-gradient weights [Cin_pad][9][Cout_pad]
 * quantised per INPUT channel (crd_weight_quant_fp8 on crd_pack_entry.dst_dgrad).  d: gather_mode 1, x = dy8 (fp8, Cin here =
 * the layer's output channels rounded up to 16), w = w8, Cout = the channels of dx to produce (multiple of 8; 128-column tiles
 * + one narrower launch for the rest), accumulate 0 / 1 (dx's read-modify-write in bf16, as crd_conv_igemm), no statistics.
 * The activation scale is read from DEVICE memory (one float): it is this step's or the previous step's amax / 448
 * (crd_fp8_scale_update), never a host constant -- gradients shrink by orders of magnitude over a run. */
int crd_conv3x3_fp8_dgrad(const crd_conv_desc* d, const float* w_scales, const float* x_scale_dev, crd_stream_t stream);
/* crd_gn_bwd_apply (bf16 dx, no accumulation, no dx2) that ALSO writes dx_fp8 = e4m3(bf16(dx) / *scale_dev) and folds max |bf16(dx)|
 * into amax_slots[CRD_FP8_AMAX_SLOTS] (u32 max on the float's bits; one slot per workgroup, spread so that the atomics do not
 * serialise on one address).  The bf16 dx is still written: the weight gradient reads it. */
#define CRD_FP8_AMAX_SLOTS 64
int crd_gn_bwd_apply_fp8(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, const void* dy, int32_t dy_f32,
                         int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                         int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask,
                         const crd_sum_t* r, float* dgamma, float* dbeta, void* dx, int32_t dx_ld, int32_t dx_coff,
                         void* dx_fp8, int32_t dx8_ld, int32_t dx8_coff, const float* scale_dev, uint32_t* amax_slots,
                         crd_stream_t stream);
/* For each of n tensors: a = max over amax_slots[i][0..CRD_FP8_AMAX_SLOTS); if a > 0: scales[i] = margin * a / 448; the slots are
 * zeroed unless keep_slots.  Delayed scaling: called once per step at the head of the backward pass; with n = 1 right behind
 * crd_gn_bwd_apply_fp8 it is just-in-time scaling (the calibration iteration and the eager module path: followed by
 * crd_quant_fp8_dev).  Round 6: one scale per decoder STAGE (its three K-concatenated gradient slices): just-in-time updates behind the
 * first two layers keep the slots (running max), the third clears them. */
int crd_fp8_scale_update(uint32_t* amax_slots, float* scales, int32_t n, float margin, int32_t keep_slots, crd_stream_t stream);
/* crd_quant_fp8 with the scale read from device memory */
int crd_quant_fp8_dev(const void* x, int64_t rows, int32_t ld, int32_t coff, int32_t C, void* y, int32_t y_ld, int32_t y_coff,
                      const float* scale_dev, crd_stream_t stream);

/* Weight gradient of the same convolutions: dw[co][tap][ci] += sum_{b,oy,ox} dy[b,oy,ox,co] *
 * x[b, oy*s-p+ky, ox*s-p+kx, ci]  (fixed-point atomics, see crd_sum_t; caller zeroes dw).  Optionally also
 * dbias[co] += sum dy.  (autograd of the conv calls listed above.) */
typedef struct {
  const void* x; int32_t x_ld, x_coff; int32_t B, IH, IW, Cin;
  const void* dy; int32_t dy_ld, dy_coff; int32_t OH, OW, Cout;
  int32_t KH, KW, stride, pad;
  crd_sum_t* dw;      /* [Cout][KH*KW][Cin], CRD_GRAD_FRAC_BITS (untouched when dw_partials is used) */
  crd_sum_t* dbias;   /* [Cout] or NULL, CRD_GRAD_FRAC_BITS */
  float* dw_partials; /* optional, only where crd_conv_wgrad_splits(d) = S > 0 (the streaming 3x3 kernel): fp32
                         [S][Cout][9][Cin], contents don't-care.  Every pixel-range split stores its weight-gradient
                         block into its own copy with plain stores and dw is NOT touched: the gradient is the sum of the
                         S copies (crd_wgrad_unpack, replicas = S).  NULL: the splits add into dw with fp32 atomics. */
  int32_t dw_partial_capacity;   /* copies dw_partials holds.  It also CAPS the number of splits (= workgroups per channel
                                    chunk): the kernel uses min(natural split count, capacity) splits and writes exactly
                                    crd_conv_wgrad_splits(d) copies */
  int32_t wg_budget;             /* workgroups the streaming 3x3 kernel may use in total (0 = one per CU): a caller that runs
                                    other kernels next to this one passes fewer to leave them CUs.  The splits follow from it:
                                    budget / channel chunks, with a short last chunk (Cin = 136 / 144 / 200) given fewer
                                    workgroups and more rows each */
} crd_wgrad_desc;

/* Two kernel families serve this entry.  3x3 / stride 1 / pad 1 layers on grids of IW >= 32, IH >= 8 with Cout <= 128 go to the
 * streaming halo-row kernel (its widest instance stages and accumulates 128 output channels per workgroup: that is the limit);
 * everything else -- wider 3x3 layers included -- goes to the generic split-K kernel, which has no Cout limit but addresses the whole
 * batch with 32-bit byte offsets (CRD_E_UNSUPPORTED beyond).  Cin, x_ld, x_coff, dy_ld and dy_coff are multiples of 8; a dy row holds
 * Cout rounded up to 8 channels from dy_coff on (the channels of that round-up may hold anything: they are read, never stored). */
int crd_conv_wgrad(const crd_wgrad_desc* d, crd_stream_t stream);
/* Number of pixel-range splits the 3x3 streaming kernel uses for this problem (honouring d->dw_partial_capacity > 0 as
 * a cap), 0 if the generic kernel handles it (every layer of more than 128 output channels among them). */
int crd_conv_wgrad_splits(const crd_wgrad_desc* d);
/* Which kernel crd_conv_wgrad(d) would launch right now, as a NUL-terminated label (host arithmetic only: nothing is launched, no
 * device memory is read).  Runs the argument checks of crd_conv_wgrad first: same status, same crd_last_error(); a label that does
 * not fit `capacity` bytes is CRD_E_INVALID.  The launch and this query share the routing rule, the tile choice and the split planning.
 *   the generic kernel:    "k_wgrad<WM,WN,TM,TN>/splits=s,chunk=c"
 *     tile = 16 WM TM output channels x 128 (tap, ci) columns; s pixel-range splits (grid.z) of c pixels each, the last one shorter
 *   the streaming kernel:  "k_wgrad3x3<WCO,WCI,TCO,RPS>/S=s,rows_per_wg=r,chunks=n"
 *     16 WCO TCO output channels staged per row, RPS image rows per step; n 64-channel chunks of Cin x s row splits = workgroups,
 *     each split walking r consecutive strip rows (a strip = 32 columns of one image, B ceil(IW/32) IH strip rows in all).
 *     s is what crd_conv_wgrad_splits returns when dw_partials is given; d->dw_partial_capacity caps it only together with dw_partials.
 * A new entry, no changed signature: CRD_ABI_VERSION stays.  tests/test_wgrad_routes_cpu.py pins the route of every case it means to run. */
int crd_conv_wgrad_route(const crd_wgrad_desc* d, char* label, int32_t capacity);

/* Grouped weight gradients: the ~190 small wgrads of the encoder blocks (autograd's per-layer conv2d_backward weight
 * calls behind simplified_attention.py:32-43,95-132) are each too small to fill the chip, so the host collects them
 * per backward segment and runs them as ONE dispatch once their inputs exist.  crd_wgrad_group_build plans the group
 * on the host (problem descriptors + one work item per workgroup) into host_table; the caller copies the table to
 * device memory once and replays it with crd_conv_wgrad_grouped.  Calling build with host_table = NULL only fills
 * info->bytes (size query); a non-NULL table smaller than that is an error (CRD_E_INVALID).  The inputs named by the descriptors must stay valid until the grouped call.
 * Round 6: the items of a configuration are ordered for the 8 XCDs (workgroup index mod 8 = XCD): all tiles of one (problem, K split)
 * -- they re-read the same x and dy rows -- sit at indices of one residue, so the re-reads hit that XCD's L2; the list may contain
 * no-op items (problem index -1) where the XCDs' shares differ in length, and n_items counts them. */
typedef struct crd_wgrad_group_info {
  int32_t n_problems;
  int32_t n_items[4];      /* work items (workgroups) per tile configuration */
  int32_t item_offset[4];  /* first item of each configuration */
  int64_t bytes;           /* table size */
} crd_wgrad_group_info;
int crd_wgrad_group_build(const crd_wgrad_desc* descs, int32_t n, void* host_table, int64_t capacity,
                          crd_wgrad_group_info* info);
int crd_conv_wgrad_grouped(const void* dev_table, const crd_wgrad_group_info* info, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GroupNorm family.  Statistics are kept as raw sums over 16-channel slabs ("g16 stats":
 * crd_sum_t [B][C/16][2] = sum, sum of squares, CRD_STAT_FRAC_BITS); a GroupNorm group is `gmul` consecutive slabs, so
 * the reference's GroupNorm(C/16, C) has gmul = 1 and Mlp.norm2 (groups from out_features,
 * simplified_attention.py:24) has gmul = hidden/dim.  Replaces torch group_norm + GELU:
 * simplified_attention.py:23-24,37-40,70,117-118,142,144,162,186; utils.py:213-214,225.
 * ------------------------------------------------------------------------------------------- */
/* stats[b][c/16] += sums over pixels of x (bf16 or fp32); optional per-channel sums chan[b][c][2]. */
int crd_gn_stats(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t P, int32_t C,
                 crd_sum_t* stats, crd_sum_t* chan_sums, crd_stream_t stream);

/* y = act((x-mean)*rstd*gamma+beta) * mask[b][c];  act: 0 none, 1 exact GELU.  mask may be NULL.
 * y is a bf16 (y_f32=0) or fp32 (y_f32=1) pixel-major slice.  eps = 1e-5. */
int crd_gn_apply(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t P, int32_t C,
                 const crd_sum_t* stats, int32_t gmul, const float* gamma, const float* beta, int32_t act,
                 const float* mask, void* y, int32_t y_f32, int32_t y_ld, int32_t y_coff, crd_stream_t stream);

/* Backward, phase 1: per (b, c) sums  r[b][c] = (sum g, sum g*xhat), g = dy*mask*act'(u),
 * u = xhat*gamma+beta, followed by the per-group sums rg[b][grp] = (sum_c gamma_c r[b][c][0], sum_c gamma_c r[b][c][1]).
 * r is crd_sum_t[B*C*2 + B*(C/(16*gmul))*2] (CRD_GRAD_FRAC_BITS), zeroed by the caller.  dy is bf16 or fp32 pixel-major.
 * scratch (optional, >= B*1024*2*C floats is always enough): per-workgroup partial sums go there with plain stores and
 * a second small kernel folds them, instead of ~1M contended atomics on large tensors. */
int crd_gn_bwd_reduce(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, const void* dy, int32_t dy_f32,
                      int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                      int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask,
                      crd_sum_t* r, float* scratch, int64_t scratch_capacity, crd_stream_t stream);
/* Backward, phase 2: dgamma[c] += sum_b r[b][c][1], dbeta[c] += sum_b r[b][c][0];
 * dx = (gamma*g - mean_grp(gamma*g) - xhat*mean_grp(gamma*g*xhat)) * rstd, written as bf16
 * (dx_f32=0) or ADDED into an fp32 tensor (dx_f32=1, accumulate).  dx2 (optional): a bf16 copy [B][P][dx2_ld] of the
 * finished dx, scaled per sample by scale2[b] when scale2 is given (the drop-path-scaled gradient the previous block's
 * fc2 backward consumes, simplified_attention.py:144). */
int crd_gn_bwd_apply(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, const void* dy, int32_t dy_f32,
                     int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t P, int32_t C, const crd_sum_t* stats,
                     int32_t gmul, const float* gamma, const float* beta, int32_t act, const float* mask,
                     const crd_sum_t* r, float* dgamma, float* dbeta, void* dx, int32_t dx_f32, int32_t dx_ld,
                     int32_t dx_coff, int32_t dx_accumulate, void* dx2, int32_t dx2_ld, const float* scale2,
                     crd_stream_t stream);
/* The partition the two elementwise passes use for B samples of P pixels and C channels (host arithmetic, no GPU): kind 0 =
 * crd_gn_apply / crd_gn_apply_fp8, kind 1 = crd_gn_bwd_apply / crd_gn_bwd_apply_fp8.  Each sample is cut into *nblk workgroups of
 * *chunk pixels (the last takes what is left); *batch_pixels is what a workgroup's lanes request at once.  Grids that would
 * leave CUs idle get fewer pixels per lane; every other grid gets chunks that are whole batches, at most 2048 workgroups in all
 * (or B, if that is more).  The results of the passes do not depend on the partition; the tests pin through this entry which
 * edges of it a shape runs.  A new entry, no changed signature: CRD_ABI_VERSION stays. */
int crd_gn_launch_shape(int32_t P, int32_t C, int32_t B, int32_t kind, int32_t* nblk, int32_t* chunk, int32_t* batch_pixels);


/* ---------------------------------------------------------------------------------------------
 * Depthwise 3x3 (DWConv, simplified_attention.py:316,318-323), pixel-major bf16 [B][H][W][C].
 * w9 is fp32 [9][C] (tap-major), bias [C] or NULL.  flip=1 mirrors the taps (data gradient).
 * Optional g16 stats of the rounded output.
 * ------------------------------------------------------------------------------------------- */
int crd_dwconv3x3(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* w9, const float* bias,
                  int32_t flip, void* y, crd_sum_t* stats, const crd_sum_t* in_stats, int32_t in_gmul, const float* in_gamma,
                  const float* in_beta, const void* red_x, const crd_sum_t* red_stats, const float* red_gamma, crd_sum_t* red_r,
                  crd_stream_t stream);
/* red_x != NULL: the first phase of the backward of the GroupNorm (gmul = 1, no activation) whose dy this call produces
 * is fused in -- red_x is that GroupNorm's raw input (bf16 [B][H][W][C]), red_stats its g16 sums, red_gamma its weight,
 * red_r the buffer crd_gn_bwd_reduce would fill (crd_sum_t [B*C*2 + B*(C/16)*2], zeroed by the caller); only
 * crd_gn_bwd_apply remains to be called (Mlp.norm1's backward after the depthwise data gradient). */
/* in_stats != NULL (both functions): the input is GroupNorm-ed on load -- xn = bf16((x-mean)*rstd*gamma+beta) with the g16
 * sums in_stats[B][C/16][2] of x and groups of in_gmul slabs, zero padding applied after the normalisation -- i.e.
 * crd_gn_apply (Mlp.norm1, simplified_attention.py:37-38) fused into the consumer; the normalised tensor is never stored. */
/* dw10: crd_sum_t [replicas][10][C] (CRD_GRAD_FRAC_BITS), zeroed by the caller.  Rows 0..8: dw[tap][c] += sum dy*x_shifted; row 9: the bias
 * gradient sum dy.  Workgroups spread their atomics over the `replicas` copies (contended atomics on one copy
 * were the whole cost of this kernel); the true gradient is the sum of the copies (crd_wgrad_unpack does that). */
int crd_dwconv3x3_wgrad(const void* x, const void* dy, int32_t B, int32_t H, int32_t W, int32_t C, crd_sum_t* dw10,
                        int32_t replicas, const crd_sum_t* in_stats, int32_t in_gmul, const float* in_gamma,
                        const float* in_beta, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused Mlp of a Block (Block.forward / Mlp.forward, simplified_attention.py:34-43,141-145):
 *   x2 = x1 + dp * bf16( fc2( GELU( norm2( dwconv3x3( norm1( fc1( Block.norm2(x1) ) ) ) ) ) ) + b_fc2 )
 * for blocks whose Mlp.norm2 groups are exactly 64 hidden channels (hidden / (C / 16) == 64: ff_expansion 4, encoder stages
 * 3 and 4) and whose pixel grid fits in LDS (H * W <= 416): one workgroup per (sample, 64-channel slab of the hidden tensor)
 * runs the whole chain -- both GroupNorms are per sample and per slab, the depthwise conv per channel -- and leaves its fp32
 * contribution to fc2 in fc2_partials [hidden/64][B][H*W][C]; crd_mlp_reduce adds the slabs in order and finishes the
 * residual.  Two launches replace crd_gn_conv(fc1) + crd_dwconv3x3 + crd_gn_apply + crd_conv_igemm(fc2).
 * x1: fp32 residual stream [B][H*W][C] with its g16 sums x1_stats (Block.norm2's statistics); weights in the packed bf16
 * forms of crd_weight_pack (w_fc1 [hidden][C], w_fc2 [C][hidden]) and the depthwise fp32 [9][hidden] form.  Optional bf16
 * outputs (NULL = not stored; the backward pass and the weight gradients read them): xn = Block.norm2(x1) [B][H*W][C],
 * h1 = fc1 output, h2 = depthwise output, h3 = GELU(norm2(h2)), all [B][H*W][hidden].  h1_stats / h2_stats: their g16
 * sums [B][hidden/16][2], written with plain stores.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const float* x1; const crd_sum_t* x1_stats; const float* norm_gamma; const float* norm_beta;
  const void* w_fc1; const float* b_fc1; const float* norm1_gamma; const float* norm1_beta;
  const float* w9; const float* b_dw; const float* norm2_gamma; const float* norm2_beta;
  const void* w_fc2;
  void* xn; void* h1; void* h2; void* h3;
  crd_sum_t* h1_stats; crd_sum_t* h2_stats;
  float* fc2_partials;
  int32_t B, H, W, C, hidden;
} crd_mlp_desc;
/* number of 64-channel slabs (= first dimension of fc2_partials) if crd_mlp_fwd covers this shape, else 0 */
int crd_mlp_fused_supported(int32_t H, int32_t W, int32_t C, int32_t hidden);
int crd_mlp_fwd(const crd_mlp_desc* d, crd_stream_t stream);
/* x2 = x1 + dp[b] * bf16(sum_s fc2_partials[s] + b_fc2) (slabs added in order: reproducible; dp may be NULL = 1); optional
 * g16 sums `stats` [B][C/16][2] and per-channel sums `chan_sums` [B][C][2] of x2 (+=, the next block's norm1 statistics) */
int crd_mlp_reduce(const float* fc2_partials, int32_t slabs, const float* x1, const float* b_fc2, const float* dp, int32_t B,
                   int32_t N, int32_t C, float* x2, crd_sum_t* stats, crd_sum_t* chan_sums, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Max-pool attention (Attention_MaxPool.forward, simplified_attention.py:90-109).
 * q: bf16 [B][N][C], k: bf16 [B][M][C], C = heads*d.
 *   S[b][n] = sum_h max_m bf16(bf16(q_h.k_h)*scale)      idx[b][n][h] = argmax m
 * Since v = mean_n(x) is shared by all heads (:103) the output of `proj` is rank one:
 *   proj(out)[b][n][c] = u[b][c]*S[b][n] + bp[c],  u[b] = Wp xbar[b],  xbar = mean_n GroupNorm(x).
 * ------------------------------------------------------------------------------------------- */
int crd_attn_scores(const void* q, const void* k, int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d,
                    float scale, float* S, int16_t* idx, crd_stream_t stream);
/* Config 5 experiment (round 6; BASELINE.json configs[4] "fp8 MFMA attention"): crd_attn_scores on e4m3 operands
 * (v_mfma_scale_f32_32x32x64_f8f6f4, one K = 64 MFMA per 32-key tile).  q8 [B][N][heads][64], k8 [B][M][heads][64]: e4m3(x / scale) per
 * tensor, the head dimension zero-padded to 64 bytes (crd_quant_fp8 per head into a zeroed buffer); qk_scale = q_scale * k_scale;
 * s = max_m bf16(bf16(qk_scale * (q8 . k8)) * scale), outputs as crd_attn_scores.  Measured against the bf16 kernel and NOT used by the
 * plan (DESIGN.md "Round 6": the kernel is bound by the arg-max bookkeeping behind the MFMA, not by the MFMA or its operand bytes). */
int crd_attn_scores_fp8(const void* q8, const void* k8, int32_t B, int32_t N, int32_t M, int32_t heads, float qk_scale, float scale,
                        float* ssum, int16_t* idx, crd_stream_t stream);
/* crd_attn_scores and crd_attn_xbar_proj in ONE launch (the value path is one extra workgroup per sample; it only needs
 * norm1's sums, so it rides along with the scores): arguments as in the two calls, C = heads * d. */
int crd_attn_fwd(const void* q, const void* k, int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d, float scale,
                 float* S, int16_t* idx, const crd_sum_t* chan_sums, const crd_sum_t* stats, const float* gamma, const float* beta,
                 const void* w_fwd, void* xbar, float* u, crd_stream_t stream);
/* xbar[b][c] (bf16) from per-channel sums chan[b][c][2] and g16 stats of x (gmul = 1). */
int crd_attn_xbar(const crd_sum_t* chan_sums, const crd_sum_t* stats, const float* gamma, const float* beta, int32_t B,
                  int32_t N, int32_t C, void* xbar, crd_stream_t stream);
/* crd_attn_xbar followed by u[b][co] = sum_ci Wp[co][ci] * xbar[b][ci] (the `proj` Conv1d applied to the rank-one value,
 * simplified_attention.py:103-107) in one launch; w_fwd is Wp in its packed bf16 forward form [C][C].  u: fp32 [B][C]. */
int crd_attn_xbar_proj(const crd_sum_t* chan_sums, const crd_sum_t* stats, const float* gamma, const float* beta, const void* w_fwd,
                       int32_t B, int32_t N, int32_t C, void* xbar, float* u, crd_stream_t stream);
/* Backward of that path: tb = bf16(t) (bf16 [B][C], the dy operand of proj's weight gradient) and
 * es[b][ci] = inv_n * sum_co Wp[co][ci] * tb[b][co] (fp32 [B][C]); w_dgrad is Wp in its packed bf16 data-gradient form
 * [C][Cpad]. */
int crd_attn_vec_bwd(const crd_sum_t* t, const void* w_dgrad, int32_t B, int32_t C, int32_t Cpad, float inv_n, void* tb, float* es,
                     crd_stream_t stream);
/* x1 = x + dp[b]*bf16(u[b][c]*S[b][n] + bp[c])   (fp32 residual stream; Block.forward :143; dp may be NULL) */
int crd_attn_out_residual(const float* x, const float* u, const float* S, const float* bp, const float* dp,
                          int32_t B, int32_t N, int32_t C, float* x1, crd_stream_t stream);
/* crd_attn_out_residual that also accumulates the g16 GroupNorm sums of x1 (what crd_gn_stats(x1) would add to `stats`,
 * crd_sum_t [B][C/16][2], zeroed by the caller): Block.norm2 reads x1 next (simplified_attention.py:143-144). */
int crd_attn_out_residual_stats(const float* x, const float* u, const float* S, const float* bp, const float* dp,
                                int32_t B, int32_t N, int32_t C, float* x1, crd_sum_t* stats, crd_stream_t stream);
/* with dy = dp[b]*dx1:  t[b][c] += sum_n dy*S ; dbp_rows[b][c] += sum_n dy ; dS[b][n] = sum_c dy*u[b][c].
 * t and dbp_rows are crd_sum_t [B][C] (CRD_GRAD_FRAC_BITS), zeroed by the caller; the bias gradient is the sum of the B rows of dbp_rows: per-sample rows keep the
 * chain of contended atomics at the workgroups of one sample; crd_wgrad_unpack (replicas = B) folds them. */
int crd_attn_out_bwd(const float* dx1, const float* u, const float* S, const float* dp, int32_t B, int32_t N,
                     int32_t C, crd_sum_t* t, crd_sum_t* dbp_rows, float* dS, crd_stream_t stream);
/* The same with the apply phase of the preceding GroupNorm's backward fused in (Block.norm2, simplified_attention.py:144: gmul = 1,
 * no activation, fp32 input x = the residual stream, dxn = bf16 d(norm2(x)) from fc1's data gradient, r = the sums
 * crd_gn_bwd_reduce / the fused data-gradient epilogue left): first dx1 += crd_gn_bwd_apply(x, dxn) (written back: dx1 is the
 * residual gradient the block's backward continues with), then crd_attn_out_bwd on the result; dgamma / dbeta (both or neither)
 * += the GroupNorm's parameter gradients.  One launch and one pass over dx1 less per block. */
int crd_attn_out_bwd_gn(float* dx1, const float* u, const float* S, const float* dp, int32_t B, int32_t N, int32_t C,
                        crd_sum_t* t, crd_sum_t* dbp_rows, float* dS, const float* x, const void* dxn, const crd_sum_t* stats,
                        const float* gamma, const crd_sum_t* r, float* dgamma, float* dbeta, crd_stream_t stream);
/* Workgroups per sample of crd_attn_out_bwd / crd_attn_out_bwd_gn at this problem size (each takes ceil(N / that many)
 * consecutive pixels); 0 for B or N < 1.  Host arithmetic only, as crd_attn_scores_bwd_partials: the launchers use the same
 * rule, and the tests pin through it which geometry a shape runs.  A new entry, no changed signature: CRD_ABI_VERSION stays. */
int crd_attn_out_bwd_blocks(int32_t B, int32_t N, int32_t C);
/* dq[b][n][c] = scale*dS[b][n]*k[b][idx][c] (bf16) ; dk[b][m][c] += scale*dS*q (caller zeroes).
 * Every workgroup accumulates its share of dk in LDS (when [M][C] fp32 fits: always at the reference's sizes).  With
 * dk_partials != NULL (float [P][B][M][C], P = crd_attn_scores_bwd_partials(B,N,M,heads,d) > 0; contents don't-care)
 * the workgroups store their accumulators there with plain stores and dk is not touched: dk = sum over P, which
 * crd_sum_partials_bf16 folds together with the bf16 conversion the next layer needs.  With dk_partials == NULL they add
 * into dk (crd_sum_t [B][M][C], CRD_GRAD_FRAC_BITS) with atomics (2.7 M of them per launch at stage 1: ~16 us at the
 * ~170 G/s the L2s sustain).  Inside a workgroup the pixels routed to a key are found through a per-key bitmask and added
 * in ascending pixel order: the partials are reproducible bit for bit. */
int crd_attn_scores_bwd_partials(int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d);
int crd_attn_scores_bwd(const void* q, const void* k, const float* dS, const int16_t* idx, int32_t B, int32_t N,
                        int32_t M, int32_t heads, int32_t d, float scale, void* dq, crd_sum_t* dk, float* dk_partials,
                        crd_stream_t stream);
/* crd_attn_scores_bwd and crd_attn_vec_bwd in ONE launch (both consume crd_attn_out_bwd's outputs; one extra workgroup per
 * sample runs the vector path): arguments as in the two calls, C = heads * d. */
int crd_attn_bwd(const void* q, const void* k, const float* dS, const int16_t* idx, int32_t B, int32_t N, int32_t M,
                 int32_t heads, int32_t d, float scale, void* dq, crd_sum_t* dk, float* dk_partials, const crd_sum_t* t,
                 const void* w_dgrad, int32_t Cpad, float inv_n, void* tb, float* es, crd_stream_t stream);
/* dst[i] = bf16(sum_{r < replicas} part[r*replica_stride + i]), i < n (n, replica_stride multiples of 8) */
int crd_sum_partials_bf16(const float* part, int32_t replicas, int64_t replica_stride, void* dst, int64_t n,
                          crd_stream_t stream);
/* crd_attn_out_bwd (x == NULL) or crd_attn_out_bwd_gn (x != NULL: x, dxn, stats, gamma, r required, dgamma / dbeta both or neither,
 * C % 16 == 0) and the partial form of crd_attn_scores_bwd in ONE launch, without the round trip of dS through memory: a workgroup
 * runs the output backward on one of the score backward's pixel chunks, hands g = scale * dS to the score backward through LDS
 * and goes on with it.  Grid (P, B), P = crd_attn_scores_bwd_partials(B, N, M, heads, d); C = heads * d.
 *   dx1 (written with x != NULL only), dq and dk_partials (float [P][B][M][C], contents don't-care, every element stored) are bit
 * for bit what the two calls give; dS (float [B][N]) is too and may be NULL: it is then not stored.  t and dbp_rows (crd_sum_t
 * [B][C], zeroed by the caller) are fixed-point sums of per-workgroup float sums over P chunks instead of crd_attn_out_bwd_blocks
 * ones: reproducible from run to run, and equal to the two calls' to fp32 rounding.  The rank-one vector path (crd_attn_vec_bwd)
 * needs the complete t and is NOT part of this launch: crd_attn_dk_fold runs it.
 *   CRD_E_UNSUPPORTED, and nothing launched, exactly where crd_attn_bwd_fused_supported returns 0: P == 0 (the masks of a chunk do
 * not fit in LDS: the caller keeps the separate calls, whose fallback adds into a dk accumulator), C > 512 (crd_attn_out_bwd's
 * limit), or a chunk's LDS (q rows, g, masks and the 2 * C channel sums) above 128 KB.  A new entry, no changed signature:
 * CRD_ABI_VERSION stays. */
/* Does crd_attn_bwd_fused take this shape?  Its workgroups per sample (= crd_attn_scores_bwd_partials) or 0; host arithmetic only, the
 * rule the entry itself applies, so a caller that asks first is never refused for the shape. */
int crd_attn_bwd_fused_supported(int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d);
int crd_attn_bwd_fused(float* dx1, const float* u, const float* S, const float* dp, const void* q, const void* k, const int16_t* idx,
                       int32_t B, int32_t N, int32_t M, int32_t heads, int32_t d, float scale, crd_sum_t* t, crd_sum_t* dbp_rows,
                       float* dS, void* dq, float* dk_partials, const float* x, const void* dxn, const crd_sum_t* stats,
                       const float* gamma, const crd_sum_t* r, float* dgamma, float* dbeta, crd_stream_t stream);
/* crd_sum_partials_bf16(part, replicas, replica_stride, dst, n) and crd_attn_vec_bwd(t, w_dgrad, B, C, Cpad, inv_n, tb, es) in
 * ONE launch: B * ceil(C / 16) extra workgroups run the vector path.  The launch behind crd_attn_bwd_fused: t is complete when
 * it starts, and nothing reads tb / es before it.  dst, tb and es are bit for bit the two calls'.  A new entry: CRD_ABI_VERSION stays. */
int crd_attn_dk_fold(const float* part, int32_t replicas, int64_t replica_stride, void* dst, int64_t n, const crd_sum_t* t,
                     const void* w_dgrad, int32_t B, int32_t C, int32_t Cpad, float inv_n, void* tb, float* es, crd_stream_t stream);
/* dst[i] = bf16(src[i] * 2^-CRD_GRAD_FRAC_BITS), i < n (n a multiple of 8): the dk accumulator of crd_attn_scores_bwd's
 * global path as the bf16 operand the next layer needs */
int crd_gsum_to_bf16(const crd_sum_t* src, void* dst, int64_t n, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Bicubic x2 up-sampling, A=-0.75, align_corners=False, clamped borders (nn.Upsample, utils.py:241,
 * 251).  bf16 slice -> bf16 slice; the backward is the exact transpose.
 * ------------------------------------------------------------------------------------------- */
int crd_bicubic2x(const void* x, int32_t x_ld, int32_t x_coff, int32_t B, int32_t H, int32_t W, int32_t C, void* y,
                  int32_t y_ld, int32_t y_coff, crd_stream_t stream);
int crd_bicubic2x_bwd(const void* dy, int32_t dy_ld, int32_t dy_coff, int32_t B, int32_t H, int32_t W, int32_t C,
                      void* dx, int32_t dx_ld, int32_t dx_coff, int32_t accumulate, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient with respect to the model input (x.grad).  For every input pixel, c < Cin (fp32 NCHW dx [B][Cin][H][W], every
 * element written):
 *   dx[b][c][iy][ix] = sum_{co < 64, ky, kx: oy = (iy + 3 - ky) / 4, ox = (ix + 3 - kx) / 4 exact and in range}
 *                          draw[b][oy * W/4 + ox][co] * wpe[co][ky * 7 + kx][c]
 *                    + dcb_depth[b][iy * W + ix][col0 + c] (+ dcb_seg[b][iy * W + ix][col0 + c] when dcb_seg is not NULL)
 * i.e. the data gradient of the stage-0 patch embed (7x7, stride 4, pad 3, Cin -> 64) plus the x columns of the last decoder
 * stages' concat gradients.  draw: bf16 pixel-major [B][H/4 * W/4][64]; wpe: the forward-packed bf16 weight [64][49][8]
 * (channels >= Cin ignored); dcb_*: bf16 [B][H*W][dcb_ld], columns [col0, col0 + 8) read (those >= col0 + Cin ignored).
 * 1 <= Cin <= 8 and H, W multiples of 4 (CRD_E_UNSUPPORTED otherwise); draw, wpe, dcb_* and dx 16-byte aligned, col0 and dcb_ld
 * multiples of 8, col0 + 8 <= dcb_ld (CRD_E_INVALID).  No atomics: two identical calls give bit-identical dx.
 * ------------------------------------------------------------------------------------------- */
int crd_input_grad(const void* draw, const void* wpe, const void* dcb_depth, const void* dcb_seg, int32_t dcb_ld, int32_t col0,
                   int32_t B, int32_t H, int32_t W, int32_t Cin, float* dx, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Layout / small elementwise helpers at the module boundary.
 * ------------------------------------------------------------------------------------------- */
/* NCHW fp32 [B][C][H][W] -> pixel-major bf16 slice; channels C..Cpad-1 of the slice are zeroed. */
int crd_nchw_to_pm(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, void* y, int32_t y_ld, int32_t y_coff,
                   int32_t Cpad, crd_stream_t stream);
/* pixel-major (bf16 or fp32) -> NCHW fp32 */
int crd_pm_to_nchw(const void* x, int32_t x_f32, int32_t x_ld, int32_t x_coff, int32_t B, int32_t C, int32_t H,
                   int32_t W, float* y, crd_stream_t stream);
/* Seg_Block (utils.py:95-100): y[row*y_ld + y_coff] = argmax_c logits[row][c] / num_classes (first max wins);
 * y is bf16 (y_f32=0, a channel of a pixel-major buffer) or fp32 (y_f32=1, the module output) */
int crd_seg_argmax(const void* logits, int32_t ld, int32_t B, int32_t P, int32_t C, int32_t num_classes, void* y,
                   int32_t y_f32, int32_t y_ld, int32_t y_coff, crd_stream_t stream);
/* dst[i] = scale * src[i]  (fp32) */
int crd_scale_f32(const float* src, float* dst, int64_t n, float scale, crd_stream_t stream);
/* dst[row][d_coff+c] (+)= src[row][s_coff+c]   (bf16 slices) */
int crd_slice_copy(const void* src, int32_t s_ld, int32_t s_coff, void* dst, int32_t d_ld, int32_t d_coff,
                   int64_t rows, int32_t C, int32_t accumulate, crd_stream_t stream);
/* dst[row][d_coff+c] = bf16(scale[row / rows_per_sample] * src[row*s_ld + c] + add[row][add_coff+c]), c < C
 * (scale and add may be NULL; add is a bf16 slice) */
int crd_f32_to_bf16_rows(const float* src, int32_t s_ld, void* dst, int32_t d_ld, int32_t d_coff, int64_t rows,
                         int32_t C, const float* scale, int64_t rows_per_sample, const void* add, int32_t add_ld,
                         int32_t add_coff, crd_stream_t stream);
/* Depth_Activation.conv_2 (utils.py:283,288): 3x3 conv 32 -> 1 (+bias) as a stencil-reduce.  a: bf16 [B][H][W][32]
 * (the sigmoid output), w: fp32 reference layout [1][32][3][3], depth: fp32 [B][H][W]; `copy` (optional) receives
 * the bf16 depth as one channel of a pixel-major buffer (the reference's torch.cat([stage, depth]), CamRaDepth.py:120,146). */
int crd_head_conv2_fwd(const void* a, const float* w, const float* bias, int32_t B, int32_t H, int32_t W, float* depth,
                       void* copy, int32_t copy_ld, int32_t copy_coff, crd_stream_t stream);
/* Backward of the above fused with the sigmoid backward: dy = gd (+ add, a bf16 channel);
 * dz = a(1-a) * conv2^T(dy) (bf16 [B][H][W][32]).  Parameter gradients: dw_rows is crd_sum_t [replicas][289] (CRD_GRAD_FRAC_BITS), zeroed by the
 * caller; every row holds dw[1][32][3][3] (288 values, reference order) followed by dbias, workgroups spread their
 * fp32 atomics over the rows and the gradient is the sum of the rows (crd_wgrad_unpack, replicas = rows). */
int crd_head_conv2_bwd(const float* gd, const void* add, int32_t add_ld, int32_t add_coff, const void* a, const float* w,
                       int32_t B, int32_t H, int32_t W, void* dz, crd_sum_t* dw_rows, int32_t replicas, crd_stream_t stream);
/* The two halves of crd_head_conv2_bwd as calls of their own (the weight-gradient half is not on the backward pass's
 * dependency chain: the graph step replays it on its late stream). */
int crd_head_conv2_bwd_data(const float* gd, const void* add, int32_t add_ld, int32_t add_coff, const void* a, const float* w,
                            int32_t B, int32_t H, int32_t W, void* dz, crd_stream_t stream);
int crd_head_conv2_wgrad(const float* gd, const void* add, int32_t add_ld, int32_t add_coff, const void* a, int32_t B, int32_t H,
                         int32_t W, crd_sum_t* dw_rows, int32_t replicas, crd_stream_t stream);
/* da <- da * a * (1-a)   (bf16, n elements, n % 8 == 0): backward of the sigmoid in Depth_Activation */
int crd_sigmoid_bwd(const void* a, void* da, int64_t n, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Weight packing: fp32 reference layout [Cout][Cin_ref][taps] -> bf16 [Cout][taps][Cin_pad]
 * and the two transposed forms the data-gradient kernels read; table-driven, one launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const float* src;    /* [Cout][Cin_ref][taps] fp32 (reference layout) */
  void* dst_fwd;       /* bf16 [Cout][taps][Cin_pad]      or NULL */
  void* dst_dgrad;     /* bf16 [Cin_pad][taps][Cout_pad]  or NULL   (gather_mode 1) */
  void* dst_scatter;   /* bf16 [taps][Cin_pad][Cout_pad]  or NULL   (out_mode 1)    */
  const int32_t* cmap; /* [Cin_pad]: reference input channel of each packed channel, -1 = zero; NULL = identity */
  int32_t Cout, Cin_ref, taps, Cin_pad, Cout_pad;
  int32_t dst_f32;     /* 1: dst_fwd is written as fp32 (plain copies of vectors); 2: fp32 holding the bf16-ROUNDED value (depthwise
                          weights [9][C]: what autocast feeds the convolution -- the reference casts conv weights to the low
                          precision, src/main/runner.py:191) */
  /* Round 6: K-CONCATENATED data-gradient weights (the write-once data gradients of a ShortResBlock, src/utils/utils.py:127-135 under
   * autograd: dx[n] of the concat buffer = sum over the layers that read channel n).  dgrad_ld > 0: dst_dgrad is a matrix
   * [rows][taps][dgrad_ld] shared by several layers; this entry writes its Cout_pad columns at column offset dgrad_coff for the input
   * channels [dgrad_row0, dgrad_row0 + dgrad_rows) as rows 0 .. dgrad_rows - 1.  dgrad_ld == 0: the plain form above. */
  int32_t dgrad_ld, dgrad_coff, dgrad_row0, dgrad_rows;
} crd_pack_entry;
int crd_weight_pack(const crd_pack_entry* table_dev, int32_t n, int64_t max_elems, crd_stream_t stream);
/* grad_ref[co][ci_ref][tap] (+)= dw_packed[co][tap][ci_pad] */
typedef struct {
  const void* src;     /* [Cout][taps][Cin_pad]: fp32 (src_sum = 0) or crd_sum_t with CRD_GRAD_FRAC_BITS (src_sum = 1) */
  float* dst;          /* fp32 [Cout][Cin_ref][taps] */
  const int32_t* cmap;
  int32_t Cout, Cin_ref, taps, Cin_pad;
  int32_t replicas;        /* > 1: the source is the sum of `replicas` copies, replica_stride ELEMENTS apart (summed in
                              index order: fixed, so reproducible) */
  int32_t src_sum;
  int64_t replica_stride;
} crd_unpack_entry;
int crd_wgrad_unpack(const crd_unpack_entry* table_dev, int32_t n, int64_t max_elems, int32_t accumulate,
                     crd_stream_t stream);

/* Train-mode masks of timm DropPath (simplified_attention.py:123,143-144) and nn.Dropout2d
 * (CamRaDepth.py:96): out[r][c] = Bernoulli(keep[r]) / keep[r].  *counter (device) is advanced by
 * the call so that a replayed HIP graph draws new masks. */
int crd_dropout_masks(float* out, const float* keep, int32_t rows, int32_t cols, uint64_t seed, uint64_t* counter,
                      crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Batch assembly (NuscenesDataset.__getitem__, src/data/dataloader.py:202-333) -- SURVEY 8f N1.
 * ------------------------------------------------------------------------------------------- */
/* out: fp32 [B][7 or 6][H][W].  Channels 0-2: (img/255 - mean)/std of the uint8 [B][H][W][3] image in the order it was
 * read (cv2 BGR; the reference applies the RGB ImageNet constants as is, :226-233); 3: clip(radar[...,0], 0, max_depth) /
 * max_depth (:304-306); 4-5: radar[...,1..2] (:309-310); 6: rad_vel (:315-318; NULL -> 6 channels).  radar: fp32
 * [B][H][W][3], rad_vel: fp32 [B][H][W]. */
int crd_assemble_input(const void* img_u8, const float* radar, const float* rad_vel, int32_t B, int32_t H, int32_t W,
                       float max_depth, float* out, crd_stream_t stream);
/* Ground-truth pyramid (:236-257): full = inverse-normalised depth (clip to [0, max], g > 0 -> (max - g)/max); half,
 * quarter, eighth = successive zero-ignoring 3x3 / stride 2 / pad 1 min-pools (:213-222); lower levels may be NULL. */
int crd_gt_pyramid(const float* depth, int32_t B, int32_t H, int32_t W, float max_depth, float* full, float* half,
                   float* quarter, float* eighth, crd_stream_t stream);
/* cv2.resize(image, (DW, DH), interpolation=cv2.INTER_NEAREST) of dataloader.py:227 on interleaved uint8 pixels
 * [B][SH][SW][C] -> [B][DH][DW][C]: source column = min(floor(dx * (1 / (DW / SW))), SW - 1) in double, rows alike. */
int crd_resize_nearest_u8(const void* src, int32_t B, int32_t SH, int32_t SW, int32_t C, void* dst, int32_t DH, int32_t DW,
                          crd_stream_t stream);
/* The segmentation targets of dataloader.py:262-267: skimage.transform.resize(mseg[:rows], (DH, DW), order=0,
 * preserve_range=True, anti_aliasing=False) (scikit-image 0.19.3 -> scipy.ndimage.zoom(order=0, grid_mode=True)): source
 * index = floor(((o + 0.5) * (S / D) - 0.5) + 0.5) in double.  uint8 [B][SH][SW] label maps in, of which the first
 * `rows` rows are used; int64 [B][DH][DW] labels out (the dtype runner.py:189-190 casts to). */
int crd_resize_labels_nearest(const void* src_u8, int32_t B, int32_t SH, int32_t SW, int32_t rows, int64_t* dst, int32_t DH,
                              int32_t DW, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Batch augmentation on the device: random crop, horizontal flip, photometric jitter of the image.  The reference trains
 * without augmentation, so these entries are defined here ("Augmentation").
 *
 * params: int32 [B][CRD_AUGMENT_WORDS], one row per sample:
 *   0 y0   1 x0   2 flip (0 / 1)      int32
 *   3 gamma   4 brightness   5..7 colour gain of the stored channels 0..2      fp32 bit patterns
 * Geometry: output pixel (y, x) of sample b reads source pixel (y0 + y, x0 + (flip ? w - 1 - x : x)) of every tensor.  The kernels
 * clamp y0 into [0, H - h] and x0 into [0, W - w], so no table makes them read outside the frame.  A flipped sample gets radar
 * channel 4 (u = (x - cx) / f, mirrored with the camera) written as v == 0 ? 0 : -v; channel 5 is untouched.
 * (h, w) is the whole frame, or a crop whose sides are multiples of 32.
 * ------------------------------------------------------------------------------------------- */
#define CRD_AUGMENT_WORDS 8
/* The augmentation stream: crd_augment_draw hashes with seed ^ CRD_AUGMENT_STREAM, so that equal user seeds for dropout and
 * augmentation give unrelated draws.  Element i = b * 8 + k of the draw (seed, counter):
 *   hash = splitmix64(splitmix64((seed ^ CRD_AUGMENT_STREAM) ^ counter * 0xD1342543DE82EF95) + i),  t = hash >> 40,  u = t * 2^-24
 *   y0 = (t * (H - h + 1)) >> 24,  x0 = (t * (W - w + 1)) >> 24,  flip = u < p_flip,
 *   gamma / brightness / colour = lo + u * (hi - lo), each product and sum rounded to fp32 on its own
 * -- the generator of crd_dropout_masks.  The slots are fixed: a transform that is switched off (its bit in `enable` clear) writes
 * 1.0 and leaves the other words as they are.  counter is a HOST integer (assembly runs outside the captured step). */
#define CRD_AUGMENT_STREAM 0xA0761D6478BD642Full
#define CRD_AUGMENT_GAMMA 1
#define CRD_AUGMENT_BRIGHTNESS 2
#define CRD_AUGMENT_COLOUR 4
/* Writes params and, when lut != NULL, the table of crd_augment_lut for it. */
int crd_augment_draw(int32_t* params, float* lut, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w, float p_flip,
                     float gamma_lo, float gamma_hi, float brightness_lo, float brightness_hi, float colour_lo, float colour_hi,
                     int32_t enable, uint64_t seed, uint64_t counter, crd_stream_t stream);
/* lut: fp32 [B][3][256], the normalised image value of byte v in stored channel c of sample b, all in fp32:
 *   t = v / 255;  t = powf(t, gamma) (gamma enabled);  t *= brightness (enabled);  t *= colour[c] (enabled);  t = min(max(t, 0), 1);
 *   lut = (t - mean[c]) / std[c]          with the constants of crd_assemble_input
 * With nothing enabled this is crd_assemble_input's own expression. */
int crd_augment_lut(const int32_t* params, int32_t B, int32_t enable, float* lut, crd_stream_t stream);
/* crd_assemble_input + the full level of crd_gt_pyramid + the label gather in one launch, cropped and flipped by params, the image
 * through lut.  seg_u8: uint8 labels [B][H][W] or NULL; final_seg: int64 [B][h][w]; inter_seg (optional): int64 [B][h/2][w/2],
 * inter_seg[y][x] = final_seg[2y + 1][2x + 1] (skimage order 0 at a halving, crd_resize_labels_nearest).  out: fp32
 * [B][7 or 6][h][w] (rad_vel NULL -> 6), gt_full: fp32 [B][h][w]. */
int crd_augment_assemble(const void* img_u8, const float* radar, const float* rad_vel, const float* depth, const void* seg_u8,
                         const int32_t* params, const float* lut, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w,
                         float max_depth, float* out, float* gt_full, int64_t* final_seg, int64_t* inter_seg,
                         crd_stream_t stream);
/* The geometry alone, for tensors that are assembled already: image fp32 [B][C][H][W] -> [B][C][h][w] (channel 4 negated on flipped
 * samples when C >= 6), gt_full fp32 [B][H][W] -> [B][h][w], seg int64 [B][H][W] or NULL -> seg_out [B][h][w] and (optional)
 * inter_out [B][h/2][w/2]. */
int crd_augment_gather(const float* image, const float* gt_full, const int64_t* seg, const int32_t* params, int32_t B, int32_t C,
                       int32_t H, int32_t W, int32_t h, int32_t w, float* image_out, float* gt_out, int64_t* seg_out,
                       int64_t* inter_out, crd_stream_t stream);
/* The min-pool levels of crd_gt_pyramid from a full map that is inverse-normalised already (an augmented one: the levels are rebuilt
 * from it, never cropped or flipped themselves -- with an even width the 3x3 / stride 2 / pad 1 windows are not mirror-symmetric). */
int crd_gt_pyramid_from_full(const float* full, int32_t B, int32_t H, int32_t W, float* half, float* quarter, float* eighth,
                             crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Radar front end: accumulated radar sweeps -> the radar [B][H][W][3] and rad_vel [B][H][W] maps of crd_assemble_input.  The
 * reference makes them offline (lib/fuse_radar.py, driven by scripts/cal_radar.py and scripts/show_v_comp.py); a live pipeline
 * needs them per frame ("Radar front end").  All arithmetic is fp64.  Every fp64 quantity is passed through device
 * memory.  Neither entry allocates or synchronises; both may be captured in a graph.
 *
 * Points of all frames lie in one array; frame b owns the points frame_offsets[b] .. frame_offsets[b + 1] - 1 (int32 [B + 1] on the
 * device, non-decreasing; an empty frame repeats a value).  A point outside every range is invalid (project) / skipped (rasterize),
 * so a captured call sized for n_points can be replayed with fewer.  K: row-major 3x3 intrinsics, one matrix for all frames
 * (k_stride 0) or one per frame (k_stride 9); fx = K[0], cx = K[2], fy = K[4], cy = K[5].
 * ------------------------------------------------------------------------------------------- */
/* The projection nested in merge_selected_radar (fuse_radar.py:30-74, :144-151).  points: fp64 [n_points][5] = x, y, z, vx_comp,
 * vy_comp in the radar sensor frame; sweep_index: int32 [n_points], the row of the point's sweep in the per-sweep tables
 * cam1_from_sensor / cam2_from_sensor (fp64 [n_sweeps][3][4], the pose chain sensor -> car -> global -> car -> camera multiplied by
 * the caller) and lags (fp64 [n_sweeps][2]: camera time minus sweep time in seconds for camera 1 and 2, signed).  Per camera c:
 *   xs = x + vx_comp * lag_c,  ys = y + vy_comp * lag_c,  (X, Y, Z) = M_c . (xs, ys, z, 1),
 *   px_c = (fx * X + cx * Z) / Z,  py_c = (fy * Y + cy * Z) / Z
 * valid = not (|x| < min_distance and |y| < min_distance) and, for both cameras, Z_c >= min_z, 0 < px_c < im_w, 0 < py_c < im_h;
 * a NaN, a sweep_index outside the tables or a point outside every frame gives valid = 0.  Outputs, over all points in their order
 * (nothing is compacted: the rasteriser's tie rule is by index): x1, y1, depth1 = Z_1, x2, y2, v_comp = sqrt(vx_comp^2 + vy_comp^2). */
int crd_radar_project(const double* points, const int32_t* sweep_index, const int32_t* frame_offsets, int32_t B, int32_t n_points,
                      const double* cam1_from_sensor, const double* cam2_from_sensor, const double* lags, int32_t n_sweeps,
                      const double* K, int32_t k_stride, int32_t im_h, int32_t im_w, float min_distance, float min_z, double* x1,
                      double* y1, double* depth1, double* x2, double* y2, double* v_comp, uint8_t* valid, crd_stream_t stream);
/* cal_depthMap_flow (:156-204) + radarFlow2uv (:276-303).  h_new = im_h / s, w_new = im_w / s (integer division, s =
 * downsample_scale).  Per point with valid != 0 (valid NULL: every point): xa = clip((x1 + 0.5) / s - 0.5, 0, w_new - 1), ya, xb, yb
 * alike from y1, x2, y2; its pixel is (rint(ya), rint(xa)), half to even.  A pixel goes to its point of smallest depth1 (compared as
 * fp64), the lowest index among equal depths -- what the reference's loop leaves -- independent of the order of arrival.  Rows above
 * y_cutoff are dropped: output row r is map row r + y_cutoff.  At the winner i of output pixel (r, c):
 *   radar[b][r][c] = (depth1[i], u, v),  rad_vel[b][r][c] = v_comp[i] > 0.5
 *   xm = fp32(c + (xb - xa)),  ym = fp32(r + (yb - ya))          (one rounding of the fp64 sum)
 *   u = (xm - cx / s) / (fx / s),  v = (ym - (cy / s - y_cutoff)) / (fx / s)          (fx in both, as the reference)
 * rounded to fp32; every other pixel is 0.  A point with a non-finite x1, y1, depth1, x2, y2 or v_comp, or depth1 <= 0, is skipped
 * (the reference raises on NaN coordinates and treats a zero depth as an empty pixel).  The time and RCS maps are not produced.
 * radar: fp32 [B][h_new - y_cutoff][w_new][3], rad_vel: fp32 [B][h_new - y_cutoff][w_new], both written in full.  workspace: n_pix =
 * B * (h_new - y_cutoff) * w_new winners (uint32) and, from the next multiple of 16 bytes, n_pix depth keys (uint64);
 * workspace_bytes >= ((4 * n_pix + 15) & ~15) + 8 * n_pix.  workspace, radar and rad_vel are 16-byte aligned. */
int crd_radar_rasterize(const double* x1, const double* y1, const double* depth1, const double* x2, const double* y2,
                        const double* v_comp, const uint8_t* valid, const int32_t* frame_offsets, int32_t B, int32_t n_points,
                        const double* K, int32_t k_stride, int32_t im_h, int32_t im_w, int32_t downsample_scale, int32_t y_cutoff,
                        void* workspace, int64_t workspace_bytes, float* radar, float* rad_vel, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Lidar ground-truth front end: accumulated lidar sweeps -> the gt_depth [B][H][W] map of crd_gt_pyramid / crd_augment_assemble, with
 * the flow (u, v) and low-height mask the reference stores beside it.  The reference makes them offline (lib/fuse_lidar.py, driven by
 * scripts/cal_gt.py) in a Python loop over about a million points per key frame ("Lidar ground-truth front end").
 * The conventions are the radar front end's: fp64 arithmetic, fp64 quantities through device memory or as IEEE-754 bit patterns
 * (uint64_t ..._f64_bits), frame_offsets, K / k_stride, no allocation, no synchronisation, capturable in a graph on one stream.  The
 * two entries add no struct and change no signature: CRD_ABI_VERSION stays.
 * ------------------------------------------------------------------------------------------- */
/* current_to_global_at_ref_time + proj2im (fuse_lidar.py:84-179), the pose chains multiplied by the caller.  points: fp64
 * [n_points][3] in the lidar sensor frame; sweep_index: int32 [n_points], the row s of the point's sweep in
 *   cam1_from_sensor, cam2_from_sensor  fp64 [n_sweeps][3][4]   sensor -> car -> global -> car -> camera 1 / 2
 *   car_z_from_sensor                   fp64 [n_sweeps][4]      the z row of car-from-sensor (the height mask)
 *   sweep_boxes                         int32 [n_sweeps + 1]    sweep s owns the box entries sweep_boxes[s] .. sweep_boxes[s + 1] - 1
 * A box entry e is a box that exists at the sweep's time and at the camera times, in the reference's iteration order (:118-119):
 *   box_entries[e]  fp64 [15] = box_from_sensor [3][4] (the box frame at the sweep's time), then the half extents l/2, w/2, h/2
 *   box_id[e]       int32, the row k of the box in cam1_from_box / cam2_from_box (fp64 [n_boxes][3][4]: camera c from the box's pose
 *                   at camera c's time) and vehicle (uint8 [n_boxes], non-zero: 'vehicle' is in the category name, :153)
 * Per point p = (x, y, z) of sweep s:
 *   z_car = car_z . (x, y, z, 1);  low_h = h_min <= z_car <= h_max                                        (:47-56, :109)
 *   q_e = box_from_sensor_e . (x, y, z, 1);  the point belongs to the FIRST entry e of its sweep with |q_e.x| < l/2, |q_e.y| < w/2,
 *   |q_e.z| < h/2, all six strict (:132-137) -- the reference takes a box's points out of the pool before it tests the next box
 *   (X, Y, Z)_c = cam_c_from_box[k] . (q_e, 1) for a box point, cam_c_from_sensor[s] . (x, y, z, 1) for any other
 *   px_c = (fx * X + cx * Z) / Z,  py_c = (fy * Y + cy * Z) / Z;  in_box = the point is in a box and vehicle[k]
 *   valid = not (|x| < min_distance and |y| < min_distance) and, for both cameras, Z_c >= min_z, 0 < px_c < im_w, 0 < py_c < im_h
 * A NaN fails every test.  A point outside every frame, with a sweep_index outside the tables or in an entry whose box_id is outside
 * [0, n_boxes) gives zeros, valid = low_h = in_box = 0 and box_entry = -1, and none of its tables is read.  Outputs over all points in
 * their order (nothing is compacted: the tie rule of crd_lidar_ground_truth is by index): x1, y1, depth1 = Z_1, x2, y2 (fp64), low_h,
 * in_box, valid (uint8), box_entry (int32: the entry e the point belongs to, or -1).
 * Not the reference's: it keeps points as float32 and rounds after every transform (the devkit's LidarPointCloud), here the chain
 * stays fp64; it moves box points behind the others (:157), here the order is the input's (it only decides exact fp64 depth ties). */
int crd_lidar_project(const double* points, const int32_t* sweep_index, const int32_t* frame_offsets, int32_t B, int32_t n_points,
                      const double* cam1_from_sensor, const double* cam2_from_sensor, const double* car_z_from_sensor,
                      const int32_t* sweep_boxes, int32_t n_sweeps, const double* box_entries, const int32_t* box_id, int32_t n_entries,
                      const double* cam1_from_box, const double* cam2_from_box, const uint8_t* vehicle, int32_t n_boxes,
                      const double* K, int32_t k_stride, int32_t im_h, int32_t im_w, float min_distance, float min_z,
                      uint64_t h_min_f64_bits, uint64_t h_max_f64_bits, double* x1, double* y1, double* depth1, double* x2, double* y2,
                      uint8_t* low_h, uint8_t* in_box, uint8_t* valid, int32_t* box_entry, crd_stream_t stream);
/* cal_depthMap_flow (:281-323), filter_occlusion_by_bbox (:634-676), filter_occlusion (:554-568) and lidarFlow2uv (:571-598), in the
 * order scripts/cal_gt.py:125-132 applies them.  h_new = im_h / s, w_new = im_w / s, h = h_new - y_cutoff, w = w_new.
 * Rasterise: crd_radar_rasterize's rule.  Per point with valid != 0 (valid NULL: every point): xa = clip((x1 + 0.5) / s - 0.5, 0,
 * w_new - 1), ya, xb, yb alike; its pixel is (rint(ya) - y_cutoff, rint(xa)), half to even, rows above the cutoff dropped.  A pixel
 * goes to its point of smallest depth1 (fp64), the lowest index among equal depths.  A point with a non-finite x1, y1, depth1, x2 or y2,
 * or depth1 <= 0, is skipped.
 * Box filter, on when seg != NULL (seg: uint8 [B][h][w], non-zero = vehicle; corners: fp64 [n_boxes][8][4] = x, y, depth, in_view
 * (non-zero) of the eight projected corners of a box; corner_offsets: int32 [B + 1], frame b owns the boxes corner_offsets[b] ..
 * corner_offsets[b + 1] - 1).  Per box: xs = clip((x + 0.5) / s - 0.5, 0, w - 1) and ys = clip((y + 0.5) / s - 0.5 - y_cutoff, 0,
 * h - 1) over its IN-VIEW corners give the rectangle rint(min xs) .. rint(max xs), rint(min ys) .. rint(max ys); d_max is the largest
 * depth of ALL eight.  The winner i of pixel (r, c) is dropped when seg[b][r][c] != 0, in_box[i] == 0 and some box of frame b has
 * (r, c) in its rectangle and depth1[i] > d_max.  A box with no corner in view (or a non-finite in-view coordinate) does nothing.
 * Flow filter, on when flow_im != NULL (fp32 [B][h][w][2]): at a pixel that is left, e = (xb - xa, yb - ya) - flow_im[b][r][c]
 * in fp64; the pixel is dropped when sqrt(ex * ex + ey * ey) > thres (thres_f64_bits: a double as its bit pattern).
 * At a pixel that is left:  gt[b][r][c] = (depth1[i], u, v) with u, v as crd_radar_rasterize's; depth[b][r][c] = depth1[i];
 * msk_lh[b][r][c] = low_h[i].  Every other pixel is 0 in all three.  gt: fp32 [B][h][w][3], depth: fp32 [B][h][w], msk_lh: uint8
 * [B][h][w], all written in full.  workspace, with n_pix = B * h * w: n_pix winners (uint32); from the next multiple of 16 bytes n_pix
 * depth keys (uint64); from the next multiple of 16 bytes, with seg only, 32 bytes per box; so workspace_bytes >=
 * ((((4 * n_pix + 15) & ~15) + 8 * n_pix + 15) & ~15) + (seg ? 32 * n_boxes : 0).  workspace, gt and depth are 16-byte aligned, msk_lh
 * 4-byte aligned.  Launches: clear, [boxes], min depth, min index, resolve. */
int crd_lidar_ground_truth(const double* x1, const double* y1, const double* depth1, const double* x2, const double* y2,
                           const uint8_t* low_h, const uint8_t* in_box, const uint8_t* valid, const int32_t* frame_offsets, int32_t B,
                           int32_t n_points, const double* K, int32_t k_stride, int32_t im_h, int32_t im_w, int32_t downsample_scale,
                           int32_t y_cutoff, const uint8_t* seg, const double* corners, const int32_t* corner_offsets, int32_t n_boxes,
                           const float* flow_im, uint64_t thres_f64_bits, void* workspace, int64_t workspace_bytes, float* gt,
                           float* depth, uint8_t* msk_lh, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Point-cloud back end: a depth map -> 3-D points in metres in the caller's frame ("Point-cloud back end").  The
 * inverse of the two rasterisers above and their conventions: fp64 arithmetic, fp64 quantities through device memory or as IEEE-754
 * bit patterns (uint64_t ..._f64_bits), K / k_stride, h_new = im_h / s, w_new = im_w / s, h = h_new - y_cutoff, w = w_new, no
 * allocation, no synchronisation, capturable in a graph on one stream, arguments checked before any GPU call.  The two entries add no
 * struct and change no signature: CRD_ABI_VERSION stays.
 *
 * Both read pixel (r, c) of frame b as p = (double)depth[b][r][c] (depth: fp32 [B][h][w]) and compute, every operation rounded on its
 * own (nothing is contracted into a fused multiply-add), with s = downsample_scale:
 *   1. d = max_depth * (1.0 - p)        encoding 0: normalised inverse depth, the network's output and gt_full (dataloader.py:245)
 *      d = p                            encoding 1: metres, the depth of crd_lidar_ground_truth, channel 0 of crd_radar_rasterize
 *   2. xf = (c + 0.5) * s - 0.5,  yf = (r + y_cutoff + 0.5) * s - 0.5      the full-resolution coordinate the rasterisers scale and
 *                                                                          round to this pixel: xa = (x + 0.5) / s - 0.5
 *   3. X = ((xf - cx) / fx) * d,  Y = ((yf - cy) / fy) * d,  Z = d         d is z-depth; fy for Y (the rasterisers' "fx for v" is the
 *                                                                          flow channels' alone)
 *   4. o_i = ((T[i][0] * X + T[i][1] * Y) + T[i][2] * Z) + T[i][3]         T = out_from_cam: fp64 [3][4] row-major, one for all frames
 *      (t_stride 0) or one per frame (t_stride 12), the pose chain multiplied by the caller; NULL: o = (X, Y, Z)
 *   5. each o_i is rounded to fp32 once.
 * The pixel is valid when p is finite, d > 0, min_range <= d <= max_range, for encoding 0 not (skip_empty and p == 0), for encoding 1
 * p > 0, mask == NULL or mask[b][r][c] != 0 (uint8 [B][h][w]), and labels == NULL or keep[labels[b][r][c]] != 0 (labels: uint8
 * [B][h][w]; keep: uint8 [256] on the device; labels needs keep).  p = 0 in a target map is "no ground truth" (skip_empty = 1); in a
 * prediction it is max_depth metres (skip_empty = 0).  max_depth is finite and positive, min_range and max_range are not NaN.  depth
 * is 16-byte aligned, mask and labels 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
/* The organised cloud, one launch: points fp32 [B][h][w][3] and valid uint8 [B][h][w], both written in full; an invalid pixel gets
 * (0, 0, 0) and 0.  points is 16-byte aligned, valid 4-byte aligned. */
int crd_depth_unproject(const float* depth, int32_t B, int32_t im_h, int32_t im_w, int32_t downsample_scale, int32_t y_cutoff,
                        const double* K, int32_t k_stride, const double* out_from_cam, int32_t t_stride, int32_t encoding,
                        uint64_t max_depth_f64_bits, uint64_t min_range_f64_bits, uint64_t max_range_f64_bits, int32_t skip_empty,
                        const uint8_t* mask, const uint8_t* labels, const uint8_t* keep, float* points, uint8_t* valid,
                        crd_stream_t stream);
/* The compact cloud.  The candidates are the pixels with r % stride == 0 and c % stride == 0 (stride >= 1): n_cand = ceil(h / stride) *
 * ceil(w / stride) per frame, cap = B * n_cand in all.  The valid candidates are written densely, ordered by (b, r, c) ascending:
 *   xyz            fp32 [cap][3]
 *   rgb            uint8 [cap][3] or NULL, gathered from image (uint8 [B][h][w][3], the layout of crd_assemble_input; rgb needs image)
 *   label          uint8 [cap] or NULL, the point's labels value (label needs labels)
 *   pixel          int32 [cap] or NULL, r * w + c
 *   frame_offsets  int32 [B + 1], WRITTEN here: frame b owns the rows frame_offsets[b] .. frame_offsets[b + 1] - 1, frame_offsets[B] is
 *                  the number of points -- the layout crd_radar_project and crd_lidar_project take.
 * Rows from frame_offsets[B] on are left untouched.  The order is a function of the inputs alone and the same bits every run: no atomic
 * and no workgroup waiting on another.  Three launches: the valid candidates of every tile of CRD_CLOUD_TILE consecutive candidates
 * of one frame (wave ballots), the exclusive prefix sums of the tile counts and frame_offsets (one workgroup), the scatter (the rank
 * inside a tile from the ballots).  workspace: one int32 per tile, 4-byte aligned:
 *   workspace_bytes >= 4 * B * ceil(n_cand / CRD_CLOUD_TILE). */
#define CRD_CLOUD_TILE 1024
int crd_point_cloud(const float* depth, int32_t B, int32_t im_h, int32_t im_w, int32_t downsample_scale, int32_t y_cutoff,
                    const double* K, int32_t k_stride, const double* out_from_cam, int32_t t_stride, int32_t encoding,
                    uint64_t max_depth_f64_bits, uint64_t min_range_f64_bits, uint64_t max_range_f64_bits, int32_t skip_empty,
                    const uint8_t* mask, const uint8_t* labels, const uint8_t* keep, int32_t stride, const uint8_t* image,
                    void* workspace, int64_t workspace_bytes, float* xyz, uint8_t* rgb, uint8_t* label, int32_t* pixel,
                    int32_t* frame_offsets, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Bird's-eye-view back end: a point cloud -> per-cell grids in the caller's frame ("Bird's-eye-view back end").  The
 * step after the point cloud, with its conventions: fp64 arithmetic, fp64 quantities through device memory or as IEEE-754 bit patterns
 * (uint64_t ..._f64_bits), no allocation, no synchronisation, capturable in a graph on one stream, arguments checked before any GPU
 * call.  The entry adds no struct and changes no signature: CRD_ABI_VERSION stays.  tests/bev_ref.py restates the arithmetic in NumPy;
 * the kernels agree with it bit for bit.
 *
 * Rows.  xyz: fp32 [n_rows][3].  valid: uint8 [n_rows] or NULL (every row).  label: uint8 [n_rows] or NULL.  The frame of row p:
 *   frame_offsets != NULL (int32 [B + 1] on the device, non-decreasing, read by the kernels; rows_per_frame must be 0): the b with
 *     frame_offsets[b] <= p < frame_offsets[b + 1]; an empty frame repeats a value; a row outside every frame is ignored.  This is
 *     crd_point_cloud's xyz with the frame_offsets it wrote.
 *   frame_offsets == NULL (rows_per_frame > 0): b = p / rows_per_frame; rows with b >= B are ignored.  This is crd_depth_unproject's
 *     points with its valid and rows_per_frame = h * w.
 * grid_from_points: fp64 [3][4] row-major, one for all frames (t_stride 0) or one per frame (t_stride 12), or NULL: the identity.
 *
 * Row p of frame b, every operation rounded on its own (nothing is contracted into a fused multiply-add), (x, y, z) its three floats
 * converted to fp64:
 *   1. the row is skipped when valid != NULL and valid[p] == 0, or when it has no frame
 *   2. X = T[0][0] * x + T[0][1] * y + T[0][2] * z + T[0][3], summed left to right; Y from row 1, Z from row 2;  NULL: (X, Y, Z) = (x, y, z)
 *   3. skipped unless X, Y and Z are finite
 *   4. Z = Z + 0.0                                  -0.0 becomes +0.0
 *   5. skipped unless z_lo <= Z <= z_hi             +-inf bounds are allowed
 *   6. qx = floor((X - x_min) / cell),  qy = floor((Y - y_min) / cell)
 *   7. skipped unless 0 <= qx < nx and 0 <= qy < ny, compared as doubles: a point on a lower cell edge belongs to that cell, a point at
 *      x_min + nx * cell is outside
 *   8. its cell is [b][flip_x ? nx - 1 - qx : qx][flip_y ? ny - 1 - qy : qy]
 * Outputs, each [B][nx][ny] and written in full; count and z_max are required, the others may be NULL:
 *   count      int32   the rows of the cell                                                       empty cell: 0
 *   z_max      fp32    the largest Z of the cell, rounded to fp32 once                            empty cell: the bit pattern 0x7fc00000
 *   z_min      fp32    the smallest Z, rounded to fp32 once                                       empty cell: 0x7fc00000
 *   top_index  int32   the row with the largest Z; among rows of equal fp64 Z the lowest index    empty cell: -1
 *   top_label  uint8   label[top_index] (needs label)                                             empty cell: 255
 *   occupancy  uint8   count >= min_points (min_points >= 1)                                      empty cell: 0
 * 0x7fc00000 is a NaN: crd_viz_draw paints it in bad_rgb.
 *
 * The same bits every run: only integer minimum, maximum and add, whose results do not depend on the order of arrival.  The key of a
 * height is its bit pattern with the sign bit flipped (Z >= 0) or with all bits flipped (Z < 0), which orders as the heights do.
 * Launches on `stream`, no workgroup waiting on another: (0) clear the workspace and count; (1) per row an unsigned 64-bit atomic
 * maximum and minimum of the key and an atomic add to count, the key atomics skipped where a plain read already settles them --
 * neighbouring rows of one wave that share a cell are folded first and issue one set of atomics, which changes no result; (2) per
 * row whose key is its cell's maximum an atomic minimum of the row index (only with top_index or top_label); (3) per cell the outputs.
 * With n_rows == 0 launches (1) and (2) are left out and every cell is empty.
 * workspace, 16-byte aligned, with n_cells = B * nx * ny: n_cells maximum keys (uint64); from the next multiple of 16 bytes n_cells
 * minimum keys (uint64); from the next multiple of 16 bytes n_cells winners (uint32):
 *   workspace_bytes >= 2 * ((8 * n_cells + 15) & ~15) + ((4 * n_cells + 15) & ~15).
 * CRD_E_INVALID, nothing launched: NULL workspace, count or z_max, NULL xyz with n_rows > 0; xyz, frame_offsets or a 4-byte output not
 * 4-byte aligned, grid_from_points not 8-byte, the workspace not 16-byte aligned; B <= 0; n_rows < 0; nx or ny outside 1 .. 65535;
 * B * nx * ny >= 2^31; cell not finite and positive; x_min or y_min not finite; a NaN z bound or z_lo > z_hi; t_stride not 0 or 12;
 * both or neither of frame_offsets and rows_per_frame; top_label without label; min_points < 1; a workspace too small.
 * ------------------------------------------------------------------------------------------- */
int crd_bev_grid(const float* xyz, const uint8_t* valid, const uint8_t* label, const int32_t* frame_offsets, int32_t rows_per_frame,
                 int32_t B, int32_t n_rows, const double* grid_from_points, int32_t t_stride, uint64_t x_min_f64_bits,
                 uint64_t y_min_f64_bits, uint64_t cell_f64_bits, int32_t nx, int32_t ny, uint64_t z_lo_f64_bits, uint64_t z_hi_f64_bits,
                 int32_t min_points, int32_t flip_x, int32_t flip_y, void* workspace, int64_t workspace_bytes, int32_t* count, float* z_max,
                 float* z_min, int32_t* top_index, uint8_t* top_label, uint8_t* occupancy, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Occupancy map: point clouds -> free / occupied / unknown per cell, fused over frames in a world-aligned rolling window
 * ("Occupancy map").  The step after the bird's-eye-view grid, with its conventions: fp64 arithmetic, fp64 quantities
 * through device memory or as IEEE-754 bit patterns, no allocation, no synchronisation, capturable in a graph on one stream, arguments
 * checked before any GPU call.  The entry adds no struct and changes no signature: CRD_ABI_VERSION stays.  Only IEEE add, multiply,
 * divide, floor and compare are used, every operation rounded on its own; tests/occupancy_ref.py restates them in NumPy and the
 * kernels agree with it bit for bit.
 *
 * The map.  M maps of nx x ny cells of `cell` metres, axes those of the map frame (a fixed world or odometry frame).  World cell
 * (wx, wy) covers wx * cell <= X < (wx + 1) * cell and wy * cell <= Y < (wy + 1) * cell; it lives in slot [m][wx mod nx][wy mod ny]
 * (the mathematical modulo, 0 .. nx - 1 for negative wx as well) of `map`, int16 [M][nx][ny]: a torus.  The window of map m covers the
 * world cells ox <= wx < ox + nx, oy <= wy < oy + ny with (ox, oy) = cur_origin[m]; prev_origin[m] is the window of the update before.
 * The window moves by whole cells; nothing is resampled or copied.  State of the caller, on the device, read and written by the kernels:
 * map; prev_origin and cur_origin, int64 [M][2]; initialised, int32 [M] (0: the map holds nothing yet, whatever its memory holds --
 * filling it with 0 resets the map); status, int32 [M], bits that are only ever set (1: an update of the map was skipped, 2: a frame
 * that feeds it had a sensor position that is not finite).
 *
 * Rows: xyz, valid, frame_offsets, rows_per_frame, B, n_rows exactly as for crd_bev_grid.  map_from_points: fp64 [3][4] row-major, one
 * for all frames (t_stride 0) or one per frame (t_stride 12), or NULL: the identity.  sensor, centre: fp64 [3], one for all frames
 * (stride 0) or one per frame (stride 3), IN THE POINTS' FRAME; sensor NULL: the origin; centre NULL: the sensor.  M == B: frame b
 * feeds map b; M == 1: every frame feeds map 0 (the cameras of one rig) and its centre is frame 0's.
 * With T the frame's matrix, "T . (x, y, z)" is X = T[0][0] * x + T[0][1] * y + T[0][2] * z + T[0][3] summed left to right, Y from
 * row 1, Z from row 2; T NULL: (x, y, z) itself.  S_b = T_b . sensor_b;  C_m = T_b . centre_b with b = m (M == B) or 0 (M == 1).
 *
 * The bin of a direction (dx, dy), not both zero, with q_bins = n_bins / 4 (four faces of a square, q_bins bins along each):
 *   |dx| >= |dy|:  face = 0 if dx > 0 else 2,  s = dy / |dx|;      otherwise:  face = 1 if dy > 0 else 3,  s = dx / |dy|
 *   q = min(floor(((s + 1.0) * 0.5) * q_bins), q_bins - 1);   k = face * q_bins + q
 *
 * Launch 1, prepare.  hit_min[b][k] = the bits of +inf and seen_max[b][k] = 0 for every frame and bin; hits[m][i][j] = 0 for every
 * window cell; S_b for every frame (status bit 2 of its map when a component is not finite); per map: fx = floor(Cx / cell),
 * fy = floor(Cy / cell); the update of the map is SKIPPED when Cx, Cy or Cz is not finite or |fx| or |fy| >= 2^31 - 65536: status bit
 * 1, the origins stay; otherwise prev_origin = cur_origin, then cur_origin = (fx - nx / 2, fy - ny / 2) with the integer quotient.
 * Launch 2, points (left out with n_rows == 0).  Row p of frame b, (x, y, z) its floats converted to fp64, m its map:
 *   1. skipped when valid != NULL and valid[p] == 0, or when it has no frame
 *   2. (X, Y, Z) = T_b . (x, y, z); skipped unless X, Y, Z and the three components of S_b are finite
 *   3. dx = X - Sx, dy = Y - Sy, r2 = dx * dx + dy * dy; skipped when r2 == 0 or r2 > max_range * max_range; k = the bin of (dx, dy)
 *   4. seen, if z_floor <= Z <= z_hi:  seen_max[b][k] = max(seen_max[b][k], bits(r2))     as unsigned 64-bit integers
 *   5. hit, if z_lo <= Z <= z_hi:      hit_min[b][k] = min(hit_min[b][k], bits(r2)), and with wx = floor(X / cell), wy = floor(Y / cell),
 *      if ox <= wx < ox + nx and oy <= wy < oy + ny, compared as doubles, (ox, oy) = cur_origin[m]:  hits[m][wx - ox][wy - oy] += 1
 * Launch 3, cells.  Window cell (m, i, j) is world cell (wx, wy) = (ox + i, oy + j) in slot (wx mod nx, wy mod ny);
 *   old = the slot's value if initialised[m] was nonzero before the call and the world cell lies in the prev_origin window, else 0
 *   evidence = 2 if hits[m][i][j] >= min_points;  otherwise 1 if for ANY frame b that feeds the map, with cx = (wx + 0.5) * cell,
 *     cy = (wy + 0.5) * cell (wx, wy converted to fp64), dx = cx - Sx, dy = cy - Sy, r2c = dx * dx + dy * dy and k the bin of (dx, dy):
 *       r2c > 0  and  r2c < hit_min[b][k]  and  r2c <= seen_max[b][k]           (the keys read back as doubles; a frame whose S_b is
 *     not finite fails the first); otherwise 0.  The centre is nearer than the first obstacle on its bearing and no farther than
 *     something seen there.  (seen_max <= max_range * max_range, so the kernel may test r2c against that before it takes the bin.)
 *   new = min(max(old + (l_occ, -l_free, 0 for evidence 2, 1, 0), -l_max), l_max)    in integers
 *   the slot = new (each slot belongs to exactly one window cell); initialised[m] = 1
 *   a skipped map: evidence = 0 and new = old at the window it had, with old = the slot's value if initialised[m] was nonzero, else
 *   0; neither the slot nor initialised[m] is written.
 * Outputs in WINDOW order, [M][nx][ny], written in full: log_odds int16 = new; state uint8 = 2 if new >= occupied_at, 1 if
 * new <= -free_at, else 0; evidence uint8; value fp32 = (float)new (may be NULL); origin int64 [M][2] = cur_origin after launch 1.
 *
 * The same bits every run: only integer minimum, maximum, add and or, whose results do not depend on the order of arrival
 * (non-negative doubles order as their bit patterns).  No workgroup waits for another.  A key atomic is skipped where a plain read
 * already settles it; rows of neighbouring lanes of a wave that share a bin, or hit the same cell, are folded first and issue one set
 * of atomics, which changes no result.
 * workspace, 16-byte aligned, each part from the next multiple of 16 bytes: hit_min uint64 [B][n_bins]; seen_max uint64 [B][n_bins];
 * S fp64 [B][3]; hits int32 [M][nx][ny]; the maps' flags of this call int32 [M]:
 *   workspace_bytes >= 2 * ((8 * B * n_bins + 15) & ~15) + ((24 * B + 15) & ~15) + ((4 * M * nx * ny + 15) & ~15) + ((4 * M + 15) & ~15).
 * CRD_E_INVALID, nothing launched: NULL workspace, map, prev_origin, cur_origin, initialised, status, log_odds, state, evidence or
 * origin, NULL xyz with n_rows > 0; xyz, frame_offsets, initialised, status or value not 4-byte aligned, map or log_odds not 2-byte,
 * map_from_points, sensor, centre or an origin not 8-byte, the workspace not 16-byte aligned; B <= 0; n_rows < 0; M neither B nor 1;
 * nx or ny outside 1 .. 65535; M * nx * ny >= 2^31; n_bins not a multiple of 4 in 4 .. 65536; cell not finite and positive;
 * max_range not positive or its square not finite; a NaN z bound or not z_floor <= z_lo <= z_hi; t_stride not 0 or 12; sensor_stride
 * or centre_stride not 0 or 3; both or neither of frame_offsets and rows_per_frame; min_points < 1; not 1 <= l_occ, l_free <= l_max
 * <= 32767; occupied_at or free_at outside 1 .. l_max; a workspace too small.
 * ------------------------------------------------------------------------------------------- */
int crd_occupancy_update(const float* xyz, const uint8_t* valid, const int32_t* frame_offsets, int32_t rows_per_frame, int32_t B,
                         int32_t n_rows, const double* map_from_points, int32_t t_stride, const double* sensor, int32_t sensor_stride,
                         const double* centre, int32_t centre_stride, int32_t M, int32_t nx, int32_t ny, uint64_t cell_f64_bits,
                         int32_t n_bins, uint64_t max_range_f64_bits, uint64_t z_floor_f64_bits, uint64_t z_lo_f64_bits,
                         uint64_t z_hi_f64_bits, int32_t min_points, int32_t l_occ, int32_t l_free, int32_t l_max, int32_t occupied_at,
                         int32_t free_at, int16_t* map, int64_t* prev_origin, int64_t* cur_origin, int32_t* initialised, int32_t* status,
                         void* workspace, int64_t workspace_bytes, int16_t* log_odds, uint8_t* state, uint8_t* evidence, float* value,
                         int64_t* origin, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Terrain map: point clouds -> a ground height per cell, fused over frames in the occupancy map's rolling window, and per cell the
 * step, the slope and a traversability state from LOCAL height differences ("Terrain map").  A stage beside the
 * occupancy map, with its conventions: fp64 quantities through device memory or as IEEE-754 bit patterns, no allocation, no
 * synchronisation, capturable in a graph on one stream, arguments checked before any GPU call.  The entry adds no struct and changes
 * no signature: CRD_ABI_VERSION stays.  The rows use IEEE fp64 add, multiply, divide, floor and compare, every operation rounded on its
 * own and every comparison made on the double; everything behind them is integer arithmetic, with floor division (Python's //).
 * tests/terrain_ref.py restates the entry in NumPy and the kernels agree with it bit for bit; csrc/terrain_cell.h holds the per-cell
 * rule for the kernels and for a host test.
 *
 * The map.  M maps of nx x ny cells of `cell` metres: the window, the torus, prev_origin, cur_origin, initialised and status are
 * crd_occupancy_update's, word for word, so the same centre and pose give the same origin.  Heights are integers of z_quantum metres
 * ("quanta").  State of the caller, on the device, per slot [m][wx mod nx][wy mod ny]: map_ground int32, the fused ground height;
 * map_top int32, the fused highest point under the headroom; map_weight int16, the number of fused observations, 0: never seen.  A
 * slot of weight 0 holds ground = top = 0.
 * Numbers the caller makes and passes as integers: head_q = min(floor(headroom / z_quantum), 2^30); step_max_q =
 * min(max(floor(step_max / z_quantum), 1), 2^30); slope2_max = min(max(floor((2 * cell * slope_max / z_quantum)^2), 1), 2^62), with
 * slope_max rise over run (a gradient is taken over two cells).  Heights stay below 2^24 quanta in size (z_min, z_max below), so a
 * step is below 2^25, slope2 below 2^53, and every product here fits int64; the bounds 2^30 and 2^62 change no result.
 *
 * Rows: xyz, valid, frame_offsets, rows_per_frame, B, n_rows, map_from_points, t_stride, sensor, sensor_stride, centre, centre_stride,
 * "T . (x, y, z)", S_b and C_m exactly as for crd_occupancy_update.  M == B: frame b feeds map b; M == 1: every frame feeds map 0.
 *
 * Launch 1, prepare.  lo[m][i][j] = INT32_MAX, hi[m][i][j] = INT32_MIN, n[m][i][j] = 0 for every window cell; S_b, status bit 2, the
 * skip rule (status bit 1) and the origins as launch 1 of crd_occupancy_update.
 * Launch 2, points A (left out with n_rows == 0).  Row p of frame b, (x, y, z) its floats converted to fp64, m its map:
 *   1. skipped when valid != NULL and valid[p] == 0, or when it has no frame; (X, Y, Z) = T_b . (x, y, z); skipped unless X, Y, Z and
 *      the three components of S_b are finite
 *   2. dx = X - Sx, dy = Y - Sy, r2 = dx * dx + dy * dy; skipped when r2 > max_range * max_range (a point at the sensor stays)
 *   3. skipped when Z < z_min or Z > z_max
 *   4. q = (int)floor(Z / z_quantum)
 *   5. wx = floor(X / cell), wy = floor(Y / cell); skipped unless ox <= wx < ox + nx and oy <= wy < oy + ny, compared as doubles,
 *      (ox, oy) = cur_origin[m]; with (i, j) = (wx - ox, wy - oy):  lo[m][i][j] = min(lo[m][i][j], q),  n[m][i][j] += 1
 * Launch 3, points B (left out with n_rows == 0).  Steps 1 to 5 again for every row; where q <= lo[m][i][j] + head_q, compared in
 * 64-bit integers:  hi[m][i][j] = max(hi[m][i][j], q).  What stands higher than the headroom above the lowest point of its cell is not
 * in the vehicle's way.  The cell is OBSERVED when n[m][i][j] >= min_points; then lo <= hi.
 * Launch 4, fuse.  Window cell (m, i, j) is world cell (wx, wy) = (ox + i, oy + j) in slot (wx mod nx, wy mod ny);
 *   w = the slot's weight if initialised[m] was nonzero before the call and the world cell lies in the prev_origin window, else 0
 *   (ground, top) = the slot's if w > 0, else (0, 0)
 *   observed and w == 0:  ground = lo, top = hi
 *   observed and w > 0:   ground = (w * ground + lo) // (w + 1),  top = (w * top + hi) // (w + 1)        in int64
 *   observed:             w = min(w + 1, w_max)
 *   the slot = (ground, top, w) (each slot belongs to exactly one window cell).  top >= ground stays true.
 *   A skipped map: no slot is written.
 * Launch 5, derive, from the slots of the current window after launch 4 (a skipped map: the window it had, its slots counting as
 * weight 0 if initialised[m] was zero).  A neighbour outside the window or of weight 0 is unknown.  For a cell of weight > 0:
 *   step   = max(top - ground, max over the known ones of the 8 neighbours of |ground_nb - ground|)
 *   gx     = ground[i+1][j] - ground[i-1][j] when both are known; 2 * (ground[i+1][j] - ground) or 2 * (ground - ground[i-1][j]) when
 *            one is; else 0.  gy likewise along j.  slope2 = gx * gx + gy * gy in int64
 *   state  = 2 (occupied) when step > step_max_q or slope2 > slope2_max, else 1 (free)
 *   hazard = 254 when occupied, else max(step * 253 // step_max_q, slope2 * 253 // slope2_max)
 *   value  = (float)((double)ground * z_quantum)
 * and for a cell of weight 0: step = 0, slope2 = 0, state = 0 (unknown), hazard = 255, value = the NaN of bits 0x7fc00000.
 * initialised[m] = 1 unless the map was skipped.
 * Outputs in WINDOW order, [M][nx][ny], written in full: ground, top int32 (INT32_MIN where the weight is 0), step int32, slope2
 * int64, weight int16, state, hazard uint8, evidence uint8 (1 where the cell was observed in this call; 0 all over a skipped map),
 * value fp32; origin int64 [M][2] = cur_origin after launch 1.
 *
 * The same bits every run: only integer minimum, maximum, add and or, whose results do not depend on the order of arrival.  No
 * workgroup waits for another.  An atomic is skipped where a plain read already settles it; rows of neighbouring lanes of a wave that
 * fall into one cell are folded first and issue one set of atomics, which changes no result.
 * workspace, 16-byte aligned, each part from the next multiple of 16 bytes: lo, hi, n int32 [M][nx][ny] each; S fp64 [B][3]; the maps'
 * flags of this call int32 [M]:
 *   workspace_bytes >= 3 * ((4 * M * nx * ny + 15) & ~15) + ((24 * B + 15) & ~15) + ((4 * M + 15) & ~15).
 * CRD_E_INVALID, nothing launched: a NULL workspace, state, output or origin pointer, NULL xyz with n_rows > 0; xyz, frame_offsets,
 * initialised, status, value, map_ground, map_top, ground, top or step not 4-byte aligned, map_weight or weight not 2-byte,
 * map_from_points, sensor, centre, slope2 or an origin not 8-byte, the workspace not 16-byte aligned; B <= 0; n_rows < 0; M neither B
 * nor 1; nx or ny outside 1 .. 65535; M * nx * ny >= 2^31; cell or z_quantum not finite and positive; max_range not positive or its
 * square not finite; z_min or z_max not finite, z_min > z_max, or |z| / z_quantum >= 2^24 for either; t_stride not 0 or 12;
 * sensor_stride or centre_stride not 0 or 3; both or neither of frame_offsets and rows_per_frame; min_points < 1; w_max outside
 * 1 .. 32767; head_q outside 0 .. 2^30 (a negative headroom); step_max_q outside 1 .. 2^30; slope2_max outside 1 .. 2^62; a workspace
 * too small.
 * ------------------------------------------------------------------------------------------- */
int crd_terrain_update(const float* xyz, const uint8_t* valid, const int32_t* frame_offsets, int32_t rows_per_frame, int32_t B,
                       int32_t n_rows, const double* map_from_points, int32_t t_stride, const double* sensor, int32_t sensor_stride,
                       const double* centre, int32_t centre_stride, int32_t M, int32_t nx, int32_t ny, uint64_t cell_f64_bits,
                       uint64_t z_quantum_f64_bits, uint64_t z_min_f64_bits, uint64_t z_max_f64_bits, uint64_t max_range_f64_bits,
                       int32_t head_q, int32_t min_points, int32_t w_max, int32_t step_max_q, int64_t slope2_max, int32_t* map_ground,
                       int32_t* map_top, int16_t* map_weight, int64_t* prev_origin, int64_t* cur_origin, int32_t* initialised,
                       int32_t* status, void* workspace, int64_t workspace_bytes, int32_t* ground, int32_t* top, int32_t* step,
                       int64_t* slope2, int16_t* weight, uint8_t* state, uint8_t* hazard, uint8_t* evidence, float* value, int64_t* origin,
                       crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Distance field: a state map -> per cell the squared distance to the nearest source cell, that cell, the clearance in metres and
 * an inflated costmap; and a check of candidate trajectories against the costmap ("Distance field").  The step after
 * the occupancy map, with its conventions: no allocation, no synchronisation, capturable in a graph on one stream, arguments checked
 * before any GPU call, fp64 scalars as IEEE-754 bit patterns.  The two entries add no struct and change no signature:
 * CRD_ABI_VERSION stays.  The field is integer arithmetic and two table look-ups, the path check adds fp64 divide, floor and compare;
 * tests/field_ref.py restates both in NumPy and the kernels agree with it bit for bit.
 *
 * crd_distance_field, two launches.  state: uint8 [M][nx][ny] in WINDOW order (crd_occupancy_update's `state`, or any uint8 map).
 * Cell (m, i, j) is a SOURCE when state < 8 and bit `state` of `sources` is set.  R = max_cells, FAR = R * R + 1.  clear_table fp32
 * [R * R + 2] and cost_table uint8 [R * R + 2] on the device, indexed by a squared distance 0 .. FAR.  Distances do not wrap: the window
 * is a rectangle here, not the torus.
 * Launch 1, rows.  row_near[m][i][j] = the j' that is a source of row i with |j - j'| <= R, minimises |j - j'| and is the lower j' of two
 * equal ones; -1 without one.  row_near, int32 [M][nx][ny], is the workspace.
 * Launch 2, columns.  The candidates of cell (m, i, j) are the rows i' with 0 <= i' < nx, |i - i'| <= R and j' = row_near[m][i'][j] >= 0;
 *   t = (i - i') * (i - i') + (j - j') * (j - j')
 *   dist2     int32   the least t if it is <= R * R, else FAR
 *   nearest   int32   i' * ny + j' of the winner, the lowest i' among equal t; -1 when FAR
 *   clearance fp32    clear_table[dist2]                                                              (may be NULL)
 *   cost      uint8   cost_table[dist2], raised to unknown_cost when unknown_cost > 0, state == 0 and it is lower   (may be NULL)
 * This equals the least squared distance over ALL sources of the map's window, ties to the lowest window index i' * ny + j'.
 * The same bits every run: no atomic, no workgroup waits for another; every output is written in full.
 * workspace: 16-byte aligned, workspace_bytes >= (4 * M * nx * ny + 15) & ~15.
 * CRD_E_INVALID, nothing launched: NULL state, clear_table, cost_table, workspace, dist2 or nearest; clear_table, dist2, nearest or
 * clearance not 4-byte aligned, the workspace not 16-byte aligned; M < 1; nx or ny outside 1 .. 65535; M * nx * ny >= 2^31; max_cells
 * outside 1 .. 255; sources outside 1 .. 255; unknown_cost outside 0 .. 255; a workspace too small.
 *
 * crd_field_paths, one launch.  xy: fp64 [K][P][2], metres in the map frame.  n_poses: int32 [K], the poses of path k that count,
 * taken as min(max(n_poses[k], 0), P); NULL: all P.  path_map: int32 [K], the map of path k; NULL: map 0.  origin: int64 [M][2] on the
 * device (crd_occupancy_update's `origin`).  state, dist2, cost: the field's input and outputs, [M][nx][ny].  FAR = max_cells *
 * max_cells + 1.  Pose p < n_poses[k] of path k with map m = path_map[k], (X, Y) its two doubles, (ox, oy) = origin[m]:
 *   wx = floor(X / cell), wy = floor(Y / cell)
 *   INSIDE when 0 <= m < M, X and Y are finite, and ox <= wx < ox + nx and oy <= wy < oy + ny compared as doubles (ox, oy, ox + nx and
 *   oy + ny converted to fp64): its cell is (i, j) = (wx - ox, wy - oy), c = i * ny + j; OUTSIDE otherwise
 *   BLOCKED when inside with cost[m][i][j] >= blocked_at, or outside with outside_blocks == 1
 * Per path, [K]:  first_blocked int32 = the lowest blocked p, or -1;  max_cost uint8 = the largest cost over the inside poses, 0
 * without one;  min_dist2 int32 = the least dist2 over the inside poses, FAR without one;  n_outside int32;  n_unknown int32 = the
 * inside poses with state == 0.  pose_cell int32 [K][P] (may be NULL) = c, -1 outside, -2 for p >= n_poses[k].
 * One wave per path; integer minimum, maximum and add over its lanes, which do not depend on any order.
 * CRD_E_INVALID, nothing launched: NULL xy, origin, state, dist2, cost or a per-path output; xy or origin not 8-byte aligned, n_poses,
 * path_map, dist2, first_blocked, min_dist2, n_outside, n_unknown or pose_cell not 4-byte; K or P < 1; M < 1; nx or ny outside
 * 1 .. 65535; M * nx * ny >= 2^31; max_cells outside 1 .. 255; blocked_at outside 1 .. 255; outside_blocks neither 0 nor 1; cell not
 * finite and positive.
 * ------------------------------------------------------------------------------------------- */
int crd_distance_field(const uint8_t* state, int32_t M, int32_t nx, int32_t ny, int32_t sources, int32_t max_cells, int32_t unknown_cost,
                       const float* clear_table, const uint8_t* cost_table, void* workspace, int64_t workspace_bytes, int32_t* dist2,
                       int32_t* nearest, float* clearance, uint8_t* cost, crd_stream_t stream);
int crd_field_paths(const double* xy, const int32_t* n_poses, const int32_t* path_map, int32_t K, int32_t P, const int64_t* origin,
                    uint64_t cell_f64_bits, const uint8_t* state, const int32_t* dist2, const uint8_t* cost, int32_t M, int32_t nx,
                    int32_t ny, int32_t max_cells, int32_t blocked_at, int32_t outside_blocks, int32_t* first_blocked, uint8_t* max_cost,
                    int32_t* min_dist2, int32_t* n_outside, int32_t* n_unknown, int32_t* pose_cell, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Navigation field: a costmap and goal points -> per cell the least cost to reach a goal and the neighbour to step to, as ROS navfn /
 * global_planner give them; and the paths that follow those steps from K starts ("Navigation field").  The step after
 * the distance field, with its conventions: no allocation, no synchronisation, capturable in a graph on one stream, arguments checked
 * before any GPU call, fp64 scalars as IEEE-754 bit patterns.  The two entries add no struct and change no signature:
 * CRD_ABI_VERSION stays.  Integer arithmetic only; the fp64 divide, floor and compare that find a cell and the cell centres of a path
 * are written out below.  tests/nav_ref.py restates both entries in NumPy and the kernels agree with it bit for bit.
 *
 * Grid.  The window's rectangle [nx][ny], 8-connected; it does not wrap (as in crd_distance_field).  Neighbour code n = 0 .. 7 is
 * (di, dj) = (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0), (1,1); its weight k_n is 7 for a diagonal, 5 for an axis move
 * (chamfer 5-7).  Cell c is PASSABLE when cost[m][i][j] < blocked_at.  Standing on it costs w(c) = neutral + cost[c], neutral 1 .. 255
 * (navfn's COST_NEUTRAL is 50).  There is no corner rule: a diagonal move between two impassable cells is allowed.  With the field's
 * inscribed >= cell the inflated walls are at least two cells thick and it cannot happen.
 *
 * crd_nav_field, three launches.  cost: uint8 [M][nx][ny] (crd_distance_field's `cost`, or any uint8 map).  goals: fp64 [M][G][2],
 * metres in the map frame; n_goals: int32 [M], the goals of map m that count, taken as min(max(n_goals[m], 0), G); NULL: all G.
 * origin: int64 [M][2] on the device.  A goal's cell is found by crd_field_paths' INSIDE rule: wx = floor(X / cell), wy = floor(Y /
 * cell), inside when X and Y are finite and ox <= wx < ox + nx, oy <= wy < oy + ny compared as doubles; (i, j) = (wx - ox, wy - oy).
 * A goal that is not finite, outside the window or on an impassable cell is SKIPPED.
 *   togo  int32 [M][nx][ny]  0 on every passable goal cell; elsewhere the least, over all 8-connected paths of passable cells from the
 *                            cell to a goal cell, of the sum of k * w(a) over every cell a of the path but the goal, k the weight of the
 *                            move that leaves a: the unique fixed point of togo[a] = min_n (togo[a + n] + k_n * w(a)).  UNREACHED =
 *                            0x7fffffff on impassable cells and on cells without a path.
 *   next  uint8 [M][nx][ny]  (may be NULL)  8 on a goal cell (togo == 0), 255 where togo is UNREACHED, else the code n that minimises
 *                            togo[a + n] + k_n * w(a) over the neighbours inside the window with togo != UNREACHED, the lowest n among
 *                            equal ones.  A launch of its own over the final togo: a function of togo, cost and neutral alone.
 *   info  int32 [M][4]       {converged (0 / 1), rounds, goals_used, goals_skipped}; goals_used + goals_skipped = the goals that count
 * One step costs at most 7 * 510 = 3570 and a shortest path visits a cell once, so with nx * ny <= 2^19 per map every togo is below
 * 3570 * 2^19 < 2^31; inside a row scan a candidate reaches at most that + 5 * 510 * 65535 < 2^31.  UNREACHED + anything is never formed.
 * Order.  Launch 1 sets togo to UNREACHED.  Launch 2, one wave per map, sets the goal cells to 0 and relaxes in ROUNDS.  A ROW STEP of
 * row i from row p takes t[j] = min(togo[i][j], togo[p][j + dj] + k * w(i, j) over dj = -1, 0, 1) on the passable cells, then left to
 * right d[j] = min(t[j], d[j - 1] + 5 * w(i, j)), then right to left the same from d[j + 1], a wall or the row's end giving nothing.  A
 * round is the row steps i = 0 .. nx - 1 from p = i - 1 (row 0 from none) and then i = nx - 2 .. 0 from p = i + 1.  Rounds end after the
 * first that lowers no value (converged = 1: togo is the fixed point) or after max_rounds, 1 .. 4096 (converged = 0: every value is still
 * the cost of a real path, or UNREACHED, so >= the true one; following `next` still strictly lowers togo, by at least 5 a step, so a
 * path always ends).  rounds, 1 .. max_rounds, is informative: it belongs to this order.  The fixed point does not.
 * The same bits every run: no atomic, no workgroup waits for another; every output is written in full.  No workspace.
 * CRD_E_INVALID, nothing launched: NULL cost, goals, origin, togo or info; goals or origin not 8-byte aligned, n_goals, togo or info not
 * 4-byte; M < 1; nx or ny outside 1 .. 65535; nx * ny > 2^19; M * nx * ny >= 2^31; G < 1; neutral outside 1 .. 255; blocked_at outside
 * 1 .. 255; max_rounds outside 1 .. 4096; cell not finite and positive.
 *
 * crd_nav_paths, one launch, one lane per path: a path is a chain of dependent reads.  starts: fp64 [K][2], metres in the map frame.
 * path_map: int32 [K], the map of path k; NULL: map 0; an index outside 0 .. M-1: no start cell.  togo, next: crd_nav_field's.  P >= 1:
 * the most cells of a path.  The start cell is found by the INSIDE rule above.  From it the path steps to the neighbour next names
 * until it stands on a cell whose next is 8, which is its last, or holds P cells.
 *   cells       int32 [K][P]     i * ny + j of the cells from the start cell on, the goal cell included when reached; -1 behind the end
 *   xy          fp64 [K][P][2]   (may be NULL)  the cells' centres ((double)(ox + i) + 0.5) * cell and ((double)(oy + j) + 0.5) * cell, ox +
 *                                i an int64 sum, each operation rounded to fp64 in that order; NaN behind the end.  crd_field_paths takes it.
 *   n_cells     int32 [K]        0 with status 2 or 3
 *   start_togo  int32 [K]        togo of the start cell; UNREACHED without a start cell
 *   status      int32 [K]        0 ended on a goal; 1 cut at P; 2 start not finite, outside the window or a bad map index; 3 the start
 *                                cell is UNREACHED
 * A next that is neither 0 .. 7 nor 8 on a reached cell, or that steps out of the window -- crd_nav_field writes neither -- ends the path
 * with status 1.
 * CRD_E_INVALID, nothing launched: NULL starts, origin, togo, next, cells, n_cells, start_togo or status; starts, origin or xy not 8-byte
 * aligned, path_map, togo, cells, n_cells, start_togo or status not 4-byte; K or P < 1; K * P >= 2^30; the shapes and the cell as above.
 * ------------------------------------------------------------------------------------------- */
int crd_nav_field(const uint8_t* cost, int32_t M, int32_t nx, int32_t ny, const double* goals, const int32_t* n_goals, int32_t G,
                  const int64_t* origin, uint64_t cell_f64_bits, int32_t neutral, int32_t blocked_at, int32_t max_rounds, int32_t* togo,
                  uint8_t* next, int32_t* info, crd_stream_t stream);
int crd_nav_paths(const double* starts, const int32_t* path_map, int32_t K, int32_t P, const int64_t* origin, uint64_t cell_f64_bits,
                  const int32_t* togo, const uint8_t* next, int32_t M, int32_t nx, int32_t ny, int32_t* cells, double* xy, int32_t* n_cells,
                  int32_t* start_togo, int32_t* status, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Map objects: a state map -> the connected sets of its source cells as a label per cell and a table of objects ("Map
 * objects").  A stage beside the distance field, with the conventions of the map stages: no allocation, no synchronisation, capturable
 * in a graph on one stream, arguments checked before any GPU call, fp64 scalars as IEEE-754 bit patterns.  The entry adds no struct and
 * changes no signature: CRD_ABI_VERSION stays.  Integer arithmetic only but the centre, which is written out below.
 * tests/objects_ref.py restates the entry in NumPy and the kernels agree with it bit for bit.
 *
 * crd_map_objects, eight launches (seven with centre == NULL), whatever the map holds.  state: uint8 [M][nx][ny] in WINDOW order
 * (crd_occupancy_update's `state`, or any uint8 map).  Cell (m, i, j) is a SOURCE when state < 8 and bit `state` of `sources` is set,
 * as in crd_distance_field.  Two source cells of one map are NEIGHBOURS when they differ by 1 in i or in j and not in the other
 * (connectivity 4), or by at most 1 in both (connectivity 8: cells that touch at a corner as well).  The window is a rectangle here, not
 * the torus.  An OBJECT is a maximal set of source cells joined by chains of neighbours.  Its FIRST CELL is its lowest window index
 * i * ny + j.  The objects of a map are ordered by their first cells (scipy.ndimage.label's numbering minus one).
 * Objects of fewer than min_cells cells are SMALL.  The others are KEPT and numbered 0, 1, ... in that order; with N = max_objects, the
 * kept objects with a number >= N OVERFLOW.
 *   label    int32 [M][nx][ny]  -1 on a non-source cell, -2 on a cell of a small object, -3 on a cell of an overflowing object, else
 *                               the object's number 0 .. N-1
 *   objects  int32 [M][N][8]    row k: {first_cell, n_cells, i_min, i_max, j_min, j_max, flags, 0} of kept object k; flags bit 0 is set
 *                               when a cell of the object lies in row 0 or nx - 1 or column 0 or ny - 1; unused rows are
 *                               {-1, 0, -1, -1, -1, -1, 0, 0}
 *   sums     int64 [M][N][2]    {sum of i, sum of j} over the object's cells; unused rows 0
 *   centre   fp64 [M][N][2]     (may be NULL)  x = (((double)ox + (double)sum_i / (double)n_cells) + 0.5) * cell and y the same with oy and
 *                               sum_j, (ox, oy) = origin[m], each operation rounded to fp64 in that order: the mean of crd_nav_paths' cell
 *                               centres, which crd_field_paths and crd_nav_field's goals take as they are.  NaN (0x7ff8000000000000) in
 *                               unused rows.  The centre of a concave object may lie off it.
 *   info     int32 [M][4]       {n_objects = the rows in use, min(kept, N); n_overflow = the kept objects without a row; n_small; guard}
 * origin: int64 [M][2] on the device (crd_occupancy_update's `origin`), read there, for the centre only.
 * Every output is a function of the partition into objects alone.  Integer atomics (min, max, or, add) write the table and the
 * counts, so no order changes a bit: the same bits every run.  No float atomic; no workgroup waits for another.
 * Order.  Launch 1 labels tiles of 16 rows x 64 columns in LDS.  Launch 2 joins the tiles along their borders by a union-find on the
 * parent table, which is `label`: the larger root is always hung under the smaller, so parent[c] <= c at all times and a root is a
 * first cell; every access is an agent-scope atomic and nothing is concluded before launch 3.  Launches 3 to 7 find every cell's root,
 * count the cells per root, number the kept roots by a count scan in index order, write label and fill the table.  Every device loop
 * is capped: a find makes at most nx * ny steps and a union at most nx * ny retries.  A loop that reaches its cap leaves and sets guard
 * to 1: guard is 0 in every correct run, and with 1 the map's outputs are not to be trusted.
 * workspace: 16-byte aligned, workspace_bytes >= (8 * M * nx * ny + 15) & ~15 (a root and a count per cell).
 * CRD_E_INVALID, nothing launched: NULL state, origin, workspace, label, objects, sums or info; label, objects or info not 4-byte
 * aligned, sums, centre or origin not 8-byte, the workspace not 16-byte; M < 1; nx or ny outside 1 .. 65535; M * nx * ny >= 2^31;
 * sources outside 1 .. 255; connectivity neither 4 nor 8; min_cells < 1; max_objects outside 1 .. 65535; a workspace too small; cell
 * not finite and positive.
 * ------------------------------------------------------------------------------------------- */
int crd_map_objects(const uint8_t* state, int32_t M, int32_t nx, int32_t ny, int32_t sources, int32_t connectivity, int32_t min_cells,
                    int32_t max_objects, const int64_t* origin, uint64_t cell_f64_bits, void* workspace, int64_t workspace_bytes,
                    int32_t* label, int32_t* objects, int64_t* sums, double* centre, int32_t* info, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Object tracks: the object table of a frame and the tracks kept over the frames -> every row's track, with an id that stays
 * ("Object tracks").  The stage behind crd_map_objects, with the conventions of the map stages: no allocation, no
 * synchronisation, capturable in a graph on one stream, arguments checked before any GPU call, fp64 scalars as IEEE-754 bit
 * patterns.  The entry adds no struct and changes no signature: CRD_ABI_VERSION stays.  tests/tracks_ref.py restates the entry in
 * NumPy and the kernel agrees with it bit for bit.
 *
 * crd_track_objects, one launch.  objects int32 [M][N][8], centre fp64 [M][N][2], objects_info int32 [M][4]: crd_map_objects' outputs
 * (N = its max_objects, here 1 .. 1024).  origin int64 [M][2] on the device, (ox, oy) = origin[m].  The STATE, T slots per map, is
 * read and written in place:
 *   ids      int64 [M][T]     the track's id, -1 in a free slot
 *   tracks   int32 [M][T][8]  {status (0 FREE, 1 TENTATIVE, 2 CONFIRMED), age, hits, misses, object, n_cells, flags, 0}
 *   pos      fp64 [M][T][2]   metres in the map frame, as centre;  vel fp64 [M][T][2]  metres per call
 *   box      int64 [M][T][4]  WORLD cells {ox + i_min, ox + i_max, oy + j_min, oy + j_max} of the row last matched
 *   next_id  int64 [M]        the id of the map's next birth
 * A FREE slot holds ids -1, tracks {0, 0, 0, 0, -1, 0, 0, 0}, pos and vel NaN (0x7ff8000000000000), box 0; a slot is LIVE when its
 * status is not 0.  Per map, in this order, every fp64 operation rounded to fp64 in the order written (no fused multiply-add):
 *   1 predict     every live slot t: pred = pos + vel, per component
 *   2 candidates  the rows k < n = min(max(objects_info[m][0], 0), N) whose centre z has two finite components.  For a live slot t and
 *                 a candidate row k: dx = z.x - pred.x, dy = z.y - pred.y, d2 = (dx * dx) + (dy * dy); (t, k) is a PAIR when
 *                 d2 <= gate * gate (the product rounded once; a NaN compares false)
 *   3 associate   the greedy assignment over the pairs in ascending order of the triple (d2, t, k): a pair is TAKEN when neither its
 *                 slot nor its row is taken yet.  Run as ROUNDS: every untaken candidate row picks its least (d2, t) over the untaken
 *                 live slots it pairs with, every untaken live slot its least (d2, k) over the untaken rows; a row and a slot that
 *                 picked each other are taken; the rounds end after the first that takes nothing.  The least pair left is always
 *                 mutual, and nothing before a mutual pair in the order shares its slot or row, so this IS the sorted greedy
 *                 assignment.  Every round but the last takes a pair, so there are at most min(N, T) + 1, which is the cap of the
 *                 loop; leaving by the cap sets guard to 1: guard is 0 in every correct run.  rounds, 1 .. min(N, T) + 1, counts the
 *                 last round too; it is the longest chain of displaced picks plus one and belongs to this order, the pairs do not.
 *   4 matched     a live slot taken by row k: r = z - pred, pos = pred + alpha * r, vel = vel + beta * r (per component); hits + 1,
 *                 misses = 0, age + 1 (hits, misses and age stop at 2^31 - 1); object = k; n_cells and flags are the row's; box from
 *                 the row and the origin (64-bit sums); status = CONFIRMED once hits >= confirm_hits
 *   5 unmatched   a live slot not taken: pos = pred, vel stays, misses + 1, age + 1, object = -1, n_cells, flags and box stay; with
 *                 misses > max_misses the slot is freed (n_missed_out)
 *   6 left        a slot still live whose pos is not INSIDE the window by crd_field_paths' rule (wx = floor(X / cell), wy = floor(Y /
 *                 cell), X and Y finite, ox <= wx < ox + nx and oy <= wy < oy + ny compared as doubles) is freed (n_left): the map
 *                 has forgotten that ground.  The row that had taken it keeps no track and is not born either.
 *   7 births      the candidate rows not taken, in row order, take the free slots, in slot order, those freed by 5 and 6 included,
 *                 rank to rank (a count scan, no ticket).  Rank r is born with ids = next_id + r, pos = z, vel = +0, hits = 1,
 *                 misses = 0, age = 1, object = k, n_cells, flags and box from the row, status TENTATIVE, or CONFIRMED when
 *                 confirm_hits == 1.  Rows beyond the free slots stay without a track (n_overflow).  next_id += the births.
 * Per call:
 *   track_of  int32 [M][N]  the slot that holds row k's track after the call (matched and still live, or born), else -1
 *   id_of     int64 [M][N]  that slot's id, else -1
 *   info      int32 [M][8]  {n_live (at the end), n_matched (the pairs taken), n_born, n_missed_out, n_left, n_overflow, rounds, guard}
 * So n_live = the n_live before + n_born - n_missed_out - n_left, tracks[..][object] and track_of are inverse to each other on the
 * live slots with object >= 0, and an id is never used twice.  Merges and splits are not modelled: when two objects grow into one, one
 * track goes on with the joint object and the other coasts and drops.
 * One workgroup per map, one thread per slot and per row, the predictions, the centres, the taken marks and the picks in LDS.  No
 * atomic, no workgroup waits for another, every output written in full: the same bits every run.
 * CRD_E_INVALID, nothing launched: NULL objects, centre, objects_info, origin, ids, tracks, pos, vel, box, next_id, track_of, id_of or
 * info; objects, objects_info, tracks, track_of or info not 4-byte aligned, centre, origin, ids, pos, vel, box, next_id or id_of not
 * 8-byte; M < 1; N or T outside 1 .. 1024; nx or ny outside 1 .. 65535; cell not finite and positive; gate not finite and positive or
 * with an infinite square; alpha outside (0, 1]; beta outside [0, 2]; confirm_hits < 1; max_misses < 0.
 * ------------------------------------------------------------------------------------------- */
int crd_track_objects(const int32_t* objects, const double* centre, const int32_t* objects_info, const int64_t* origin, int32_t M, int32_t N,
                      int32_t T, int32_t nx, int32_t ny, uint64_t cell_f64_bits, uint64_t gate_f64_bits, uint64_t alpha_f64_bits,
                      uint64_t beta_f64_bits, int32_t confirm_hits, int32_t max_misses, int64_t* ids, int32_t* tracks, double* pos, double* vel,
                      int64_t* box, int64_t* next_id, int32_t* track_of, int64_t* id_of, int32_t* info, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scan matcher: a cloud, its prior pose and the occupancy map as it stands -> the pose corrected by the best of a window of turns and
 * whole-cell shifts ("Scan matching"; correlative scan matching, Olson, ICRA 2009).  The stage in front of
 * crd_occupancy_update, with the conventions of the map stages: no allocation, no synchronisation, capturable in a graph on one
 * stream, arguments checked before any GPU call, fp64 scalars as IEEE-754 bit patterns.  The entry adds no struct and changes no
 * signature: CRD_ABI_VERSION stays.  The device only adds, multiplies, divides, floors and compares, every operation rounded on its own;
 * tests/match_ref.py restates the entry in NumPy and the kernels agree with it bit for bit.  The map is READ ONLY here.
 *
 * Rows: xyz, valid, frame_offsets, rows_per_frame, B, n_rows exactly as for crd_bev_grid.  map_from_points (the prior pose, T_b),
 * t_stride, sensor, sensor_stride, M, nx, ny, cell, max_range, z_lo, z_hi, min_points: as for crd_occupancy_update, the numbers those of
 * the map.  map int16 [M][nx][ny] (the torus), cur_origin int64 [M][2], initialised int32 [M]: the map's state, as the last update left
 * it.  M == B: frame b is matched against map b; M == 1: all frames against map 0, with one correction for all.
 *
 * Candidates.  t in 0 .. 2 * n_theta, dx and dy in -n_xy .. n_xy (whole cells); n_xy 0 .. 16, n_theta 0 .. 32; NT = 2 * n_theta + 1,
 * NS = 2 * n_xy + 1.  rot fp64 [NT][2] on the device: (c, s) = (cos, sin) of the turn of t, (t - n_theta) * d_theta, made on the host;
 * the row of t = n_theta is not read.
 * The candidate pose T'[b][t] turns T = T_b (NULL: the identity) about the vertical axis of the map frame through S = T_f . sensor_f,
 * f = b (M == B) or 0 (M == 1).  With (c, s) = rot[t], for k = 0, 1, 2:
 *   R'[0][k] = c * T[0][k] - s * T[1][k];   R'[1][k] = s * T[0][k] + c * T[1][k];   row 2 of T is copied
 *   t'x = (c * T[0][3] - s * T[1][3]) + (Sx - (c * Sx - s * Sy));   t'y = (s * T[0][3] + c * T[1][3]) + (Sy - (s * Sx + c * Sy))
 * and T'[b][n_theta] is T itself, copied: the zero candidate sees exactly the cells crd_occupancy_update would.
 * Scan cells.  A row is an obstacle row when it passes steps 1 to 3 of crd_occupancy_update's launch 2 and z_lo <= Z <= z_hi, all with
 * the unturned T_b and S_b.  For every t an obstacle row counts into world cell (floor(X_t / cell), floor(Y_t / cell)), (X_t, Y_t)
 * rows 0 and 1 of T'[b][t] . (x, y, z) summed left to right, when that cell lies in the window of its map grown by n_xy cells on every
 * side, ox - n_xy <= wx < ox + nx + n_xy and oy - n_xy <= wy < oy + ny + n_xy compared as doubles, (ox, oy) = cur_origin[m] (cells
 * farther out meet the map under no shift).  A cell is a SCAN CELL of (m, t) when its count reaches min_points.
 * Map value.  L(wx, wy) = map[m][wx mod nx][wy mod ny] (the mathematical modulo) when initialised[m] != 0 and ox <= wx < ox + nx and
 * oy <= wy < oy + ny; otherwise 0.
 * Score.  table[m][t][dx + n_xy][dy + n_xy] = the sum of L(wx + dx, wy + dy) over the scan cells (wx, wy) of (m, t), in 64-bit integers.
 * Pick.  The candidate with the largest score; among equals the least dx * dx + dy * dy, then the least |t - n_theta|, then the least
 * t, then dx, then dy.  A symmetric scene keeps the prior.
 * status int32 [M], this call's alone: 1 initialised[m] == 0; 2 an entry of T_b or a component of S_b of a frame that feeds the map is
 * not finite; 4 n_cells[m] < min_cells, n_cells[m] the scan cells of (m, n_theta) inside the window itself; 8 the pick's score <
 * min_score.  Each of these four KEEPS THE PRIOR.  16, only when none of them is set: the pick lies on the border of a search range
 * that is not empty (|dx| or |dy| == n_xy > 0, or |t - n_theta| == n_theta > 0); the pose is applied all the same.
 * Outputs, written in full:
 *   pose         fp64 [B][3][4]  T'[b][t*] with t'x + dx* * cell and t'y + dy* * cell (dx*, dy* converted to fp64, the product rounded,
 *                                then the sum); T_b itself, copied, when the map keeps the prior
 *   pick         int32 [M][3]    (t* - n_theta, dx*, dy*), the best candidate whether it is applied or not;  score int64 [M], its score
 *   prior_score  int64 [M]       table[m][n_theta][n_xy][n_xy];   n_cells int32 [M]
 *   scores       int64 [M][NT][NS][NS], the table; may be NULL
 * Four launches: prepare (T', S, clears), points (one thread per row, every turn, an integer atomic add per run of neighbouring lanes
 * that share a cell), scores (a workgroup per tile of 32 x 32 count cells, turn and map: the tile's scan cells compacted, the log-odds
 * under it with a halo of n_xy cells in LDS, a thread per shift, one 64-bit atomic add per shift), pick (a workgroup per map).  Integer
 * atomics only and a pick that is the least element of a total order: the same bits every run.  No workgroup waits for another.
 * workspace, 16-byte aligned, each part from the next multiple of 16 bytes: T' fp64 [B][NT][3][4]; S fp64 [B][3]; the counts int32
 * [M][NT][nx + 2 n_xy][ny + 2 n_xy]; the table int64 [M][NT][NS][NS]:
 *   workspace_bytes >= ((96 * B * NT + 15) & ~15) + ((24 * B + 15) & ~15) + ((4 * M * NT * (nx + 2 n_xy) * (ny + 2 n_xy) + 15) & ~15)
 *                      + ((8 * M * NT * NS * NS + 15) & ~15).
 * CRD_E_INVALID, nothing launched: NULL workspace, map, cur_origin, initialised, rot, pose, pick, score, prior_score, n_cells or status,
 * NULL xyz with n_rows > 0; xyz, frame_offsets, initialised, pick, n_cells or status not 4-byte aligned, map not 2-byte,
 * map_from_points, sensor, cur_origin, rot, pose, score, prior_score or scores not 8-byte, the workspace not 16-byte aligned; B outside
 * 1 .. 65535; n_rows < 0; M neither B nor 1; nx or ny outside 1 .. 65535; M * nx * ny >= 2^31; n_xy outside 0 .. 16; n_theta outside
 * 0 .. 32; 2^31 counts or more; cell not finite and positive; max_range not positive or its square not finite; a NaN z bound or not
 * z_lo <= z_hi; t_stride not 0 or 12; sensor_stride not 0 or 3; both or neither of frame_offsets and rows_per_frame; min_points < 1;
 * min_cells < 0; a workspace too small.
 * ------------------------------------------------------------------------------------------- */
int crd_match_scan(const float* xyz, const uint8_t* valid, const int32_t* frame_offsets, int32_t rows_per_frame, int32_t B, int32_t n_rows,
                   const double* map_from_points, int32_t t_stride, const double* sensor, int32_t sensor_stride, int32_t M, int32_t nx,
                   int32_t ny, uint64_t cell_f64_bits, uint64_t max_range_f64_bits, uint64_t z_lo_f64_bits, uint64_t z_hi_f64_bits,
                   int32_t min_points, const int16_t* map, const int64_t* cur_origin, const int32_t* initialised, int32_t n_xy,
                   int32_t n_theta, const double* rot, int32_t min_cells, int64_t min_score, void* workspace, int64_t workspace_bytes,
                   double* pose, int32_t* pick, int64_t* score, int64_t* prior_score, int32_t* n_cells, int32_t* status, int64_t* scores,
                   crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Local planner: the vehicle's pose, the costmap, the cost-to-go and the object tracks -> a velocity command, the best of K velocity
 * candidates rolled out over a short horizon ("Local planner"; the dynamic window approach of Fox, Burgard and Thrun,
 * 1997, as ROS base_local_planner / dwa_local_planner run it).  The stage behind the map stages, with their conventions: no
 * allocation, no synchronisation, capturable in a graph on one stream, arguments checked before any GPU call, fp64 scalars as IEEE-754
 * bit patterns.  The entry adds no struct and changes no signature: CRD_ABI_VERSION stays.  The device only adds, subtracts,
 * multiplies, divides, floors and compares, every operation rounded to fp64 on its own (no fused multiply-add); the sines and cosines
 * of the arcs are in a table made on the host.  tests/rollout_ref.py restates the entry in NumPy and the kernels agree with it bit for
 * bit.  Every input is READ ONLY.
 *
 * crd_plan_rollouts, two launches.  Candidates k = iv * n_w + iw, iv in 0 .. n_v - 1 (n_v 1 .. 64), iw in 0 .. n_w - 1 (n_w odd,
 * 1 .. 129), c = (n_w - 1) / 2, K = n_v * n_w <= 4096.  P poses per candidate, 1 .. 256.  Tables on the device, made on the host:
 *   vw   fp64 [K][2]     the candidate's velocities (v, w)
 *   arc  fp64 [K][P][2]  (x, y), the pose of candidate k at time (p + 1) * dt in the vehicle's frame (x forward, y left)
 *   tau  fp64 [P]        (p + 1) * dt in track updates
 * pose fp64 [M][3][4], T = pose[m]: the map-from-vehicle pose; rows 0 and 1 are used.  origin int64 [M][2], cost uint8 [M][nx][ny]:
 * as for crd_field_paths.  togo int32 [M][nx][ny], crd_nav_field's; may be NULL.  tracks int32 [M][T][8], pos and vel fp64 [M][T][2]:
 * crd_track_objects' state, T 1 .. 1024; tracks may be NULL with T = 0.  twist fp64 [M][2], the current (v, w); may be NULL.
 * For map m, candidate k and pose p, with (x, y) = arc[k][p], in this order:
 *   Map-frame pose.  X = T[0][0] * x + T[0][1] * y + T[0][3] and Y = T[1][0] * x + T[1][1] * y + T[1][3], summed left to right.
 *   Static test.  crd_field_paths' rule: wx = floor(X / cell), wy = floor(Y / cell); INSIDE when X and Y are finite and ox <= wx <
 *     ox + nx and oy <= wy < oy + ny compared as doubles, its cell (i, j) = (wx - ox, wy - oy); BLOCKED when inside with
 *     cost[m][i][j] >= blocked_at, or outside with outside_blocks == 1.
 *   Track test.  Slot s of map m COUNTS when tracks[m][s][0] (status) >= min_status, the two components of pos[m][s] and of
 *     vel[m][s] are finite, tracks[m][s][5] (n_cells) <= max_object_cells and vel_x * vel_x + vel_y * vel_y >= min_speed2.  For a
 *     counting slot: qx = pos_x + vel_x * tau[p], qy = pos_y + vel_y * tau[p], dx = X - qx, dy = Y - qy, d2 = dx * dx + dy * dy; the
 *     pose is HIT by s when d2 <= keep_out2 (a NaN compares false).
 * Per candidate:
 *   first_blocked  the lowest p that is blocked or hit by a counting slot, or -1
 *   first_track    the lowest slot that hits the lowest hit pose, whether or not an earlier pose is blocked, or -1
 *   max_cost, sum_cost  the largest and the sum of cost over the inside poses; 0 without one
 *   end_togo       togo[m][cell of pose P - 1]; UNREACHED = 0x7fffffff when that pose is outside or togo is NULL
 *   ADMISSIBLE     twist is NULL, or |vw[k][0] - twist[m][0]| <= a_v_dt and |vw[k][1] - twist[m][1]| <= a_w_dt (a NaN compares false)
 *   CLEAR_STATIC   no pose is blocked;  CLEAR  first_blocked == -1
 *   VALID          admissible, clear, and not (togo given, w_togo > 0 and end_togo == UNREACHED)
 *   score  int64   w_togo * end_togo (left out when togo is NULL) + w_max_cost * max_cost + w_sum_cost * sum_cost
 *                  + w_slow * (n_v - 1 - iv) + w_turn * |iw - c|; each weight 0 .. 32767
 * Pick, per map: the valid candidate of least score; among equals the least |iw - c|, then the larger iv, then the least k.
 * status: 1 NOT_FINITE, one of the 12 entries of pose[m] or, with a twist, of the 2 of twist[m] is not finite; 2 NO_CANDIDATE, no
 * candidate is valid.  A candidate is picked when status is 0.
 * Outputs, written in full:
 *   best     int32 [M]     the picked k, or -1;   score int64 [M]  its score, or 0
 *   command  fp64 [M][2]   vw[best] copied, or (+0.0, +0.0): the vehicle stops
 *   info     int32 [M][8]  {n_admissible, n_clear_static, n_clear, n_valid, status, 0, 0, 0}, each count over all K candidates
 *   scores int64, first_blocked, first_track, max_cost, end_togo int32, each [M][K]: the per-candidate values; all five or all NULL
 *   xy       fp64 [M][K][P][2]  (X, Y) of every pose; may be NULL.  crd_field_paths takes a map's [K][P][2] as it is.
 * Launch 1, rollouts: one wave per (candidate, map), four to a workgroup, the lanes over the poses; the workgroup first compacts the
 * counting slots of its map into LDS by ballot, in slot order, and every lane walks that list; integer minimum, maximum and add over
 * the wave; one record per candidate into the workspace.  Launch 2, pick: one workgroup per map.  No global atomic and a pick that is
 * the least element of a total order: the same bits every run.  No workgroup waits for another.
 * workspace: 16-byte aligned, workspace_bytes >= 32 * M * K (a record of 32 bytes per candidate).
 * CRD_E_INVALID, nothing launched: NULL pose, vw, arc, tau, origin, cost, workspace, best, command, score or info; tracks without pos
 * or vel; some but not all of the five tables; pose, vw, arc, tau, origin, pos, vel, twist, command, score, scores or xy not 8-byte
 * aligned, togo, tracks, best, info, first_blocked, first_track, max_cost or end_togo not 4-byte, the workspace not 16-byte; M outside
 * 1 .. 65535; n_v outside 1 .. 64; n_w even or outside 1 .. 129; K > 4096; P outside 1 .. 256; nx or ny outside 1 .. 65535; M * nx * ny
 * >= 2^31; blocked_at outside 1 .. 255; outside_blocks neither 0 nor 1; cell not finite and positive; min_speed2 or keep_out2 negative
 * or not finite; with a twist a_v_dt or a_w_dt negative or NaN; T outside 0 .. 1024, T > 0 without tracks or T == 0 with them;
 * min_status outside 0 .. 2; max_object_cells < 0; a weight outside 0 .. 32767; a workspace too small.
 * ------------------------------------------------------------------------------------------- */
int crd_plan_rollouts(const double* pose, const double* vw, const double* arc, const double* tau, int32_t M, int32_t n_v, int32_t n_w,
                      int32_t P, const int64_t* origin, uint64_t cell_f64_bits, const uint8_t* cost, const int32_t* togo, int32_t nx,
                      int32_t ny, int32_t blocked_at, int32_t outside_blocks, const int32_t* tracks, const double* pos, const double* vel,
                      int32_t T, int32_t min_status, int32_t max_object_cells, uint64_t min_speed2_f64_bits, uint64_t keep_out2_f64_bits,
                      const double* twist, uint64_t a_v_dt_f64_bits, uint64_t a_w_dt_f64_bits, int32_t w_togo, int32_t w_max_cost,
                      int32_t w_sum_cost, int32_t w_slow, int32_t w_turn, void* workspace, int64_t workspace_bytes, int32_t* best,
                      double* command, int64_t* score, int32_t* info, int64_t* scores, int32_t* first_blocked, int32_t* first_track,
                      int32_t* max_cost, int32_t* end_togo, double* xy, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Visualisation back end: float maps, label maps and the radar channel -> uint8 RGB pictures ("Visualisation back
 * end"; the reference's src/visualization/visualization.py:102-151 without its PNG files).  No allocation, no synchronisation,
 * capturable in a graph on one stream, arguments checked before any GPU call.  The three entries add no struct and change no
 * signature: CRD_ABI_VERSION stays.  tests/viz_ref.py restates the arithmetic in NumPy; the kernels agree with it bit for bit.
 *
 * A map is fp32 [B][h][w] (kind CRD_VIZ_FLOAT) or uint8 [B][h][w] (kind CRD_VIZ_LABELS).  Its colour is a row of table, uint8
 * [256][3] (R, G, B) on the device.  With (vmin, vmax) the frame's range, both fp32:
 *   float map: the map and the scaling are fp32, the range is held in fp64 -- matplotlib 3.10 keeps vmin / vmax as Python floats and
 *   NumPy 2 then takes the fp64 loop for `fp32 array -= fp64 scalar` and `/=`, rounding each result into the fp32 array:
 *     t = (float)((double)x - (double)vmin);  q = (float)((double)t / ((double)vmax - (double)vmin));  y = q * 256   (fp32)
 *   labels, all in fp64 (matplotlib promotes integer input):  y = ((double)l - vmin) / ((double)vmax - vmin) * 256
 *   row = 255 where y >= 256 (so x == vmax is the last row), trunc(y) where 0 <= y < 256, 0 otherwise (y < 0 and NaN);
 *   vmin == vmax: row 0 for every pixel.  This is what matplotlib's plt.imsave(cmap=) writes, alpha dropped.
 * A non-finite pixel of a float map is left out of the range and drawn in bad_rgb (matplotlib turns the whole frame "bad").
 *
 * There are three entries where the per-frame range, the drawing and the arg-max make three kinds of launch.  crd_seg_argmax above is
 * Seg_Block's normalised arg-max into a pixel-major channel; the label map the pictures and crd_point_cloud take is crd_seg_labels.
 * ------------------------------------------------------------------------------------------- */
#define CRD_VIZ_TILE 1024      /* pixels of one frame per workgroup of the range pass and per workspace entry */
#define CRD_VIZ_FLOAT 0
#define CRD_VIZ_LABELS 1
#define CRD_VIZ_NONE 0         /* out = colour */
#define CRD_VIZ_PASTE 1        /* out = colour where x > 0 (l > 0), the image elsewhere            visualization.py:108,141 */
#define CRD_VIZ_BLEND 2        /* out = clamp(rint(img * alpha + colour * beta), 0, 255)            visualization.py:150 */
#define CRD_VIZ_IMAGE 3        /* out = the image in R, G, B order (grey applies); src, table and the range are not read */
/* range[b] = (vmin, vmax), fp32 [B][2]: the smallest and the largest finite value of frame b, (0, 0) when it has none; labels are
 * converted to fp32 (exact).  The same bits every run: minimum and maximum of monotone integer keys, per tile of CRD_VIZ_TILE pixels
 * of one frame into the workspace, then folded by one workgroup per frame; no atomic, no workgroup waits for another.
 * dilate = 0: the range of src itself.  dilate = k, odd, 1 <= k <= 9 (float maps only): src is the normalised radar depth r (input
 * channel 3); t = 1 - r where r != 0 and r is finite, else 0 (visualization.py:135); dilated[b][r][c] = the maximum of t over the part
 * of the k x k window around (r, c) that lies inside the frame (cv2.dilate's default border, visualization.py:137); dilated, fp32
 * [B][h][w], is written in full and the range is that of dilated.
 * workspace: 8-byte aligned, workspace_bytes >= 8 * B * ceil(h * w / CRD_VIZ_TILE).  A float src, dilated and range are 4-byte aligned;
 * 16-byte aligned maps of a multiple of four pixels per frame take the vector loads.
 * CRD_E_INVALID: a NULL src, workspace or range (or dilated with dilate != 0); B, h or w <= 0; kind not 0 or 1; dilate even, negative,
 * above 9 or given with labels; a workspace too small; misaligned pointers.  CRD_E_UNSUPPORTED: h * w or the number of tiles beyond the
 * 32-bit indices. */
int crd_viz_range(const void* src, int32_t kind, int32_t B, int32_t h, int32_t w, int32_t dilate, float* dilated, void* workspace,
                  int64_t workspace_bytes, float* range, crd_stream_t stream);
/* The one drawing launch: out[b][r][c] = 3 bytes R, G, B at out + b * out_frame_pitch + r * out_row_pitch + 3 * c (pitches in bytes), so
 * out may be a panel of a larger canvas; bytes outside the h x 3w rectangles are not touched.
 * range: fp32 [B][2] on the device (crd_viz_range's, or the caller's own, e.g. smoothed over time), or NULL: every frame takes vmin and
 * vmax (finite, vmin <= vmax).  bad_rgb: R | G << 8 | B << 16.
 * image: uint8 [B][h][w][3], the layout of crd_assemble_input, in B, G, R order (image_bgr != 0, "as cv2 reads it") or R, G, B; NULL
 * with CRD_VIZ_NONE.  grey != 0: the image is first replaced by (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15 in all three channels
 * (visualization.py:131-132; the 15-bit fixed point of 0.299 / 0.587 / 0.114).  CRD_VIZ_BLEND, per channel in fp32, each operation
 * rounded on its own: t = img * alpha, u = colour * beta, s = t + u, then round half to even and clamp to 0 .. 255 (|alpha|, |beta| <=
 * 1e30).  Blend and grey are this definition; they are not pinned to OpenCV's.
 * Map, image and table are read once; four pixels make three dword stores when w is a multiple of 4, src is 16-byte (labels: 4-byte)
 * aligned and image, out and both pitches are multiples of 4, byte stores otherwise.
 * CRD_E_INVALID: NULL out, src or table (unless CRD_VIZ_IMAGE), image (unless CRD_VIZ_NONE); B, h or w <= 0; kind or mode out of range;
 * out_row_pitch < 3 * w; B > 1 and out_frame_pitch < (h - 1) * out_row_pitch + 3 * w; without range vmin or vmax not finite or vmax <
 * vmin; alpha or beta out of range; bad_rgb outside 24 bits; a misaligned range or float map.  CRD_E_UNSUPPORTED as above. */
int crd_viz_draw(const void* src, int32_t kind, int32_t B, int32_t h, int32_t w, const uint8_t* table, const float* range, float vmin,
                 float vmax, int32_t bad_rgb, const uint8_t* image, int32_t image_bgr, int32_t mode, float alpha, float beta,
                 int32_t grey, uint8_t* out, int64_t out_row_pitch, int64_t out_frame_pitch, crd_stream_t stream);
/* labels[b][r][c] = the first index of the maximum of logits[b][.][r][c] (fp32 [B][C][h][w], 1 <= C <= 256; labels uint8 [B][h][w]); a
 * NaN counts as larger than everything and the first NaN wins: np.argmax(axis=1), torch.max(dim=1)[1] (visualization.py:120).
 * CRD_E_INVALID: NULL pointers, B, h or w <= 0, C outside 1 .. 256, logits not 4-byte aligned. */
int crd_seg_labels(const float* logits, int32_t B, int32_t C, int32_t h, int32_t w, uint8_t* labels, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Camera front end: raw camera frames -> the network's image ("Camera front end").  The reference makes its `_im`
 * image offline (scripts/prepare_flow_im.py:18-26, downsample_im): skimage.transform.resize(im, (H / 2, W / 2, 3), order=1,
 * preserve_range=True, anti_aliasing=False).astype('uint8')[y_cutoff:] on the host in fp64.  One launch, no allocation, no
 * synchronisation, capturable in a graph on one stream, arguments checked before any GPU call.  The entry adds no struct and changes
 * no signature: CRD_ABI_VERSION stays.  tests/camera_ref.py restates the arithmetic in NumPy; the kernel agrees with it bit for bit.
 *
 * frames: uint8, B frames of im_h x im_w pixels of `channels` (3 or 4) bytes; pixel (y, x) of frame b begins at
 * frames + b * frame_pitch + y * row_pitch + x * channels (pitches in bytes: a strided capture buffer needs no copy) and a fourth
 * byte (alpha, padding) is ignored.  swap_rb != 0: stored channel k reads source byte 2 - k (frames in R, G, B as skimage.io.imread
 * gives them, the network trained on cv2.imread's B, G, R); else byte k.
 * Geometry, as for the other ends, s = downsample_scale: h_new = im_h / s, w_new = im_w / s, h = h_new - y_cutoff, w = w_new.
 * Output pixel (r, c), stored channel k, with R = r + y_cutoff and p[y][x] the source byte of that channel:
 *   s even, o = s / 2 - 1:  v = (p[R*s+o][c*s+o] + p[R*s+o][c*s+o+1] + p[R*s+o+1][c*s+o] + p[R*s+o+1][c*s+o+1]) >> 2
 *   s odd:                  v = p[R*s + s/2][c*s + s/2]
 * This is scikit-image 0.19.3's resize(order=1, anti_aliasing=False) -> scipy.ndimage.zoom(order=1, grid_mode=True) where s divides
 * the frame: the sample point (R + 0.5) * s - 0.5 then lies midway between the two central pixels (even s: four weights of 1/4, the
 * sum exact in fp64) or on a pixel (odd s), and astype('uint8') truncates.  s outside 1 .. 4 is refused.
 * Outputs (either may be NULL, not both):
 *   image_u8  uint8 [B][h][w][3], the layout of crd_assemble_input, of crd_point_cloud's image and of crd_viz_draw's
 *   x         fp32 [B][x_channels][h][w], channels 0 .. 2 only: (v / 255 - mean[k]) / std[k], crd_assemble_input's own expression and
 *             constants, indexed by the stored channel k -- the bits of crd_assemble_input on image_u8; channels >= 3 are not touched
 * With s = 2, 3 channels and frames, row_pitch and frame_pitch multiples of 16, a thread makes eight adjacent pixels from three
 * 16-byte loads of each of the two source rows; everything else, and the tail of a row, goes pixel by pixel.  Same bytes either way.
 * CRD_E_INVALID: NULL frames; both outputs NULL; B, im_h or im_w <= 0; channels not 3 or 4; row_pitch < im_w * channels; frame_pitch <
 * im_h * row_pitch; downsample_scale outside 1 .. 4; y_cutoff outside 0 .. h_new - 1; x with x_channels < 3; x not 4-byte aligned.
 * CRD_E_UNSUPPORTED: im_h % s or im_w % s non-zero (the zoom factor is then not 1 / s and the rule above is not skimage's); B * h * w *
 * max(3, x_channels) beyond the 32-bit indices.
 * ------------------------------------------------------------------------------------------- */
int crd_camera_frontend(const uint8_t* frames, int32_t B, int32_t im_h, int32_t im_w, int32_t channels, int64_t row_pitch,
                        int64_t frame_pitch, int32_t swap_rb, int32_t downsample_scale, int32_t y_cutoff, uint8_t* image_u8, float* x,
                        int32_t x_channels, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Losses (src/utils/loss_funcs.py:14-46,77-91; combination src/main/runner.py:197-218).
 * ------------------------------------------------------------------------------------------- */
/* acc[0] += sum smooth_l1(pred-target), acc[1] += #(target>0), acc[2] += sum (target-pred)^2 ; crd_sum_t with
 * CRD_STAT_FRAC_BITS (so that a SUM all-reduce over ranks stays exact); caller zeroes acc */
int crd_masked_l1_fwd(const float* pred, const float* target, int64_t n, crd_sum_t* acc, crd_stream_t stream);
/* Trainer.test metrics (runner.py:443-465) for `frames` fp32 maps of n pixels each, without a host sync per frame:
 * p = clip(pred,0,1)*max_depth, g = gt*max_depth with g > max_distance dropped; on g > 0:
 * acc[f][0] += sum |p-g|, acc[f][1] += sum (p-g)^2, acc[f][2] += sum |p-g|/g, acc[f][3] += count   (crd_sum_t,
 * CRD_STAT_FRAC_BITS; caller zeroes acc;
 * MAE = acc0/acc3, RMSE = sqrt(acc1/acc3), REL = acc2/acc3; frames with acc3 == 0 are skipped by the reference) */
int crd_test_metrics(const float* pred, const float* gt, int32_t frames, int64_t n, float max_depth, float max_distance,
                     crd_sum_t* acc, crd_stream_t stream);
/* Per-frame confusion matrices for the Jaccard index of Trainer.test (runner.py:432-436, torchmetrics 0.10.2
 * JaccardIndex(num_classes=C, ignore_index=255)): prediction = arg-max over the C fp32 logits [frames][C][HW],
 * confmat[f][target][pred] += 1 (int64 [frames][C][C], caller zeroes); labels outside [0, C) are skipped and counted
 * in out_of_range[f] (torchmetrics raises ValueError on them, which the reference catches: that frame's IoU is NaN). */
int crd_seg_confusion(const float* logits, const int64_t* labels, int32_t frames, int32_t C, int64_t HW, int64_t* confmat,
                      int64_t* out_of_range, crd_stream_t stream);
/* The standard depth-evaluation sums (threshold accuracies, AbsRel, SqRel, RMSE(log), SILog, iRMSE / iMAE, ...) of `frames` fp32
 * maps of n pixels each, binned by TRUE distance so that one pass serves every distance cap; no host sync.
 * pred, gt: normalised INVERTED depth (gt = (max_depth - d) / max_depth for a lidar hit, 0 = no hit).  Per pixel, in fp32, every
 * statement rounded on its own (no contraction into fused multiply-adds):
 *   dg    = max_depth * (1.0f - gt)                                        the true distance in metres
 *   valid = gt > 0 and dg >= min_depth
 *   dp    = min(max(max_depth * (1.0f - clamp(pred, 0, 1)), min_depth), max_depth)      (a NaN pred stays NaN through the clamps)
 *   bin   = min(n_bins - 1, (int)floorf(dg / bin_width)),   n_bins = ceil(max_depth / bin_width)
 *   e = dp - dg,  r = logf(dp) - logf(dg),  q = 1/dp - 1/dg,  m = max(dp/dg, dg/dp)
 * acc[f][bin][c] += (CRD_EVAL_COLUMNS columns, caller zeroes acc)
 *   0 count   1 |e|   2 e^2   3 |e|/dg   4 e^2/dg   5 r   6 r^2   7 |q|   8 q^2   9 #(m < 1.25)   10 #(m < 1.25^2)   11 #(m < 1.25^3)
 * For a cap c (a multiple of bin_width) add the bins below c / bin_width; with n = column 0 and s1..s11 the others:
 *   MAE = s1/n, RMSE = sqrt(s2/n), AbsRel = s3/n, SqRel = s4/n, RMSElog = sqrt(s6/n), SILog = 100 sqrt(max(0, s6/n - (s5/n)^2)),
 *   iMAE = 1000 s7/n and iRMSE = 1000 sqrt(s8/n) (1/km), delta_k = s(8+k)/n.
 * acc is crd_sum_t with ONE FIXED-POINT SCALE PER COLUMN: value = acc * 2^-CRD_EVAL_FRAC_BITS[c] (the 2^-20 grid of
 * CRD_STAT_FRAC_BITS is too coarse for a per-pixel |q| of 1e-3).  Every per-pixel term is rounded once to its column's grid and
 * added as an integer (a table per workgroup in LDS, then one 64-bit integer add per non-zero entry): the sums do not depend on
 * the order of arrival, and two calls give identical bits.  A term that is not finite or whose scaled magnitude reaches 2^62
 * adds nothing and raises the sticky flag (crd_nonfinite_status).  Ranges per (frame, bin) -- |sum| < 2^(63 - bits) -- and the
 * largest per-pixel term at max_depth = 100, min_depth = 1e-3 (dg, dp in [1e-3, 100]):
 *   column  bits  grid      sum below   largest term            928 x 1600 all-valid pixels (1.48e6) in ONE bin
 *   1       32    2.3e-10   2.1e9       100                     1.5e8   fits
 *   2       26    1.5e-8    1.4e11      1e4                     1.5e10  fits
 *   3       24    6.0e-8    5.5e11      1e5                     1.5e11  fits
 *   4       24    6.0e-8    5.5e11      1e7                     1.5e13  DOES NOT fit in the worst case: the sum of e^2/dg over a
 *                                                               (frame, bin) must stay below 5.5e11 m, a mean of 3.7e5 m over such a
 *                                                               frame -- held whenever no ground truth is closer than 2.7 cm
 *   5       36    1.5e-11   1.3e8       11.6                    1.7e7   fits
 *   6       33    1.2e-10   1.1e9       133                     2.0e8   fits
 *   7       31    4.7e-10   4.3e9       1e3                     1.5e9   fits
 *   8       40    9.1e-13   8.4e6       1e6                     1.5e12  DOES NOT fit in the worst case: the sum of q^2 over a
 *                                                               (frame, bin) must stay below 8.4e6 m^-2, a mean of 5.6 m^-2 over
 *                                                               such a frame (an rms inverse-depth error of 2.4 per metre)
 *   0, 9-11 0     1         9.2e18      1
 * A sum that leaves its range wraps around silently (the per-term guard cannot see the total): columns 4 and 8 are the ones to
 * watch with ground truth at centimetres.
 * CRD_E_INVALID before any launch: NULL pred / gt / acc; frames <= 0; n <= 0; max_depth, min_depth or bin_width not finite and
 * > 0; min_depth >= max_depth; n_bins != ceil(max_depth / bin_width) or > CRD_EVAL_MAX_BINS.  CRD_E_UNSUPPORTED: frames > 65535
 * or n >= 2^35.  No read past frames * n elements; 64-bit indexing; any alignment of pred / gt and any n. */
#define CRD_EVAL_COLUMNS 12
#define CRD_EVAL_MAX_BINS 64
static const int CRD_EVAL_FRAC_BITS[CRD_EVAL_COLUMNS] = {0, 32, 26, 24, 24, 36, 33, 31, 40, 0, 0, 0};
int crd_depth_eval(const float* pred, const float* gt, int32_t frames, int64_t n, float max_depth, float min_depth, float bin_width,
                   int32_t n_bins, crd_sum_t* acc /* [frames][n_bins][12], caller zeroes */, crd_stream_t stream);
/* dpred = gmul * gout[0] * clamp(pred-target,-1,1) / acc[1] on target>0, else 0   (gout may be NULL = 1) */
int crd_masked_l1_bwd(const float* pred, const float* target, int64_t n, const crd_sum_t* acc, const float* gout,
                      float gmul, float* dpred, crd_stream_t stream);
/* NCHW fp32 logits [B][C][HW], int64 labels [B][HW], ignore_index 255:
 * acc[0] += sum -log softmax[label], acc[1] += #valid, acc[2] += #out-of-range (all three crd_sum_t, CRD_STAT_FRAC_BITS).
 * A label that is neither 255 nor in [0, C) is OUT OF RANGE (torch raises on it): it is never used to form an address, adds
 * nothing to acc[0] and acc[1], gets a zero gradient from crd_ce_focal_bwd, and is counted in acc[2] -- the caller decides;
 * MaskedFocalLoss and TrainStep.losses() raise on a non-zero count.  The call owns acc[0..2]. */
int crd_ce_fwd(const float* logits, const int64_t* labels, int32_t B, int32_t C, int64_t HW, crd_sum_t* acc,
               crd_stream_t stream);
/* focal on the scalar mean CE (loss_funcs.py:27-29): dlogits = gmul*gout[0]*dF/dce*(softmax-onehot)/acc[1] on the valid pixels,
 * 0 on ignored and out-of-range ones (gout may be NULL = 1) */
int crd_ce_focal_bwd(const float* logits, const int64_t* labels, int32_t B, int32_t C, int64_t HW, const crd_sum_t* acc,
                     const float* gout, float gmul, float* dlogits, crd_stream_t stream);

/* More depth criteria (loss_funcs.py:49-59,118-180; camradepth_amd/csrc/losses.hip, as every loss above).  MaskedHuberLoss
 * (nn.HuberLoss, delta = 1) is smooth-L1 with beta = 1 and runs crd_masked_l1_fwd / _bwd.  d = pred - target over target > 0;
 * crd_sum_t sums with CRD_STAT_FRAC_BITS, zeroed by the caller. */
/* MaskedL1Loss / MaskedRMSELoss: acc[0] += sum |d|, acc[1] += #(target>0), acc[2] += sum d^2
 * (L1 = acc0/acc1, RMSE = sqrt(acc2/acc1)) */
int crd_masked_dist_fwd(const float* pred, const float* target, int64_t n, crd_sum_t* acc, crd_stream_t stream);
/* mode 0 (L1):   dpred = gmul * gout[0] * sign(d) / acc[1]   (sign(0) = 0, as torch's abs backward)
 * mode 1 (RMSE): dpred = gmul * gout[0] * d / (acc[1] * rmse)   (NaN on the mask when rmse = 0, as torch's sqrt backward)
 * 0 where target <= 0; gout may be NULL = 1 */
int crd_masked_dist_bwd(const float* pred, const float* target, int64_t n, const crd_sum_t* acc, const float* gout,
                        float gmul, int32_t mode, float* dpred, crd_stream_t stream);
/* MaskedBerHuLoss, phase (a): *maxbits = max(*maxbits, bits of max |d|) (the fp32 bit pattern of a non-negative value; an
 * integer MAX all-reduce of it is the global max; caller zeroes it), acc[1] += #(target>0), acc[2] += sum d^2 (acc[0] untouched). */
int crd_masked_berhu_max(const float* pred, const float* target, int64_t n, crd_sum_t* acc, int32_t* maxbits, crd_stream_t stream);
/* MaskedBerHuLoss, phase (b), with c = thresh * (fp32 at maxbits) in fp64 (the global max after an all-reduce) and count = acc[1].
 * thresh is a double passed as its IEEE-754 bit pattern (the reference's delta is an fp64 product; the C ABI's argument types are
 * pointers, int32 / int64 / uint64 and float).  The reference's fp32 edges:
 *   part1 = |d| if |d| < fp32(c) else 0,  part2 = |d|^2 / (2c) if fp32(|d|^2) - fp32(c^2) > 0 else 0  (F.threshold's strict
 *   comparisons: |d| == c contributes nothing and gets no gradient);
 * loss (optional, crd_sum_t[2]): loss[0] += sum part1, loss[1] += sum of part2's numerators; the loss is
 *   (loss[0] + loss[1] / (2c)) / acc[1] -- NaN when c = 0 (all |d| equal to 0) or the mask is empty;
 * dpred (optional) = gmul * gout[0] * sign(d) * (1 if |d| < c, |d| / c if part2 applies, else 0) / acc[1], 0 where target <= 0
 * (zero everywhere when c = 0).  At least one of loss / dpred; thresh finite and > 0. */
int crd_masked_berhu(const float* pred, const float* target, int64_t n, const crd_sum_t* acc, const int32_t* maxbits,
                     uint64_t thresh_f64_bits, crd_sum_t* loss, const float* gout, float gmul, float* dpred, crd_stream_t stream);
/* SmoothnessLoss: pred [B][1][H][W], image [B][C][H][W] fp32, H, W >= 2.  n = pred / (per-sample mean + 1e-7), edge weights
 * exp(-mean_c |image difference|); acc crd_sum_t[B][3]: acc[b][0] += sum pred_b, acc[b][1] += sum over x-neighbours of
 * w |n_j - n_j+1|, acc[b][2] += the same over y-neighbours (two launches).  loss = sum_b acc[b][1] / (B H (W-1)) +
 * sum_b acc[b][2] / (B (H-1) W). */
int crd_smoothness_fwd(const float* pred, const float* image, int32_t B, int32_t C, int32_t H, int32_t W, crd_sum_t* acc,
                       crd_stream_t stream);
/* dpred = gmul * gout[0] * dloss/dpred including the term through the per-sample mean (from the forward's acc; no reduction).  The
 * image gets no gradient.  Under data parallelism gmul = local B / global B makes the denominators the gathered batch's. */
int crd_smoothness_bwd(const float* pred, const float* image, int32_t B, int32_t C, int32_t H, int32_t W, const crd_sum_t* acc,
                       const float* gout, float gmul, float* dpred, crd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * diffGradNorm.step (src/models/diffGradNorm.py:41-113) over flat fp32 buffers: one descriptor, three entry points.
 * Three independent switches, each a nullable pointer of the descriptor: gate (skip_nonfinite), clip (max_grad_norm), ema
 * (ema_decay).  Which kernel instantiations run follows from gate != NULL, clip != NULL, ema != NULL and nothing else.
 *
 * Layout.  Tensor t occupies [seg_off[2t], seg_off[2t+1]) of every flat buffer (int64 pairs; gaps allowed).  Workgroup w processes
 * chunk blk2chunk[w] (4096 elements) of tensor blk2seg[w]; the workgroups of a tensor are consecutive and in chunk order.
 * exp_grad_norm / factor are float[n_tensors].  active[t]=0 skips tensor t (`p.grad is None`, :54-55); NULL = all active.  `step` is
 * the 1-based step count used for the bias corrections.
 * parts is scratch: without clip float[n_blocks], ONE row: workgroup w stores its part of ||g||^2 = sum (g + wd p)^2 in parts[w] and
 * one wave per tensor adds its workgroups' parts in a fixed order (reproducible; the e > n branch of diffGradNorm.py:84 turns
 * rounding noise into a discrete jump).  With clip float[4 * parts_stride], four rows of per-workgroup parts: [0] sum (g + wd p)^2
 * (the row above), [1] sum g^2, [2] sum g p and [3] sum p^2 (rows 2 and 3: with weight decay only).  parts_stride is read with clip
 * only.
 * hp_dev (optional, device float[5] = beta1, beta2, eps, weight_decay, lr*sqrt(1-beta2^t)/(1-beta1^t+1e-8)) overrides the scalar
 * fields so that a captured HIP graph can follow a per-iteration schedule.  With gate or ema it is float[16], see below.
 *
 * crd_diffgradnorm_norm: k_dgn_norm's pass over the blocks given.  It reads only p, g, parts, parts_stride, seg_off, blk2seg,
 * blk2chunk, n_blocks, active, weight_decay, hp_dev, gate and clip (as a flag) and demands nothing else.  One bucket may be passed
 * at a time: parts / blk2seg / blk2chunk then point at that bucket's first block, n_blocks is the bucket's count and parts_stride
 * stays the full count.  With gate it also tests every gradient element for finiteness; with clip it also writes rows 1-3.
 * crd_diffgradnorm_commit: [with clip: total + coefficient,] the per-tensor scalars and the update over ALL blocks.
 * crd_diffgradnorm_step: norm, then commit, with the same descriptor.
 *
 * gate (skip_nonfinite, GradScaler.step semantics): nothing is written when the window saw a non-finite gradient.  Device int32[8],
 * zeroed by the caller except for the counters: [0] a gradient element was NaN / inf (set by crd_diffgradnorm_norm), [1] a crd_sum_t
 * partial was dropped during the window's backward (crd_nonfinite_capture), [2] committed steps, [3] skipped steps, [4] the verdict
 * of the last window (1 = skipped), [5] scratch (the step size in use).  The commit writes every tensor's scalar and update, or
 * none.  Bias corrections: `step` / lr / beta1 / beta2 when hp_dev is NULL (the host knows every verdict); with hp_dev, hp_dev[4]
 * as long as the device count of this step equals the host's step number (int32 at hp_dev[14]), otherwise computed on the device
 * in fp64 from the fp64 lr, beta1, beta2 at hp_dev[8..13].  hp_dev is then float[16].
 *
 * clip (max_grad_norm): the optimizer step behind torch.nn.utils.clip_grad_norm_(params, max_norm): every gradient is scaled by
 * coef = min(1, max_norm / (total + 1e-6)), total = the 2-norm over all blocks, before the weight decay is added; the norm,
 * exp_avg, exp_avg_sq and previous_grad all see the scaled gradient.  The gradient buffer itself is not written.  The commit: ONE
 * workgroup adds row 1 over all n_blocks in a fixed order in fp64 and writes clip[0] = total, clip[1] = coef (device float[2];
 * torch's fp32 coefficient, a NaN total gives NaN), then the per-tensor scalars (from row 0 when coef == 1, else from rows 1-3) and
 * the update.  coef == 1 gives the bits of the step without clip.  Row 1 is added over the commit's n_blocks, so commit and step
 * require parts_stride == n_blocks with clip: a commit over one bucket's slice would clip with a partial norm.  max_norm > 0; +inf
 * gives coef = 1 (the total only).  With gate: the gate's semantics above (gate[0] set by the norm pass).
 *
 * ema (ema_decay): an exponential moving average of the parameters updated in the same pass; a device fp32 buffer with the layout
 * of p.  For every element the update kernel writes (active tensors of a committed step only), in fp32:
 *            d_n = ema_warmup ? fminf(ema_decay, (float)(1 + n) / (float)(10 + n)) : ema_decay;   w_n = 1.0f - d_n;
 *            ema = fmaf(w_n, p_new - ema, ema)          (p_new: the value stored to p; 0 <= ema_decay < 1)
 * n = 1, 2, ... counts the committed steps since the EMA was created or restored.  Without a gate the host knows it: ema_n = n, or
 * with hp_dev the host leaves w_n itself in hp_dev[5] (ema_n is then ignored), so a captured graph follows n without re-capture.
 * With a gate only the device knows which steps were committed: n = gate[2] (after this step's verdict) - ema_base, w_n is formed
 * on the device by the expression above; with hp_dev, ema_decay / ema_base / ema_warmup are read from hp_dev[6], the int32 at
 * hp_dev[7] and the int32 at hp_dev[15].  ema_n is read without a gate only, ema_base with one only.
 * Everything else -- p, the optimizer state, the status codes -- is what the call with ema = NULL does, bit for bit.
 *
 * CRD_E_INVALID before any launch: a NULL descriptor, buffer or table, n_blocks <= 0; commit / step: n_tensors <= 0, step < 1; clip:
 * parts_stride < n_blocks, and on commit / step max_norm not > 0 (NaN included) or parts_stride != n_blocks; ema on commit / step:
 * ema_decay outside [0, 1), ema_base < 0 with a gate, ema_n < 1 without one (ema_n < 0 with hp_dev).
 * ------------------------------------------------------------------------------------------- */
typedef struct crd_dgn_desc {
  float* p; const float* g; float* exp_avg; float* exp_avg_sq; float* prev_grad; float* exp_grad_norm; float* factor;
  float* parts;                                       /* per-workgroup norm parts: 1 row, with clip 4 rows parts_stride apart */
  const int64_t* seg_off; const int32_t* blk2seg; const int32_t* blk2chunk;
  const uint8_t* active;                              /* nullable */
  const float* hp_dev;                                /* nullable: overrides the scalars below */
  int32_t* gate;                                      /* NULL = ungated */
  float* clip;                                        /* NULL = no clipping; [total, coef] */
  float* ema;                                         /* NULL = no EMA */
  int64_t parts_stride;
  int32_t n_tensors, n_blocks;
  float lr, beta1, beta2, eps, weight_decay;
  int32_t step;
  float max_norm;
  float ema_decay;
  int32_t ema_warmup, ema_n, ema_base;
} crd_dgn_desc;
int crd_diffgradnorm_norm(const crd_dgn_desc* d, crd_stream_t stream);
int crd_diffgradnorm_commit(const crd_dgn_desc* d, crd_stream_t stream);
int crd_diffgradnorm_step(const crd_dgn_desc* d, crd_stream_t stream);
/* a[i] <-> b[i] for i < n, in place (no temporary): two fp32 buffers that do not overlap, any 4-byte alignment (16-byte loads and
 * stores where both buffers allow them, single elements at the ends); n = 0 does nothing.  Exchanges the parameters with their EMA. */
int crd_swap_f32(float* a, float* b, int64_t n, crd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
