"""ctypes binding of libcamradepth_hip.so (include/camradepth_hip.h).

The product path has no fallback: if the shared library is missing or a call fails, this module
raises.  PyTorch is used only to own device memory and streams.
"""
import ctypes as C
import os
import struct

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRD_LIB: load another build of the library (developer builds with profiling stamps -- tools/prof_*.sh link them to their own
# file instead of overwriting the product library)
LIB_PATH = os.environ.get("CRD_LIB") or os.path.join(_HERE, "libcamradepth_hip.so")


class CrdError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x_ld", C.c_int32), ("x_coff", C.c_int32),
        ("B", C.c_int32), ("IH", C.c_int32), ("IW", C.c_int32), ("Cin", C.c_int32),
        ("w", C.c_void_p), ("Cout", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32),
        ("stride", C.c_int32), ("pad", C.c_int32), ("OH", C.c_int32), ("OW", C.c_int32),
        ("gather_mode", C.c_int32),
        ("y", C.c_void_p), ("y_ld", C.c_int32), ("y_coff", C.c_int32), ("y_f32", C.c_int32),
        ("out_mode", C.c_int32), ("patch_k", C.c_int32), ("patch_c", C.c_int32),
        ("bias", C.c_void_p), ("bias_bstride", C.c_int32), ("act", C.c_int32),
        ("res", C.c_void_p), ("res_ld", C.c_int32), ("res_scale", C.c_void_p),
        ("accumulate", C.c_int32), ("stats", C.c_void_p),
        ("stats_partial", C.c_void_p), ("stats_partial_capacity", C.c_int64),
        ("red_x", C.c_void_p), ("red_x_ld", C.c_int32), ("red_gmul", C.c_int32), ("red_act", C.c_int32),
        ("red_x_f32", C.c_int32), ("red_stats", C.c_void_p), ("red_gamma", C.c_void_p), ("red_beta", C.c_void_p),
        ("red_r", C.c_void_p), ("chan_sums", C.c_void_p),
    ]


class GnInput(C.Structure):
    _fields_ = [("x_f32", C.c_int32), ("gmul", C.c_int32), ("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("act", C.c_int32), ("xn_ld", C.c_int32), ("xn", C.c_void_p)]


class GnBwdInput(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gx_f32", C.c_int32), ("gx_ld", C.c_int32), ("gmul", C.c_int32), ("act", C.c_int32),
                ("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("mask", C.c_void_p), ("r", C.c_void_p),
                ("dx", C.c_void_p), ("dx_ld", C.c_int32), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p)]


class WgradDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x_ld", C.c_int32), ("x_coff", C.c_int32),
        ("B", C.c_int32), ("IH", C.c_int32), ("IW", C.c_int32), ("Cin", C.c_int32),
        ("dy", C.c_void_p), ("dy_ld", C.c_int32), ("dy_coff", C.c_int32),
        ("OH", C.c_int32), ("OW", C.c_int32), ("Cout", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("dw", C.c_void_p), ("dbias", C.c_void_p), ("dw_partials", C.c_void_p), ("dw_partial_capacity", C.c_int32), ("wg_budget", C.c_int32),
    ]


class WgradGroupInfo(C.Structure):
    _fields_ = [("n_problems", C.c_int32), ("n_items", C.c_int32 * 4), ("item_offset", C.c_int32 * 4), ("bytes", C.c_int64)]


class PackEntry(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("dst_fwd", C.c_void_p), ("dst_dgrad", C.c_void_p), ("dst_scatter", C.c_void_p),
        ("cmap", C.c_void_p),
        ("Cout", C.c_int32), ("Cin_ref", C.c_int32), ("taps", C.c_int32), ("Cin_pad", C.c_int32),
        ("Cout_pad", C.c_int32), ("dst_f32", C.c_int32),
        ("dgrad_ld", C.c_int32), ("dgrad_coff", C.c_int32), ("dgrad_row0", C.c_int32), ("dgrad_rows", C.c_int32),
    ]


class MlpDesc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x1", "x1_stats", "norm_gamma", "norm_beta", "w_fc1", "b_fc1", "norm1_gamma", "norm1_beta",
                                          "w9", "b_dw", "norm2_gamma", "norm2_beta", "w_fc2", "xn", "h1", "h2", "h3", "h1_stats",
                                          "h2_stats", "fc2_partials")] + \
               [(n, C.c_int32) for n in ("B", "H", "W", "C", "hidden")]


class UnpackEntry(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("dst", C.c_void_p), ("cmap", C.c_void_p),
        ("Cout", C.c_int32), ("Cin_ref", C.c_int32), ("taps", C.c_int32), ("Cin_pad", C.c_int32),
        ("replicas", C.c_int32), ("src_sum", C.c_int32), ("replica_stride", C.c_int64),
    ]


class DgnDesc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("p", "g", "exp_avg", "exp_avg_sq", "prev_grad", "exp_grad_norm", "factor", "parts", "seg_off",
                                          "blk2seg", "blk2chunk", "active", "hp_dev", "gate", "clip", "ema")] + \
               [("parts_stride", C.c_int64), ("n_tensors", C.c_int32), ("n_blocks", C.c_int32)] + \
               [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + \
               [("step", C.c_int32), ("max_norm", C.c_float), ("ema_decay", C.c_float),
                ("ema_warmup", C.c_int32), ("ema_n", C.c_int32), ("ema_base", C.c_int32)]


_lib = None
ABI_VERSION = 13         # include/camradepth_hip.h: CRD_ABI_VERSION


def load():
    """Load the HIP library; raises CrdError when it is not built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CrdError(f"{LIB_PATH} is missing: run `python -m camradepth_amd.build` (hipcc, gfx950). "
                       "camradepth_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.crd_last_error.restype = C.c_char_p
    lib.crd_arch.restype = C.c_char_p
    lib.crd_version.restype = C.c_int
    if lib.crd_version() != ABI_VERSION:
        raise CrdError(f"{LIB_PATH} was built for ABI version {lib.crd_version()}, this binding is version {ABI_VERSION}: rebuild it "
                       "(python -m camradepth_amd.build)")
    missing = [n for n in EXPORTS if not hasattr(lib, n)]
    if missing:
        raise CrdError(f"{LIB_PATH} lacks symbols {missing}: rebuild it (python -m camradepth_amd.build)")
    for name, sig in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [_CT[ch] for ch in sig]
    # developer aids (A/B of a whole test or bench run; CRD_DEV_SWITCHES=1 only): kernel-selection knobs of the C ABI set once at load time
    if os.environ.get("CRD_DEV_SWITCHES") == "1":
        if os.environ.get("CRD_TUNE_REGE") is not None:
            lib.crd_tune_igemm_reg_epilogue(int(os.environ["CRD_TUNE_REGE"]))
        if os.environ.get("CRD_TUNE_NARROW") is not None:
            lib.crd_tune_pw_narrow(int(os.environ["CRD_TUNE_NARROW"]))
    _lib = lib
    return lib


# Signatures of include/camradepth_hip.h (all return int status). p = pointer, i = int32, l = int64, f = float
_SIGS = {
    "crd_conv_igemm": "pp", "crd_conv_igemm_route": "ppi", "crd_gn_conv": "ppp", "crd_gn_conv2": "ppppp", "crd_gn_bwd_conv": "ppp", "crd_pw_narrow_supported": "iii", "crd_tune_pw_narrow": "i", "crd_conv3x3_fp8": "ppfp", "crd_amax_bf16": "pliiipp", "crd_quant_fp8": "pliiipiifp",
    "crd_weight_quant_fp8": "piiiippp", "crd_conv3x3_fp8_dgrad": "pppp", "crd_gn_bwd_apply_fp8": "piiipiiiiiipippipppppiipiippp",
    "crd_fp8_scale_update": "ppifip", "crd_quant_fp8_dev": "pliiipiipp", "crd_tune_conv3x3_small_grid": "i", "crd_tune_igemm_reg_epilogue": "i", "crd_conv_wgrad": "pp", "crd_conv_wgrad_splits": "p", "crd_conv_wgrad_route": "ppi", "crd_wgrad_group_build": "piplp", "crd_conv_wgrad_grouped": "ppp",
    "crd_gn_stats": "piiiiiippp", "crd_gn_apply": "piiiiiipippipPiiip".replace("P", "p"),
    "crd_gn_bwd_reduce": "piiipiiiiiipippippplp", "crd_gn_bwd_apply": "piiipiiiiiipippipppppiiiipipp",
    "crd_gn_launch_shape": "iiiippp",
    "crd_dwconv3x3": "piiiippipppippppppp", "crd_dwconv3x3_wgrad": "ppiiiipipippp",
    "crd_attn_scores": "ppiiiiifppp", "crd_attn_scores_fp8": "ppiiiiffppp", "crd_attn_fwd": "ppiiiiifpppppppppp", "crd_attn_xbar": "ppppiiipp", "crd_attn_xbar_proj": "pppppiiippp", "crd_attn_vec_bwd": "ppiiifppp", "crd_attn_out_residual": "pppppiiipp", "crd_attn_out_residual_stats": "pppppiiippp",
    "crd_attn_out_bwd": "ppppiiipppp", "crd_attn_out_bwd_blocks": "iii", "crd_attn_out_bwd_gn": "ppppiiippppppppppp", "crd_attn_scores_bwd": "ppppiiiiifpppp", "crd_attn_bwd": "ppppiiiiifpppppifppp", "crd_attn_scores_bwd_partials": "iiiii", "crd_sum_partials_bf16": "pilplp", "crd_gsum_to_bf16": "pplp",
    "crd_attn_bwd_fused_supported": "iiiii", "crd_attn_bwd_fused": "ppppppp" "iiiii" "f" "ppppp" "ppppppp" "p", "crd_attn_dk_fold": "pilpl" "pp" "iii" "f" "pp" "p",
    "crd_bicubic2x": "piiiiiipiip", "crd_bicubic2x_fp8": "piiiiiipiifpiip", "crd_gn_apply_fp8": "piiiiiipippippiifpiip", "crd_bicubic2x_bwd": "piiiiiipiiip",
    "crd_input_grad": "ppppiiiiiipp",
    "crd_nchw_to_pm": "piiiipiiip", "crd_pm_to_nchw": "piiiiiiipp", "crd_seg_argmax": "piiiiipiiip", "crd_scale_f32": "pplfp",
    "crd_slice_copy": "piipiiliip", "crd_f32_to_bf16_rows": "pipiiliplpiip", "crd_dropout_masks": "ppiiLpp", "crd_sigmoid_bwd": "pplp", "crd_head_conv2_fwd": "pppiiippiip", "crd_head_conv2_bwd": "ppiippiiippip", "crd_head_conv2_bwd_data": "ppiippiiipp", "crd_head_conv2_wgrad": "ppiipiiipip",
    "crd_weight_pack": "pilp", "crd_wgrad_unpack": "pilip",
    "crd_assemble_input": "pppiiifpp", "crd_gt_pyramid": "piiifppppp",
    "crd_augment_draw": "ppiiiiifffffffiLLp", "crd_augment_lut": "piipp", "crd_augment_assemble": "pppppppiiiiifppppp",
    "crd_augment_gather": "ppppiiiiiippppp", "crd_gt_pyramid_from_full": "piiipppp",
    "crd_radar_project": "pppiipppipiiiffpppppppp", "crd_radar_rasterize": "ppppppppiipiiiiiplppp",
    "crd_lidar_project": "pppiippppippipppipiiiffLLpppppppppp", "crd_lidar_ground_truth": "pppppppppiipiiiiipppipLplpppp",
    "crd_depth_unproject": "piiiiipipiiLLLipppppp", "crd_point_cloud": "piiiiipipiiLLLipppipplpppppp",
    "crd_bev_grid": "ppppiiipiLLLiiLLiiiplppppppp",
    "crd_occupancy_update": "pppiiipipipiiiiLiLLLLiiiiiipppppplpppppp",
    "crd_terrain_update": "pppiii" "pipipi" "iii" "LLLLL" "iiiil" "ppppppp" "pl" "pppppppppp" "p",
    "crd_distance_field": "piiiiiippplppppp", "crd_field_paths": "pppiipLpppiiiiiippppppp",
    "crd_nav_field": "piiippipLiiipppp", "crd_nav_paths": "ppiipLppiiipppppp",
    "crd_map_objects": "piiiiiiipLplpppppp",
    "crd_track_objects": "pppp" "iiiii" "LLLL" "ii" "ppppppppp" "p",
    "crd_match_scan": "ppp" "iii" "pipi" "iii" "LLLL" "i" "ppp" "ii" "p" "il" "pl" "ppppppp" "p",
    "crd_plan_rollouts": "pppp" "iiii" "pLpp" "iiii" "ppp" "iii" "LL" "pLL" "iiiii" "pl" "pppp" "ppppp" "p" "p",
    "crd_viz_range": "piiiiipplpp", "crd_viz_draw": "piiiippffipiiffipllp", "crd_seg_labels": "piiiipp",
    "crd_camera_frontend": "piiiilliiippip",
    "crd_resize_nearest_u8":"piiiipiip", "crd_resize_labels_nearest": "piiiipiip", "crd_seg_confusion": "ppiilppp",
    "crd_masked_l1_fwd": "pplpp", "crd_test_metrics": "ppilffpp", "crd_depth_eval": "ppilfffipp", "crd_masked_l1_bwd": "pplppfpp", "crd_ce_fwd": "ppiilpp",
    "crd_ce_focal_bwd": "ppiilppfpp",
    "crd_masked_dist_fwd": "pplpp", "crd_masked_dist_bwd": "pplppfipp", "crd_masked_berhu_max": "pplppp",
    "crd_masked_berhu": "pplppLppfpp", "crd_smoothness_fwd": "ppiiiipp", "crd_smoothness_bwd": "ppiiiippfpp",
    "crd_diffgradnorm_norm": "pp", "crd_diffgradnorm_commit": "pp", "crd_diffgradnorm_step": "pp",
    "crd_mlp_fused_supported": "iiii", "crd_mlp_fwd": "pp", "crd_mlp_reduce": "pipppiiipppp",
    "crd_nonfinite_status": "ip", "crd_nonfinite_capture": "pp",
    "crd_swap_f32": "pplp",
}
_CT = {"p": C.c_void_p, "i": C.c_int32, "l": C.c_int64, "L": C.c_uint64, "f": C.c_float}
EXPORTS = list(_SIGS)


# crd_sum_t (include/camradepth_hip.h): 64-bit fixed-point accumulators, value = integer * 2^-FRAC_BITS
STAT_FRAC_BITS, GRAD_FRAC_BITS = 20, 44
SUM_DTYPE = torch.int64
# crd_depth_eval: one scale per column of its [frames][bins][12] accumulator (CRD_EVAL_FRAC_BITS), at most CRD_EVAL_MAX_BINS bins
EVAL_FRAC_BITS = (0, 32, 26, 24, 24, 36, 33, 31, 40, 0, 0, 0)
EVAL_MAX_BINS = 64
# crd_augment_draw: words per row of the table, the stream constant xor-ed into the seed, the bits of `enable`
AUGMENT_WORDS, AUGMENT_STREAM = 8, 0xA0761D6478BD642F
AUGMENT_GAMMA, AUGMENT_BRIGHTNESS, AUGMENT_COLOUR = 1, 2, 4


def stat_value(t):
    """float64 value of forward-statistic / loss sums (CRD_STAT_FRAC_BITS)."""
    return t.double() * 2.0 ** -STAT_FRAC_BITS


def grad_value(t):
    """float64 value of gradient sums (CRD_GRAD_FRAC_BITS)."""
    return t.double() * 2.0 ** -GRAD_FRAC_BITS


def nonfinite(reset=True):
    """True if a non-finite (or out-of-range) partial was dropped from a crd_sum_t accumulator since the flag was last cleared
    (include/camradepth_hip.h: crd_nonfinite_status).  The query runs on torch's current stream (behind the kernels enqueued
    there) and waits for it."""
    rc = load().crd_nonfinite_status(1 if reset else 0, stream())
    if rc < 0:
        check(rc, "crd_nonfinite_status")
    return rc == 1


def nonfinite_clear():
    """Clear the sticky flag asynchronously on torch's current stream (no read, no wait): the head of an eager step."""
    check(load().crd_nonfinite_status(2, stream()), "crd_nonfinite_status")


def stat_checked(acc):
    """stat_value(acc) as the reference would report it: NaN in every slot when a non-finite / out-of-range partial was dropped
    from a crd_sum_t sum since the flag was last cleared (the sums are then finite but too small; the reference's float sums
    would be NaN or inf there -- src/utils/loss_funcs.py:85-91 has no guard).  Reads the sticky flag WITHOUT clearing it (round 6,
    ADVICE r5: the first loss of a step used to clear it, so the step's other losses read finite); the eager model forward clears
    it when the next step begins (model.forward -> nonfinite_clear), TrainStep.losses() and the epoch scopes of runner.Trainer
    clear it when they read it.  Waits for the current stream."""
    v = stat_value(acc)
    if nonfinite(reset=False):
        v = torch.full_like(v, float("nan"))
    return v


def f64_bits(x):
    """IEEE-754 bit pattern of a double, for C ABI arguments declared uint64_t ..._f64_bits."""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def check(rc, what=""):
    if rc != 0:
        msg = load().crd_last_error().decode()
        raise CrdError(f"{what} failed with status {rc}: {msg}")


def conv_route(desc):
    """Label of the kernel crd_conv_igemm would launch for this ConvDesc right now (crd_conv_igemm_route: host arithmetic, no GPU)."""
    buf = C.create_string_buffer(96)
    check(load().crd_conv_igemm_route(C.byref(desc), buf, len(buf)), "crd_conv_igemm_route")
    return buf.value.decode()


def wgrad_route(desc):
    """Label of the kernel crd_conv_wgrad would launch for this WgradDesc right now (crd_conv_wgrad_route: host arithmetic, no GPU)."""
    buf = C.create_string_buffer(96)
    check(load().crd_conv_wgrad_route(C.byref(desc), buf, len(buf)), "crd_conv_wgrad_route")
    return buf.value.decode()


def gn_launch_shape(P, Cn, B, kind):
    """(nblk, chunk, batch_pixels) of crd_gn_apply (kind 0) / crd_gn_bwd_apply (kind 1) for B samples of P pixels and Cn channels
    (crd_gn_launch_shape: host arithmetic, no GPU)."""
    out = (C.c_int32 * 3)()
    ptr = [C.cast(C.byref(out, 4 * i), C.c_void_p) for i in range(3)]
    check(load().crd_gn_launch_shape(P, Cn, B, kind, *ptr), "crd_gn_launch_shape")
    return out[0], out[1], out[2]


def stream():
    """Raw hipStream_t of torch's current stream (kernels are enqueued there)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())
