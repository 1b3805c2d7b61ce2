"""Descriptors: the ctypes structs of the C ABI, built from the specs a plan records.

While a plan is recorded a launch's descriptor is a dict (a "spec") that names its kind and refers to tensors that may not be
allocated yet (packed weights, zero-arena slices) or not final (accumulate flags).  Plan._finalise resolves every spec through
make_desc(): one small builder per kind below.  Owns nothing else: no launch is recorded or reordered here."""
import ctypes as C

import torch

from . import lib as L
from .plan_values import PM, ConvW, persistent_conv3


def _p(v):
    if v is None:
        return None
    return v.t.data_ptr() if isinstance(v, PM) else v.data_ptr()


def _conv(plan, sp):
    x, y, w = sp["x"], sp["y"], sp["w"]
    if isinstance(w, tuple) and w[0] == "kcat":
        w = w[2]
    elif isinstance(w, tuple):
        w = w[1].w_dgrad if w[0] == "dgrad" else w[1].w_scatter
        assert w is not None, "packed data-gradient weights were not requested for this convolution"
    elif isinstance(w, ConvW):
        w = w.w_fwd
    d = L.ConvDesc()
    d.x, d.x_ld, d.x_coff, d.B, d.IH, d.IW, d.Cin = _p(x), x.ld, x.coff, plan.B, x.H, x.W, sp["cin"]
    d.w, d.Cout, d.KH, d.KW, d.stride, d.pad = _p(w), sp["cout"], sp["k"], sp["k"], sp["stride"], sp["pad"]
    if sp.get("w_row0"):                          # output-channel sub-range: skip the packed weight rows before it
        d.w += sp["w_row0"] * sp["k"] * sp["k"] * sp["cin"] * 2
    d.OH, d.OW, d.gather_mode = sp["OH"], sp["OW"], sp["gather"]
    d.y, d.y_ld, d.y_coff, d.y_f32 = _p(y), y.ld, y.coff, y.f32
    d.out_mode, d.patch_k, d.patch_c = sp["out_mode"], sp["patch_k"], sp["patch_c"]
    d.bias, d.bias_bstride, d.act = _p(sp["bias"]), sp["bias_bstride"], sp["act"]
    res = sp["res"]
    d.res, d.res_ld, d.res_scale = _p(res), (res.ld if res is not None else 0), _p(sp["res_scale"])
    d.accumulate, d.stats = sp["accumulate"], _p(sp["stats"])
    if sp.get("stats") is not None and persistent_conv3(sp, plan.B):
        # GroupNorm sums of the persistent 3x3 kernel: per-(tile, wave) partial rows + a finalize launch (produced and consumed
        # inside one crd_conv_igemm call)
        scratch = plan.scratch("stats_scratch", plan.B * -(-sp["OW"] // 32) * -(-sp["OH"] // 16) * 8 * (sp["cout"] // 16) * 2)
        d.stats_partial, d.stats_partial_capacity = scratch.data_ptr(), scratch.numel()
    # (otherwise stats_partial stays NULL: workgroup-level sums go in with one atomic each.  The library's deterministic
    # partial-store + finalize path measured the same step time (34.6 vs 34.9 ms) and costs 261 more dispatches.)
    d.chan_sums = _p(sp.get("chan"))
    if sp.get("red") is not None:        # fused reduce phase of the GroupNorm backward this output feeds
        rx, rstats, rgamma, rbeta, rgmul, ract, rr = sp["red"]
        assert rx.coff == 0, "the fused reduce reads the GroupNorm input from channel 0"
        d.red_x, d.red_x_ld, d.red_gmul, d.red_act, d.red_x_f32 = _p(rx), rx.ld, rgmul, ract, rx.f32
        d.red_stats, d.red_gamma, d.red_beta, d.red_r = _p(rstats), _p(rgamma), _p(rbeta), _p(rr)
    return d


def _gn_in(plan, sp):
    n = L.GnInput()
    n.x_f32, n.gmul, n.act = sp["x_f32"], sp["gmul"], sp["act"]
    n.stats, n.gamma, n.beta = _p(sp["stats"]), _p(sp["gamma"]), _p(sp["beta"])
    n.xn, n.xn_ld = (_p(sp["xn"]), sp["xn"].ld) if sp["xn"] is not None else (None, 0)
    return n


def _gnb_in(plan, sp):
    n = L.GnBwdInput()
    gx = sp["gx"]
    n.gx, n.gx_f32, n.gx_ld, n.gmul, n.act = _p(gx), gx.f32, gx.ld, sp["gmul"], sp["act"]
    n.stats, n.gamma, n.beta, n.mask, n.r = _p(sp["stats"]), _p(sp["gamma"]), _p(sp["beta"]), _p(sp["mask"]), _p(sp["r"])
    n.dx, n.dx_ld = (_p(sp["dx"]), sp["dx"].ld) if sp["dx"] is not None else (None, 0)
    n.dgamma, n.dbeta = _p(sp["dgamma"]), _p(sp["dbeta"])
    return n


def _mlp(plan, sp):
    d = L.MlpDesc()
    for k, v in sp["ptrs"].items():
        setattr(d, k, _p(v))
    d.B, d.H, d.W, d.C, d.hidden = sp["dims"]
    return d


def _fp8_conv(plan, sp, w8, cout):
    """What the e4m3 forward and data-gradient launches share: 3x3, stride 1, e4m3 operands with their own row stride, bf16 output."""
    y = sp["y"]
    d = L.ConvDesc()
    d.x, d.x_ld, d.x_coff, d.B, d.IH, d.IW, d.Cin = sp["x8"].data_ptr(), sp["x8_ld"], 0, plan.B, sp["H"], sp["W"], sp["cin"]
    d.w, d.Cout, d.KH, d.KW, d.stride, d.pad, d.OH, d.OW = w8.data_ptr(), cout, 3, 3, 1, 1, sp["H"], sp["W"]
    d.y, d.y_ld, d.y_coff = _p(y), y.ld, y.coff
    return d


def _fp8_fwd(plan, sp):
    cw = sp["cw"]
    d = _fp8_conv(plan, sp, cw.w8, cw.cout)
    scratch = plan.scratch("stats_scratch", plan.B * -(-sp["W"] // 32) * -(-sp["H"] // 16) * 4 * (cw.cout // 16) * 2)
    d.stats, d.stats_partial, d.stats_partial_capacity = _p(sp["stats"]), scratch.data_ptr(), scratch.numel()
    return d


def _fp8_dgrad(plan, sp):
    d = _fp8_conv(plan, sp, sp["w8"], sp["cout"])
    d.gather_mode, d.accumulate = 1, sp["accumulate"]
    return d


def _wgrad(plan, sp, into=None):
    x, dy, cw = sp["x"], sp["dy"], sp["cw"]
    d = into if into is not None else L.WgradDesc()
    d.x, d.x_ld, d.x_coff, d.B, d.IH, d.IW, d.Cin = _p(x), x.ld, x.coff, plan.B, x.H, x.W, sp["cin"]
    d.dy, d.dy_ld, d.dy_coff, d.OH, d.OW, d.Cout = _p(dy), dy.ld, dy.coff, sp["OH"], sp["OW"], cw.cout
    d.KH, d.KW, d.stride, d.pad = sp["k"], sp["k"], sp["stride"], sp["pad"]
    d.dw, d.dbias = _p(cw.dw), _p(sp["dbias"])
    if cw.dw_parts is not None:
        d.dw_partials, d.dw_partial_capacity, d.wg_budget = cw.dw_parts.data_ptr(), cw.dw_S, cw.wg_budget
    return d


def _wgrad_group(plan, sp):
    """-> the two arguments of crd_conv_wgrad_grouped: the device table of the problems and their work items, and its info struct."""
    specs = sp["problems"]
    descs = (L.WgradDesc * len(specs))()
    for i, s in enumerate(specs):
        _wgrad(plan, s, into=descs[i])
    info = L.WgradGroupInfo()
    L.check(plan.lib.crd_wgrad_group_build(descs, len(specs), None, 0, C.byref(info)), "crd_wgrad_group_build")
    host = (C.c_uint8 * info.bytes)()
    L.check(plan.lib.crd_wgrad_group_build(descs, len(specs), host, info.bytes, C.byref(info)), "crd_wgrad_group_build")
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(plan.dev)
    plan.buffers.append(table)
    return table.data_ptr(), info


_BUILDERS = {"conv": _conv, "gn_in": _gn_in, "gnb_in": _gnb_in, "mlp": _mlp, "fp8": _fp8_fwd, "fp8d": _fp8_dgrad, "wg": _wgrad}


def make_desc(plan, sp):
    """Spec -> the op argument(s) it stands for (a list: the group is two).  The plan keeps the structs alive."""
    if sp["kind"] == "wg_group":
        table, info = _wgrad_group(plan, sp)
        plan.keep.append(info)
        return [table, C.byref(info)]
    d = _BUILDERS[sp["kind"]](plan, sp)
    plan.keep.append(d)
    return [C.byref(d)]
