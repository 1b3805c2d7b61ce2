"""Tables: what Plan._finalise lays out once every launch is recorded.

Owns the packed-weight arena and the pack table (fp32 parameters -> operand layouts), the destinations of the weight gradients
and the unpack table (accumulators -> flat gradient, one contiguous range per backward segment), the two zero arenas, and the
pass that puts the backward groups into execution order and decides which launch into a gradient region stores and which
accumulates.  Each function reads the lists the recording left on the plan and sets the attributes named in its docstring."""
import ctypes as C

import torch

from . import lib as L
from .plan_values import BF16, F32, SUM, rup

SEGMENTS = ["dec", "enc3", "enc2", "enc1", "enc0"]      # backward segments in execution order
DW_REPLICAS = 16      # accumulator copies of a depthwise weight gradient (spreads contended atomics)


def _struct_table(entries, dev):
    if not entries:
        return torch.zeros(8, dtype=torch.uint8, device=dev)
    raw = b"".join(bytes(e) for e in entries)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)


def _pack_entry(plan, name, dims, cmap=None, **dst):
    """dims: (Cout, Cin_ref, taps, Cin_pad, Cout_pad); dst: the destination fields of crd_pack_entry (tensors or ints)."""
    e = L.PackEntry()
    e.src = plan.p(name + ".weight").data_ptr()
    e.cmap = cmap.data_ptr() if cmap is not None else None
    e.Cout, e.Cin_ref, e.taps, e.Cin_pad, e.Cout_pad = dims
    for k, v in dst.items():
        setattr(e, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return e


def build_pack_table(plan):
    """-> w_arena, cw.w_fwd / w_dgrad / w_scatter / cmap_dev, pack_table, pack_stride, pack_offs, pack_elems, n_pack."""
    dev = plan.dev
    sizes = lambda cw: (cw.cout * cw.taps * cw.cin_pad, cw.cin_pad * cw.taps * cw.cout_pad)
    plan.w_arena = torch.zeros(sum(sizes(cw)[0] + (sizes(cw)[1] if cw.need_dgrad or cw.scatter else 0) for cw in plan.convs) + 8,
                               dtype=BF16, device=dev)
    off = 0

    def take(n):
        nonlocal off
        t = plan.w_arena[off:off + n]
        off += rup(n)
        return t
    entries = []                                   # (entry, elements of its largest destination)
    for cw in plan.convs:
        n_fwd, n_bwd = sizes(cw)
        cw.w_fwd = take(n_fwd)
        if cw.need_dgrad and not cw.scatter:
            cw.w_dgrad = take(n_bwd)
        if cw.scatter:
            cw.w_scatter = take(n_bwd)
        if cw.cmap is not None:
            cw.cmap_dev = torch.tensor(cw.cmap, dtype=torch.int32, device=dev)
        dst = {k: t for k, t in (("dst_fwd", cw.w_fwd), ("dst_dgrad", cw.w_dgrad), ("dst_scatter", cw.w_scatter)) if t is not None}
        entries.append((_pack_entry(plan, cw.name, cw.dims, cw.cmap_dev, **dst), max(n_fwd, n_bwd)))
    for (cw, Wt, ld, coff, row0, rows) in plan.kcat_entries:    # this layer's columns / row range of a K-concatenated data-gradient matrix
        entries.append((_pack_entry(plan, cw.name, cw.dims, cw.cmap_dev, dst_dgrad=Wt, dgrad_ld=ld, dgrad_coff=coff, dgrad_row0=row0,
                                    dgrad_rows=rows), cw.cin_pad * cw.taps * cw.cout_pad))
    for (name, hid, w9, fmt) in plan.dw_entries:          # fmt: crd_pack_entry.dst_f32 (2: fp32 holding bf16-rounded values, 0: bf16)
        entries.append((_pack_entry(plan, name, (1, hid, 9, hid, 8), dst_fwd=w9, dst_f32=fmt), 9 * hid))
    # Sorted by the parameter's position in the model's flat buffer, so that the entries of a gradient bucket (a contiguous
    # range of that buffer, trainer.GradSync) are a contiguous range of the table: pack(lo, hi) re-packs one bucket right
    # behind its optimizer slice instead of everything at the head of the next step's forward (169 us on the critical path).
    base = plan.model.flat.data_ptr()
    entries.sort(key=lambda en: en[0].src)
    plan.pack_offs = [(e.src - base) // 4 for e, _ in entries]
    plan.pack_elems = [n for _, n in entries]
    plan.pack_table = _struct_table([e for e, _ in entries], dev)
    plan.pack_stride = C.sizeof(L.PackEntry)
    plan.n_pack = len(entries)


def stream3_splits(lib, B, ih, iw, cin, cout, k=3, stride=1, pad=1, wg_budget=0):
    """crd_conv_wgrad_splits of a same-size k x k layer: the row splits of the streaming 3x3 weight-gradient kernel, 0 where
    crd_conv_wgrad sends the layer to the generic kernel.  The routing rule lives in the library (csrc/wgrad.hip: uses_stream3) and is
    asked, not repeated: the query reads no pointer."""
    probe = L.WgradDesc()
    probe.B, probe.IH, probe.IW, probe.OH, probe.OW = B, ih, iw, (ih + 2 * pad - k) // stride + 1, (iw + 2 * pad - k) // stride + 1
    probe.Cin, probe.Cout, probe.KH, probe.KW, probe.stride, probe.pad = cin, cout, k, k, stride, pad
    probe.wg_budget = wg_budget
    return int(lib.crd_conv_wgrad_splits(C.byref(probe)))


def place_weight_gradients(plan):
    """-> cw.dw (+ dw_parts, dw_S, wg_budget) of every trainable convolution; returns those convolutions.
    Destination: a crd_sum_t scratch block (order-independent integer atomics) that the segment's unpack converts.  The streaming
    3x3 kernel splits the pixels S ways; each split stores its block into its own copy (no atomics, nothing to zero) and the
    unpack kernel sums the copies."""
    out = []
    for cw in plan.convs:
        if cw.frozen:                  # no weight-gradient launch was recorded: nothing to accumulate or un-pack
            continue
        if cw.stream3_geom is not None:
            ih, iw, cin = cw.stream3_geom
            cw.wg_budget = int(getattr(plan.model, "w3_total_wgs", None) or 0)      # set by TrainStep in late-wgrad mode
            cw.dw_S = stream3_splits(plan.lib, plan.B, ih, iw, cin, cw.cout, wg_budget=cw.wg_budget)
        if cw.dw_S > 0:
            cw.dw = cw.dw_parts = plan.new((cw.dw_S, cw.cout, cw.taps, cw.cin_pad), F32)
        else:
            cw.dw = plan.zb(cw.cout, cw.taps, cw.cin_pad)
        out.append(cw)
    return out


def build_zero_arenas(plan):
    """-> zf_arena, zb_arena; every _Lazy handed out by Plan.zf / Plan.zb becomes a view of its arena."""
    def materialise(views):
        arena = torch.zeros(max(sum(v.numel for v in views), 1), dtype=SUM, device=plan.dev)
        off = 0
        for v in views:
            v.t = arena[off:off + v.numel].view(v.shape)
            off += v.numel
        return arena
    plan.zf_arena = materialise(plan._zf_views)
    plan.zb_arena = materialise(plan._zb_views)


def _unpack_entry(src, dst, dims, cmap=None, replicas=0, replica_stride=0, src_sum=1):
    """dims: (Cout, Cin_ref, taps, Cin_pad).  src_sum 1: crd_sum_t accumulators; 0: fp32 partial copies, added in index order."""
    u = L.UnpackEntry()
    u.src, u.dst, u.cmap = src, dst.data_ptr(), cmap.data_ptr() if cmap is not None else None
    u.Cout, u.Cin_ref, u.taps, u.Cin_pad = dims
    u.replicas, u.replica_stride, u.src_sum = replicas, replica_stride, src_sum
    return u


def build_unpack_table(plan, convs):
    """-> unpack_table, unpack_stride, unpack_ranges {segment: (first entry, one past last, largest entry)}, n_unpack, max_unpack.
    (needs the zero arenas)"""
    items = []                                          # (segment index, entry, elements)
    for cw in convs:
        nel = cw.cout * cw.taps * cw.cin_pad
        parts = dict(src=cw.dw_parts.data_ptr(), replicas=cw.dw_S, replica_stride=nel, src_sum=0) if cw.dw_parts is not None \
            else dict(src=cw.dw.t.data_ptr())
        items.append((cw.tag, _unpack_entry(dst=plan.g(cw.name + ".weight"), dims=cw.dims[:4], cmap=cw.cmap_dev, **parts), nel))
    for name, hid, dw10, tag in plan.dw_grads:          # depthwise [copy][9 taps + bias][channel]: one entry for the taps, one for the bias row
        for which, taps, row in (("weight", 9, 0), ("bias", 1, 9)):
            items.append((tag, _unpack_entry(dw10.t.data_ptr() + row * hid * 8, plan.g(name + "." + which), (1, hid, taps, hid),
                                             replicas=DW_REPLICAS, replica_stride=10 * hid), taps * hid))
    for name, Cn, rows, R, tag, off, stride in plan.row_grads:      # R rows of a vector gradient
        items.append((tag, _unpack_entry(rows.t.data_ptr() + 8 * off, plan.g(name), (1, Cn, 1, Cn), replicas=R, replica_stride=stride), Cn))
    items.sort(key=lambda it: SEGMENTS.index(it[0]))
    plan.unpack_ranges = {}
    for i, (tag, _, nel) in enumerate(items):
        lo, _, mx = plan.unpack_ranges.get(tag, (i, i, 1))
        plan.unpack_ranges[tag] = (lo, i + 1, max(mx, nel))
    plan.unpack_table = _struct_table([u for _, u, _ in items], plan.dev)
    plan.unpack_stride = C.sizeof(L.UnpackEntry)
    plan.n_unpack, plan.max_unpack = len(items), max([1] + [nel for _, _, nel in items])


def order_backward(plan):
    """-> bwd, bwd_segments [(tag, first op, one past last)]: the groups in reverse order of recording; and the accumulate flag of every
    op with a gradient region: the first launch into a column range stores, later ones accumulate."""
    written = {}
    plan.bwd, plan.bwd_segments = [], []
    for grp, tag in zip(reversed(plan.bwd_groups), reversed(plan.bwd_tags)):
        if plan.bwd_segments and plan.bwd_segments[-1][0] == tag:
            plan.bwd_segments[-1][2] = len(plan.bwd) + len(grp)
        else:
            plan.bwd_segments.append([tag, len(plan.bwd), len(plan.bwd) + len(grp)])
        for op in grp:
            if op.region is not None:
                key, c0, c1 = op.region[:-2], op.region[-2], op.region[-1]
                prev = written.setdefault(key, [])
                overlap = [r for r in prev if r[0] < c1 and c0 < r[1]]
                if overlap:
                    lo, hi = min(r[0] for r in overlap), max(r[1] for r in overlap)
                    assert lo <= c0 and hi >= c1, f"partial gradient overlap at {op.name} {op.region}: {overlap}"
                else:
                    prev.append((c0, c1))
                if isinstance(op.acc_slot, tuple):
                    op.acc_slot[1]["accumulate"] = int(bool(overlap))
                elif op.acc_slot is not None:
                    op.args[op.acc_slot] = int(bool(overlap))
            plan.bwd.append(op)
