"""Autograd-aware operators over libstag_hip.so.

`aggregate` is the hot path: one call = noise draw + relu + in-norm + degree
scaling + `update_all(u_mul_e, sum|mean)` of the reference (stag/layers.py:84-113,
stag/zoo/gcn.py:67-108), as one fused HIP pass.  Its backward walks the
source-major CSR and REDRAWS the forward's noise from the Philox counters
(`csr_t.nidx`), so no [E, D] tensor is saved for autograd.
"""
import ctypes as C

import torch

from . import _lib, _torch_ext
from .graph import DEFAULT_SEG_LEN, Graph
from .noise import EdgeNoise
from .random import _MASK64

_REDUCE = {"sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN}


def _owner(graph):
    """The graph object that owns the cached structure.  Autograd contexts keep THIS, never a
    `local_var()` copy: a copy's frames hold the step's tensors, whose grad_fn holds the context
    — a cycle through the autograd graph that kept an [E, D] tensor alive per training step."""
    return graph._cache_owner() if hasattr(graph, "_cache_owner") else graph


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    t = t.contiguous()
    if t.dim() == 2 and t.stride(0) >= _MAX_ROW_STRIDE:
        # one row is contiguous whatever stride its view carries; the library takes 32 bits of bytes (STAG_ENOSYS past them)
        t = t.clone(memory_format=torch.contiguous_format)
    return t


_MAX_ROW_STRIDE = 1 << 30      # floats: the aggregation entry points refuse a row stride of 2^32 bytes or more


# A noise description travels to the library in one of two forms: the ctypes `stag_noise_spec`, or — when
# the TORCH_LIBRARY front end is loaded (_torch_ext) — the argument tuple of torch.ops.stag.* (ints, 64-bit
# patterns, floats, the parameter tensors themselves).  _agg_raw / _agg_bwd_raw take either.
def _none_spec():
    if _torch_ext.available():
        return _NONE_ARGS
    s = _lib.NoiseSpec()
    s.kind = _lib.NOISE_NONE
    return s


def _explicit_spec(w, relu=False, in_norm=False, group=0):
    if _torch_ext.available():
        return ([_lib.NOISE_EXPLICIT, 0, int(relu), int(in_norm), 0, int(group), 0, 0], [0, 0, 0], [0.0, 0.0], w, None, None)
    s = _lib.NoiseSpec()
    s.kind = _lib.NOISE_EXPLICIT
    s.p0 = w.data_ptr()
    s.relu, s.in_norm, s.group = int(relu), int(in_norm), int(group)
    return s


def _noise_spec(noise, in_norm=None):
    """The spec of an EdgeNoise (in_norm optionally overridden: the backward passes redraw the raw weights)."""
    if _torch_ext.available():
        return noise.torch_args(in_norm=in_norm)
    s = noise.spec()
    if in_norm is not None:
        s.in_norm = int(in_norm)
    return s


def _targs_or_c(spec):
    """The ctypes form, whichever form came in (entry points bound through ctypes only)."""
    return _targs_to_ctypes(spec) if isinstance(spec, tuple) else spec


def _spec_in_norm(spec):
    return bool(spec[0][3]) if isinstance(spec, tuple) else bool(spec.in_norm)


_COMBINE_GROUP = 16     # kCombineGroup (csrc/agg_kernel.hpp): partials per group of a long row's combine


def _counter_count(n_long, n_seg, tiles):
    """ints of stag_plan.seg_counters: a row counter per (channel tile, long row), then — once a row can have more
    than one group of segments — a group counter per (channel tile, segment index), taken by a group's first segment."""
    return max(n_long, 1) * tiles + (n_seg * tiles if n_seg > _COMBINE_GROUP else 0)


def _plan_counters(plan_t, tiles, dev):
    """The plan's arrival counters: one set per (channel tiles, stream) — two launches that may be in flight together
    (different streams) must not share them; zeroed once, every completed launch leaves them zero again."""
    key = (tiles, _lib.stream_of(dev))
    counters = plan_t["counters"].get(key)
    if counters is None:
        counters = torch.zeros(_counter_count(plan_t["n_long"], plan_t["n_seg"], tiles), dtype=torch.int32, device=dev)
        plan_t["counters"][key] = counters
    return key, counters


def _plan_struct(csrv, seg_len, tiles, nbytes, dev, plan_t=None, width=None, gat_width=None, drawn=False, share=0):
    """ctypes stag_plan for csrv (None when planning is off), plus the tensors it points into.
    plan_t: a sub-plan of csrv (CsrView.subplan) instead of its whole plan.  width: the row width of an aggregation
    launch — it may walk the plan's XCD-aware order (stag_plan.xcd_order).  gat_width: H * F of a cooperative GAT
    launch — its unit batches may be the XCD-aware ones (stag_plan_blocks_xcd).  share: the row width (in fp32 lanes' worth of channels) of a
    launch that walks whole-row units in any order and adds nothing across them — it takes the plan's share order
    (CsrView.share_units) in place of its unit records where the view has one for this width.  The other entry points use none of these."""
    if plan_t is None:
        plan_t = csrv.plan(seg_len)
    if plan_t is None:
        return None, None
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
    key, counters = _plan_counters(plan_t, tiles, dev)
    order, strides, fine = csrv.xcd_order(plan_t, width, drawn) if width and plan_t.get("xcd_on") else (None, (0, 0), 0)
    units, block_ptr, n_blocks, n_heavy = plan_t["units"], plan_t["block_ptr"], plan_t["n_blocks"], plan_t["n_heavy"]
    if gat_width and plan_t.get("xcd_on"):
        blocks = csrv.gat_blocks(plan_t, gat_width)
        if blocks is not None:
            units, block_ptr, n_blocks, fine, n_heavy = blocks[0], blocks[1], blocks[2], -blocks[3], 0
            order = units       # (non-NULL xcd_order: "these batches are XCD-local" — the GAT forward keeps two rows in flight)
    shared = csrv.share_units(plan_t, share) if share else None
    if shared is not None:
        units, fine = shared, "share"      # (the same records, the same counts: only the struct's units pointer differs)
    # the struct is kept per (tiles, stream, order): only the workspace changes from call to call (host time of a
    # call matters on launch-bound graphs).  Safe to reuse: the library reads it during the call only.
    plan_c = plan_t.setdefault("_structs", {}).get(key + (fine,))
    if plan_c is None:
        plan_c = _lib.Plan(plan_t["seg_len"], plan_t["n_units"], plan_t["n_long"], plan_t["n_seg"],
                           _lib.ptr(units), _lib.ptr(plan_t["long_rows"]),
                           _lib.ptr(plan_t["long_seg_ptr"]), _lib.ptr(counters), None, 0,
                           n_heavy, n_blocks, _lib.ptr(block_ptr),
                           _lib.ptr(order), *strides)
        plan_t["_structs"][key + (fine,)] = plan_c
    plan_c.workspace, plan_c.workspace_bytes = _lib.ptr(ws), nbytes
    return plan_c, (ws, counters)


def _share_width(spec, D):
    """The `share` argument of _plan_struct / _plan_args for a launch of this spec (either form): D, or 0 for the launch of
    a shard (a node-range shard draws from pos_base, a channel shard from chunk_base), which keeps plan order."""
    shard = (spec[1][2] or spec[0][6]) if isinstance(spec, tuple) else (spec.pos_base or spec.chunk_base)
    return 0 if shard else D


_NONE_ARGS = ([_lib.NOISE_NONE, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0], [0.0, 0.0], None, None, None)


def _plan_args(csrv, plan_t, tiles, dev, width=None, drawn=False, share=0):
    """(units, long_rows, long_seg_ptr, block_ptr, xcd, counters, plan_ints) of torch.ops.stag.*
    (width, drawn, share: as for _plan_struct)"""
    if plan_t is None:
        return (None, None, None, None, None, None, [0, 0, 0, 0, 0, 0, 0, 0])
    _, counters = _plan_counters(plan_t, tiles, dev)
    order, strides, _ = csrv.xcd_order(plan_t, width, drawn) if width and plan_t.get("xcd_on") else (None, (0, 0), 0)
    ints = [plan_t["seg_len"], plan_t["n_units"], plan_t["n_long"], plan_t["n_seg"], plan_t["n_heavy"], plan_t["n_blocks"],
            *strides]
    shared = csrv.share_units(plan_t, share) if share else None
    return (plan_t["units"] if shared is None else shared, plan_t["long_rows"], plan_t["long_seg_ptr"], plan_t["block_ptr"],
            order, counters, ints)


def _agg_fwd_torch(csrv, x, noise_args, reduce, src_scale, dst_scale, seg_len, want_norm_scale, broadcast_x):
    """stag_agg_fwd through the dispatcher op (csrc/torch_ext.cpp): same library call, no ctypes."""
    dev = _lib.require_device(x, csrv.indptr, src_scale, dst_scale)
    D = x.numel() if broadcast_x else x.shape[1]
    plan_t = csrv.plan(seg_len)
    out, ns = torch.ops.stag.agg_fwd(*csrv.torch_args(), *_plan_args(csrv, plan_t, (D + 255) // 256, dev, width=D,
                                                                     drawn=noise_args[0][0] >= _lib.NOISE_NORMAL,
                                                                     share=_share_width(noise_args, D)), x,
                                     broadcast_x, *noise_args, reduce, src_scale, dst_scale, want_norm_scale)
    return out, (ns if want_norm_scale else None)


def _agg_raw(csrv, x, D, spec, reduce, src_scale, dst_scale, seg_len, want_norm_scale=False,
             broadcast_x=False, out=None, plan_t=None, ns_out=None):
    """One stag_agg_fwd launch on csrv (a CsrView). x: [n_src, D] fp32 contiguous.
    out / plan_t: write the rows of a sub-plan's units into an existing [n_dst, D] tensor (ns_out: and their
    in-norm factors into an existing one)."""
    if isinstance(spec, tuple):
        if out is None and plan_t is None:
            return _agg_fwd_torch(csrv, x, spec, reduce, src_scale, dst_scale, seg_len, want_norm_scale, broadcast_x)
        spec = _targs_to_ctypes(spec)
    dev = _lib.require_device(x, csrv.indptr, src_scale, dst_scale)
    if out is None:
        out = torch.empty((csrv.n_dst, D), dtype=torch.float32, device=dev)
    ns = ns_out if ns_out is not None else (
        torch.empty((csrv.n_dst, D), dtype=torch.float32, device=dev) if want_norm_scale else None)
    if csrv.n_dst == 0:          # no row: nothing to launch (a node-range shard whose cut left it without rows)
        return out, ns
    if plan_t is None:
        plan_t = csrv.plan(seg_len)
    nbytes = (_lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], D, int(spec.in_norm))
              if plan_t is not None else 0)
    plan_c, _keep = _plan_struct(csrv, seg_len, (D + 255) // 256, nbytes, dev, plan_t, width=D,
                                 drawn=spec.kind >= _lib.NOISE_NORMAL, share=_share_width(spec, D))
    # (spec is the ctypes form from here on)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_fwd(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x),
            0 if broadcast_x else x.stride(0), D, C.byref(spec), reduce, _lib.ptr(src_scale),
            _lib.ptr(dst_scale), _lib.ptr(out), D, _lib.ptr(ns), _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_fwd")
    return out, ns


_HALF_DTYPES = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def _unit_sum_raw(entry, csrv, x, x_args, D, spec, reduce, src_scale, dst_scale, seg_len, plan_t):
    """One launch of a plan-order sum entry point (stag_agg_fwd_half | stag_agg_fwd_w1) on csrv: out [n_dst, D] fp32.
    x_args(): what the entry point takes between x and D.  Bound through ctypes only; the plan is walked in plan order, or in the view's share order."""
    spec = _targs_or_c(spec)
    dev = _lib.require_device(x, csrv.indptr, src_scale, dst_scale)
    out = torch.empty((csrv.n_dst, D), dtype=torch.float32, device=dev)
    if csrv.n_dst == 0:
        return out
    if plan_t is None:
        plan_t = csrv.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], D, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv, seg_len, (D + 255) // 256, nbytes, dev, plan_t, width=None,
                                 share=max(D // 2, 1) if entry == "stag_agg_fwd_half" else D)      # (a lane owns 8 halves)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = getattr(_lib.lib(), entry)(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x), *x_args(), D, C.byref(spec),
            reduce, _lib.ptr(src_scale), _lib.ptr(dst_scale), _lib.ptr(out), D, _lib.stream_of(dev))
    _lib.check(rc, entry)
    return out


def _agg_half_raw(csrv, x, D, spec, reduce, src_scale, dst_scale, seg_len, plan_t=None):
    """stag_agg_fwd_half: x [n_src, D] fp16 | bf16 as it is (unit column stride, any row stride the entry point takes)."""
    return _unit_sum_raw("stag_agg_fwd_half", csrv, x, lambda: (_HALF_DTYPES[x.dtype], x.stride(0)), D, spec, reduce,
                         src_scale, dst_scale, seg_len, plan_t)


def _agg_w1_raw(csrv, x, D, spec, reduce, src_scale, dst_scale, seg_len, plan_t=None):
    """stag_agg_fwd_w1: x [n_src, D] fp32 (unit column stride), spec of width 1 — an EdgeNoise's with dn = 1, or EXPLICIT
    with p0 = w[E].  On csr_t (nidx = forward positions) the same weights are redrawn: how the backward forms dx."""
    return _unit_sum_raw("stag_agg_fwd_w1", csrv, x, lambda: (x.stride(0),), D, spec, reduce, src_scale, dst_scale, seg_len,
                         plan_t)


def _targs_to_ctypes(t):
    """The torch-op argument tuple as a ctypes stag_noise_spec (for the entry points bound through ctypes)."""
    ni, nu, nf, p0, p1, epoch = t
    s = _lib.NoiseSpec()
    s.kind, s.param_mode, s.relu, s.in_norm, s.deriv, s.group, s.chunk_base, s.p1_log = ni
    s.seed, s.offset, s.pos_base = nu[0] & ((1 << 64) - 1), nu[1] & ((1 << 64) - 1), nu[2]
    s.p0_scalar, s.p1_scalar = nf
    s.p0, s.p1, s.epoch = _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(epoch)
    return s


def _agg_bwd_raw(csrv_t, g, D, spec, g_scale, row_scale, seg_len, want_dp):
    """One stag_agg_bwd launch on the source-major CSR: dx and, if want_dp, the two per-row
    parameter-derivative aggregates (same gather, same Philox block)."""
    if isinstance(spec, tuple):
        dev = _lib.require_device(g, csrv_t.indptr, g_scale, row_scale)
        plan_t = csrv_t.plan(seg_len)
        dx, t0, t1 = torch.ops.stag.agg_bwd(*csrv_t.torch_args(), *_plan_args(csrv_t, plan_t, (D + 255) // 256, dev, width=D,
                                                                               drawn=spec[0][0] >= _lib.NOISE_NORMAL,
                                                                               share=_share_width(spec, D)),
                                            g, *spec, g_scale, row_scale, want_dp)
        return dx, (t0 if want_dp else None), (t1 if want_dp else None)
    dev = _lib.require_device(g, csrv_t.indptr, g_scale, row_scale)
    dx = torch.empty((csrv_t.n_dst, D), dtype=torch.float32, device=dev)
    t0 = torch.empty_like(dx) if want_dp else None
    t1 = torch.empty_like(dx) if want_dp else None
    plan_t = csrv_t.plan(seg_len)
    nbytes = (_lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], (3 if want_dp else 1) * D, 0)
              if plan_t is not None else 0)
    plan_c, _keep = _plan_struct(csrv_t, seg_len, (D + 255) // 256, nbytes, dev, plan_t=plan_t, width=D,
                                 drawn=spec.kind >= _lib.NOISE_NORMAL, share=_share_width(spec, D))
    cs = csrv_t.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_bwd(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(g), g.stride(0), D,
            C.byref(spec), _lib.ptr(g_scale), _lib.ptr(row_scale), _lib.ptr(dx), _lib.ptr(t0),
            _lib.ptr(t1), D, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd")
    return dx, t0, t1


def _agg_bwd_edge_raw(csrv_t, g, x, D, spec, g_scale, row_scale, seg_len, want_dx=True):
    """One stag_agg_bwd_edge launch on the source-major CSR: dx (if wanted) and the gradients of the
    [E, 1] parameter pair of every edge, by edge id.  None when the shape has no one-pass form
    (D > 256: the caller takes stag_agg_bwd + stag_agg_bwd_w)."""
    if D > 256:
        return None
    dev = _lib.require_device(g, x, csrv_t.indptr, g_scale, row_scale)
    dx = torch.empty((csrv_t.n_dst, D), dtype=torch.float32, device=dev) if want_dx else None
    e0 = torch.empty((csrv_t.n_edges, 1), dtype=torch.float32, device=dev)
    e1 = torch.empty_like(e0)
    plan_t = csrv_t.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], D, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv_t, seg_len, 1, nbytes, dev, plan_t=plan_t, width=D, drawn=True, share=D)
    cs = csrv_t.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_bwd_edge(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(g), g.stride(0), D,
            C.byref(spec), _lib.ptr(g_scale), _lib.ptr(row_scale), _lib.ptr(x), x.stride(0),
            _lib.ptr(dx), D, _lib.ptr(e0), _lib.ptr(e1), _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd_edge")
    return dx, e0, e1


def _agg_bwd_pedge_raw(csrv_t, g, x, D, spec, g_scale, row_scale, seg_len, want_dx=True, want_p1=True):
    """One stag_agg_bwd_pedge launch on the source-major CSR: dx (if wanted) and the gradients of the [E, D] parameter
    tables, by edge id (the second only if wanted).  Bound through ctypes only; the plan is walked in plan order."""
    dev = _lib.require_device(g, x, csrv_t.indptr, g_scale, row_scale)
    dx = torch.empty((csrv_t.n_dst, D), dtype=torch.float32, device=dev) if want_dx else None
    e0 = torch.empty((csrv_t.n_edges, D), dtype=torch.float32, device=dev)
    e1 = torch.empty_like(e0) if want_p1 else None
    if csrv_t.n_edges == 0 or csrv_t.n_dst == 0:        # (an empty table has no address to hand over)
        return (dx.zero_() if want_dx else None), e0, e1
    plan_t = csrv_t.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], D, 0) if plan_t is not None and want_dx else 0
    plan_c, _keep = _plan_struct(csrv_t, seg_len, (D + 255) // 256, nbytes, dev, plan_t=plan_t)
    cs = csrv_t.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_bwd_pedge(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(g), g.stride(0), D,
            C.byref(spec), _lib.ptr(g_scale), _lib.ptr(row_scale), _lib.ptr(x), x.stride(0),
            _lib.ptr(dx), D, _lib.ptr(e0), _lib.ptr(e1), D, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd_pedge")
    return dx, e0, e1


def _agg_bwd_dp_raw(csrv_t, g, x, D, spec, g_scale, row_scale, seg_len, want_dx=True):
    """One stag_agg_bwd_dp launch on the source-major CSR: dx (if wanted) and the FINISHED gradients of scalar /
    per-channel parameters, dp0 [D], dp1 [D] (x = None: ones in its place)."""
    dev = _lib.require_device(g, x, csrv_t.indptr, g_scale, row_scale)
    if isinstance(spec, tuple):     # the dispatcher op (csrc/torch_ext.cpp)
        plan_t = csrv_t.plan(seg_len)
        dx, dp0, dp1 = torch.ops.stag.agg_bwd_dp(*csrv_t.torch_args(), *_plan_args(csrv_t, plan_t, (D + 255) // 256, dev),
                                                 g, x, *spec, g_scale, row_scale, bool(want_dx))
        return (dx if want_dx else None), dp0, dp1
    dx = torch.empty((csrv_t.n_dst, D), dtype=torch.float32, device=dev) if want_dx else None
    dp0 = torch.empty(D, dtype=torch.float32, device=dev)
    dp1 = torch.empty(D, dtype=torch.float32, device=dev)
    plan_t = csrv_t.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], D, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv_t, seg_len, (D + 255) // 256, nbytes, dev, plan_t=plan_t, width=D)
    n_units = plan_t["n_units"] if plan_t is not None else csrv_t.n_dst
    wbytes = _lib.lib().stag_agg_bwd_dp_workspace_bytes(n_units, D)
    ws = torch.empty(max(wbytes // 4, 1), dtype=torch.float32, device=dev)
    cs = csrv_t.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_bwd_dp(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(g), g.stride(0), D,
            C.byref(spec), _lib.ptr(g_scale), _lib.ptr(row_scale), _lib.ptr(x), x.stride(0) if x is not None else 0,
            _lib.ptr(dx), D, _lib.ptr(dp0), _lib.ptr(dp1), _lib.ptr(ws), wbytes, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd_dp")
    return dx, dp0, dp1


_AGG_BWD_DP_ONE_PASS = True     # stag_agg_bwd_dp | stag_agg_bwd + stag_coldot (A/B, and the torch-op argument form)


def coldot(x, t0, t1=None):
    """out_i[k] = sum_n x[n,k] * t_i[n,k]  (stag_coldot; no autograd — a backward-pass helper)."""
    dev = _lib.require_device(x, t0, t1)
    x, t0, t1 = _f32c(x), _f32c(t0), _f32c(t1)
    n, D = x.shape
    if n == 0:          # empty tensors have no device pointer to hand over
        z = torch.zeros(D, dtype=torch.float32, device=dev)
        return z, (z.clone() if t1 is not None else None)
    nbytes = _lib.lib().stag_coldot_workspace_bytes(D)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    o0 = torch.empty(D, dtype=torch.float32, device=dev)
    o1 = torch.empty(D, dtype=torch.float32, device=dev) if t1 is not None else None
    with _lib.on_device(dev):
        rc = _lib.lib().stag_coldot(_lib.ptr(x), x.stride(0), _lib.ptr(t0), _lib.ptr(t1), t0.stride(0), n, D,
                                    _lib.ptr(o0), _lib.ptr(o1), _lib.ptr(ws), nbytes, _lib.stream_of(dev))
    _lib.check(rc, "stag_coldot")
    return o0, o1


_COLSUM_OFFSETS = {}


def column_sum(g):
    """sum over the rows of g [N, D] — a bias gradient.  torch's reduction takes a slow path when D is not a multiple
    of 4 (575 us for [56,944, 121] on MI355X against 13 us for [56,944, 256]); those widths go through the readout
    kernel over 512 row chunks and a sum of the 512 partial rows (fixed order)."""
    n, D = g.shape
    if not g.is_cuda or D % 4 == 0 or n < 8192:
        return g.sum(0)
    g = _f32c(g)
    key = (n, g.device)
    offs = _COLSUM_OFFSETS.get(key)
    if offs is None:
        step = (n + 511) // 512
        offs = torch.clamp(torch.arange(513, dtype=torch.int64) * step, max=n).to(torch.int32).to(g.device)
        if len(_COLSUM_OFFSETS) > 64:
            _COLSUM_OFFSETS.clear()
        _COLSUM_OFFSETS[key] = offs
    return _segment_reduce_raw(g, offs, _lib.REDUCE_SUM, g.device).sum(0)


class _BiasAdd(torch.autograd.Function):
    """x + bias with the bias gradient by column_sum (autograd's own reduction for a broadcast add is the slow one)."""

    @staticmethod
    def forward(ctx, x, bias):
        return x + bias

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.needs_input_grad[0] else None), (column_sum(g).reshape(-1) if ctx.needs_input_grad[1] else None)


def add_bias(x, bias):
    """x [N, D] + bias [D]; the bias gradient avoids torch's slow column reduction for D % 4 != 0."""
    if x.dim() != 2 or not x.is_cuda or bias.dim() != 1 or x.shape[1] % 4 == 0:
        return x + bias
    return _BiasAdd.apply(x, bias)


class _NodeLinear(torch.autograd.Function):
    """y = x @ w for a tall x [N, in] (the dense transform after an aggregation,
    stag/zoo/gcn.py:97-98).  Forward and dx are plain rocBLAS/hipBLASLt GEMMs; the weight gradient
    x^T g is a K = N reduction that the library runs as ONE tile column (403 us at N = 169,343,
    128 x 128, MI355X) — here it is split over K into a batched GEMM + sum (67 us)."""

    SPLIT = 64

    # Under torch.autocast the products below would come out half-typed and hand the backward a half-typed gradient
    # for fp32 saved operands (a dtype error in its GEMMs): the transform behind an aggregation stays fp32 — the
    # aggregated rows are fp32 whatever the gathered rows were (stag_agg_fwd_half).  Outside autocast: no effect.
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, bias=None, add=None):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.has_add = add is not None
        # the bias — or a whole addend [rows, out]: GraphSAGE's other branch — rides in the GEMM's epilogue (one
        # pass over the result instead of two)
        if add is not None:
            return torch.addmm(add if bias is None else add + bias, x, w)
        return torch.addmm(bias, x, w) if bias is not None else x @ w

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        # g @ w^T as an NN product on a transposed copy of w (64 KB): 75 against 92 us for the NT form at
        # N = 169,343, 128 x 128 (tools/gemm_probe.py)
        # (and when the output is wider than the input — GAT's fc, 128 -> 8 x 32 — the NT form on a contiguous w
        # wins instead: 119 against 158 us; the library's kernel choice is what differs)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = (torch.nn.functional.linear(g, w.contiguous()) if g.shape[1] > w.shape[0]
                  else g @ w.t().contiguous())
        db = column_sum(g) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        dw = None
        if ctx.needs_input_grad[1]:
            n, S = x.shape[0], _NodeLinear.SPLIT
            n1 = (n // S) * S
            if n1 >= 64 * S:
                g = g.contiguous()
                dw = torch.bmm(x[:n1].view(S, n1 // S, x.shape[1]).transpose(1, 2),
                               g[:n1].view(S, n1 // S, g.shape[1])).sum(0)
                if n1 < n:
                    dw = dw + x[n1:].t() @ g[n1:]
            else:
                dw = x.t() @ g
        return dx, dw, db, (g if (ctx.has_add and ctx.needs_input_grad[3]) else None)


def node_linear(x, w, bias=None, add=None):
    """x [N, in] @ w [in, out] (+ bias, + add [N, out], both in the GEMM's epilogue) with a split-K weight gradient
    (see _NodeLinear)."""
    if x.dim() == 3 and x.is_contiguous() and add is None:
        # [S, N, in]: the Monte-Carlo samples of one layer (aggregate_mc) — ONE product over S*N rows, so the weight
        # gradient keeps its split-K form instead of a K = S*N single-tile-column reduction
        S, n = x.shape[0], x.shape[1]
        return _NodeLinear.apply(x.view(S * n, x.shape[2]), w, bias).view(S, n, w.shape[1])
    if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        y = x @ w if bias is None else x @ w + bias
        return y if add is None else y + add
    # (rows may be strided — the [:, :D] view of a padded aggregation result: the GEMMs take the leading dimension,
    # the split-K weight gradient views the rows in groups, neither needs a packed copy)
    if add is not None and (add.shape != (x.shape[0], w.shape[1]) or add.dtype != x.dtype):
        return _NodeLinear.apply(x, w, bias) + add
    return _NodeLinear.apply(x, w, bias, add)


class _GatherRows(torch.autograd.Function):
    """x[src] or x[dst] as an [E, D] tensor by edge id.  Forward is an index_select; the backward —
    a scatter-add of E rows into N — is the aggregation kernel with the incoming gradient as
    explicit edge weights over one broadcast row of ones (torch's index backward takes 3.9 ms
    for [1.17M, 128] on MI355X, this 0.2 ms)."""

    @staticmethod
    def forward(ctx, x, graph, which):
        if getattr(graph, "is_shard", False):     # sources are buffer rows, destinations this rank's rows
            src, dst = graph.edge_endpoints()
            if which == "dst":
                dst = dst - graph.loc_off
        else:
            src, dst = graph.edges()
        ctx.graph, ctx.which = _owner(graph), which
        return x.index_select(0, (src if which == "src" else dst).long())

    @staticmethod
    def backward(ctx, g):
        graph = ctx.graph
        g = _f32c(g)
        csrv = graph.csr_t if ctx.which == "src" else graph.csr
        D = g.shape[1]
        ones = torch.ones(D, dtype=torch.float32, device=g.device)
        out, _ = _agg_raw(csrv, ones, D, _explicit_spec(g), _lib.REDUCE_SUM, None, None, DEFAULT_SEG_LEN,
                          broadcast_x=True)
        return out, None, None


def gather_rows(graph, x, which):
    """x[u] (which="src") or x[v] (which="dst") for every edge u -> v, rows by edge id."""
    if (x.dim() != 2 or not x.is_cuda) and not getattr(graph, "is_shard", False):
        src, dst = graph.edges()
        return x[(src if which == "src" else dst).long()]
    return _GatherRows.apply(x, graph, which)


# ---- amortised per-edge parameters with narrow heads (csrc/amort.hip) ---------------------------------------
# MI355X, N = 169,343, K = 128, forward + backward: 122 | 125 | 137 | 238 us for 2 | 4 | 8 | 16 columns against
# 193-273 us for the library GEMMs: the one-pass kernels take up to 8 columns (the library builds them for 16)
NARROW_MAX_HIDDEN, NARROW_MAX_PAR, NARROW_MAX_COLS = 4, 4, 8


def _amort_ws(n_values, dev):
    nbytes = _lib.lib().stag_amort_workspace_bytes(n_values)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev), nbytes


class _NodeProject(torch.autograd.Function):
    """y = x [N, K] . w [K, C] + b for C <= 16 columns: one pass over x forward, one pass backward (dx, dw, db
    together) — the library GEMMs take 75 us per call at N = 169,343, K = 128, C = 1 and run one such call per
    projected column and per gradient (stag_node_project_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, w, b):
        dev = _lib.require_device(x, w, b)
        x, w, b = _f32c(x), _f32c(w), _f32c(b)
        n, K = x.shape
        C_ = w.shape[1]
        y = torch.empty((n, C_), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_node_project_fwd(_lib.ptr(x), x.stride(0), n, K, _lib.ptr(w), _lib.ptr(b), C_,
                                                  _lib.ptr(y), _lib.stream_of(dev))
        _lib.check(rc, "stag_node_project_fwd")
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        dev = x.device
        gy = _f32c(gy)
        n, K = x.shape
        C_ = w.shape[1]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        want_w = ctx.needs_input_grad[1]
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if dx is None and not want_w and not want_b:
            return None, None, None
        dw = torch.empty_like(w) if want_w else None
        db = torch.empty(C_, dtype=torch.float32, device=dev) if want_b else None
        ws, nbytes = _amort_ws((K + 1) * C_, dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_node_project_bwd(_lib.ptr(x), x.stride(0), n, K, _lib.ptr(w), C_, _lib.ptr(gy),
                                                  _lib.ptr(dx), K, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes,
                                                  _lib.stream_of(dev))
        _lib.check(rc, "stag_node_project_bwd")
        return dx, dw, db


def node_project(x, w, b=None):
    """x [N, K] @ w [K, C] (+ b) for a handful of output columns (C <= 8; wider: node_linear)."""
    if w.shape[1] > NARROW_MAX_COLS or not x.is_cuda or x.dim() != 2:
        return node_linear(x, w, b)
    return _NodeProject.apply(x, w, b)


class _HeadDot(torch.autograd.Function):
    """(ft * attn_l).sum(-1) and (ft * attn_r).sum(-1) — GAT's el / er (stag/zoo/gat.py:109-110) — from one pass over
    ft [N, H, F], and d ft, d attn_l, d attn_r from one pass back (stag_head_dot_fwd / _bwd).  As elementwise
    multiply + reduce: 2 x 242 us at cfg5 and as much again backward; as a GEMM with a block-diagonal right side:
    53 + 168 + 47 us in the library."""

    @staticmethod
    def forward(ctx, ft, al, ar):
        dev = _lib.require_device(ft, al, ar)
        n, H, F = ft.shape
        ft = _f32c(ft)
        w = torch.stack([al.reshape(H * F), ar.reshape(H * F)], 0).float().contiguous()
        y = torch.empty((2, n, H), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_head_dot_fwd(_lib.ptr(ft), H * F, n, H, F, _lib.ptr(w), 2, _lib.ptr(y),
                                              _lib.stream_of(dev))
        _lib.check(rc, "stag_head_dot_fwd")
        ctx.save_for_backward(ft, w)
        ctx.wshape = (al.shape, ar.shape)
        return y[0], y[1]

    @staticmethod
    def backward(ctx, gl, gr):
        ft, w = ctx.saved_tensors
        dev = ft.device
        n, H, F = ft.shape
        gy = torch.stack([_f32c(gl), _f32c(gr)], 0)
        dft = torch.empty_like(ft) if ctx.needs_input_grad[0] else None
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dw = torch.empty_like(w) if want_w else None
        ws, nbytes = _amort_ws(2 * H * F, dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_head_dot_bwd(_lib.ptr(ft), H * F, n, H, F, _lib.ptr(w), 2, _lib.ptr(gy), _lib.ptr(dft),
                                              H * F, _lib.ptr(dw), _lib.ptr(ws), nbytes, _lib.stream_of(dev))
        _lib.check(rc, "stag_head_dot_bwd")
        dal = dw[0].reshape(ctx.wshape[0]) if (want_w and ctx.needs_input_grad[1]) else None
        dar = dw[1].reshape(ctx.wshape[1]) if (want_w and ctx.needs_input_grad[2]) else None
        return dft, dal, dar


def head_dot(ft, attn_l, attn_r):
    """el, er [N, H] = (ft * attn_l).sum(-1), (ft * attn_r).sum(-1) for ft [N, H, F], attn_* [1, H, F] | [H, F].
    None when the shape has no one-pass form (F % 4 != 0 or F > 256): the caller takes the GEMM form."""
    if ft.dim() != 3 or not ft.is_cuda or ft.shape[0] == 0:
        return None
    F = ft.shape[2]
    if F < 4 or F > 256 or F % 4 != 0:
        return None
    return _HeadDot.apply(ft, attn_l, attn_r)


def _pre_grad_tables(g, dpre):
    """d P[u, j] = sum over the out-edges of u, d P[v, hidden + j] = sum over the in-edges of v of dpre[e, j] (dpre
    [E, hidden] by edge id of `g`): the aggregation kernel over explicit rows and one broadcast row of ones, on the two
    CSR views of g.  Returns the two [N, hidden] halves."""
    hidden = dpre.shape[1]
    ones = torch.ones(hidden, dtype=torch.float32, device=dpre.device)
    spec = _explicit_spec(dpre)
    d_src, _ = _agg_raw(g.csr_t, ones, hidden, spec, _lib.REDUCE_SUM, None, None, DEFAULT_SEG_LEN, broadcast_x=True)
    d_dst, _ = _agg_raw(g.csr, ones, hidden, spec, _lib.REDUCE_SUM, None, None, DEFAULT_SEG_LEN, broadcast_x=True)
    return d_src, d_dst


class _EdgeMlp(torch.autograd.Function):
    """par_c[e] = b_c + sum_j SiLU(P[src_e, j] + P[dst_e, hidden + j]) wh[j, c]: the heads of an
    AmortizedDistribution with narrow hidden / output widths (stag/distributions.py:178-191, 225-231) on the two
    projected node tables, a thread per edge (stag_edge_mlp_fwd / _bwd).  Returns one [E, 1] tensor per head."""

    @staticmethod
    def forward(ctx, graph, P, wh, bh):
        dev = _lib.require_device(P, wh, bh)
        P, wh, bh = _f32c(P), _f32c(wh), _f32c(bh)
        hidden, n_par = wh.shape
        g = _owner(graph)
        src, dst = g._src, g._dst
        E = src.shape[0]
        par = torch.empty((n_par, E), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_edge_mlp_fwd(_lib.ptr(src), _lib.ptr(dst), E, _lib.ptr(P), _lib.ptr(P[:, hidden:]),
                                              P.stride(0), hidden, _lib.ptr(wh), _lib.ptr(bh), n_par, _lib.ptr(par),
                                              _lib.stream_of(dev))
        _lib.check(rc, "stag_edge_mlp_fwd")
        ctx.graph = g
        ctx.has_bias = bh is not None
        ctx.save_for_backward(P, wh)
        return tuple(par[c].unsqueeze(1) for c in range(n_par))

    @staticmethod
    def backward(ctx, *gs):
        P, wh = ctx.saved_tensors
        g = ctx.graph
        dev = P.device
        hidden, n_par = wh.shape
        src, dst = g._src, g._dst
        E = src.shape[0]
        gpar = torch.stack([_f32c(t).reshape(E) for t in gs], 0)
        dpre = torch.empty((E, hidden), dtype=torch.float32, device=dev)
        dwh = torch.empty_like(wh) if ctx.needs_input_grad[2] else None
        dbh = torch.empty(n_par, dtype=torch.float32, device=dev) if (ctx.has_bias and ctx.needs_input_grad[3]) else None
        ws, nbytes = _amort_ws(36, dev)      # 8 hidden x 4 parameters + 4: the library's largest shape
        with _lib.on_device(dev):
            rc = _lib.lib().stag_edge_mlp_bwd(_lib.ptr(src), _lib.ptr(dst), E, _lib.ptr(P), _lib.ptr(P[:, hidden:]),
                                              P.stride(0), hidden, _lib.ptr(wh), n_par, _lib.ptr(gpar), _lib.ptr(dpre),
                                              _lib.ptr(dwh), _lib.ptr(dbh), _lib.ptr(ws), nbytes, _lib.stream_of(dev))
        _lib.check(rc, "stag_edge_mlp_bwd")
        dP = None
        if ctx.needs_input_grad[1]:
            d_src, d_dst = _pre_grad_tables(g, dpre)
            if getattr(g, "is_shard", False):      # P is the exchanged buffer: destinations are this rank's rows of it
                full = torch.zeros_like(d_src)
                full[g.loc_off:g.loc_off + g.n_rows] = d_dst
                d_dst = full
            dP = torch.cat([d_src, d_dst], 1)
        return None, dP, dwh, dbh


def edge_mlp(graph, P, wh, bh=None):
    """The per-edge heads of a narrow AmortizedDistribution: P [N, 2 hidden] (source half | destination half),
    wh [hidden, n_par], bh [n_par]  ->  n_par tensors [E, 1] by edge id."""
    return _EdgeMlp.apply(graph, P, wh, bh)


# ---- the wide edge embedding of amortised per-edge parameters (csrc/edge_embed.hip) ---------------------------------------
# stag_edge_embed_fwd / _bwd | the composed route (two index_selects, an add and a SiLU over [E, hidden] tensors, the
# pre-activation kept for SiLU's backward, two aggregations of explicit rows behind it).  The values agree within
# tolerance either way: a speed and memory decision only.  True because no timed case is slower than the composed route
# (profiles/r24/edge_embed.txt): the forward alone 59 against 148 us Cora-sized at hidden 1433, 107 against 368 us
# Pubmed-sized at 500, 128 against 327 us on the PPI batch at 50, 258 against 1095 us at the arxiv shape at 128; forward +
# backward 168 / 293 / 383 / 718 against 265 / 599 / 589 / 1727 us (two repeats of the composed route differ by 0.0-7.3 us,
# of the fused one by 2.5-8.9); peak allocation of a forward + backward 73 / 207 / 157 / 572 against 188 / 545 / 447 /
# 1545 MiB; a StagLayer(GCN, AmortizedDistribution(in, in), vi=True) training step 5.26 / 5.85 / 3.85 / 7.74 against 5.36 /
# 6.19 / 4.08 / 8.79 ms.
EDGE_EMBED_FUSED = True


def edge_embed_why_not(graph, p_src, p_dst, mods):
    """The first reason the wide branch of AmortizedDistribution.condition keeps the composed route, or None: the hidden
    layer h = SiLU(p_src[src] + p_dst[dst]) comes from one stag_edge_embed_fwd launch and its gradients from two
    stag_edge_embed_bwd launches.  mods: the modules of the embedding MLP.  One clause per case that has no fused form."""
    if not EDGE_EMBED_FUSED:
        return "switch"
    if getattr(graph, "is_shard", False):
        return "shard"
    if not (getattr(p_src, "is_cuda", False) and getattr(p_dst, "is_cuda", False)) or not hasattr(graph, "_src"):
        return "device"
    if p_src.dim() != 2 or p_dst.dim() != 2 or p_src.shape != p_dst.shape or p_src.shape[1] == 0:
        return "shape"
    if any(t.dtype not in (torch.float32, torch.float16, torch.bfloat16) for t in (p_src, p_dst)):
        return "dtype"
    if torch.compiler.is_compiling():
        return "compiling"
    mods = list(mods)
    if len(mods) != 2 or not isinstance(mods[0], torch.nn.Linear) or type(mods[1]) is not torch.nn.SiLU:
        return "embedding"
    return None


def _rows32(t):
    """t as fp32 rows with unit column stride: the tensor itself when it already is (any row stride the library takes —
    the half of an [N, 2 hidden] table stays a view), else a packed copy."""
    if (t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] <= t.stride(0) < _MAX_ROW_STRIDE
            and t.shape[0] > 1):
        return t
    return _f32c(t)


def _edge_embed_fwd_raw(src, dst, ps, pd, out=None):
    """One stag_edge_embed_fwd: h [E, hidden] = SiLU(ps[src] + pd[dst]) on fp32 rows (_rows32), edges by edge id."""
    dev = _lib.require_device(src, dst, ps, pd)
    E, hidden = src.shape[0], ps.shape[1]
    h = torch.empty((E, hidden), dtype=torch.float32, device=dev) if out is None else out
    with _lib.on_device(dev):
        rc = _lib.lib().stag_edge_embed_fwd(_lib.ptr(src), _lib.ptr(dst), E, _lib.ptr(ps), max(ps.stride(0), hidden),
                                            _lib.ptr(pd), max(pd.stride(0), hidden), hidden, _lib.ptr(h),
                                            max(h.stride(0), hidden), _lib.stream_of(dev))
    _lib.check(rc, "stag_edge_embed_fwd")
    return h


def _edge_embed_bwd_raw(csrv, own, other, g, seg_len=DEFAULT_SEG_LEN, out=None):
    """One stag_edge_embed_bwd on csrv: d_own [n_dst, hidden] from g [E, hidden] by edge id.  graph.csr with own = pd,
    other = ps gives d pd; graph.csr_t with own = ps, other = pd gives d ps.  Plan order; bound through ctypes."""
    dev = _lib.require_device(csrv.indptr, own, other, g)
    hidden = own.shape[1]
    if out is None:
        out = torch.empty((csrv.n_dst, hidden), dtype=torch.float32, device=dev)
    if csrv.n_dst == 0:
        return out
    plan_t = csrv.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], hidden, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv, seg_len, (hidden + 255) // 256, nbytes, dev, plan_t)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_edge_embed_bwd(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(own), max(own.stride(0), hidden),
            _lib.ptr(other), max(other.stride(0), hidden), hidden, _lib.ptr(g), max(g.stride(0), hidden), _lib.ptr(out),
            max(out.stride(0), hidden), _lib.stream_of(dev))
    _lib.check(rc, "stag_edge_embed_bwd")
    return out


class _EdgeEmbed(torch.autograd.Function):
    """h [E, hidden] = SiLU(p_src[src] + p_dst[dst]) by edge id: the hidden layer of an AmortizedDistribution with wide
    heads on the two projected node tables (stag/distributions.py:178-183, 225-227), one launch forward
    (stag_edge_embed_fwd).  Only the two [N, hidden] tables are saved: the backward forms the pre-activation again and
    sums g * SiLU' over the in-edges of every destination and the out-edges of every source (stag_edge_embed_bwd on the
    two CSR views), so nothing [E, hidden] is kept between the passes or allocated by the backward."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, p_src, p_dst, graph):
        g = _owner(graph)
        ps, pd = _rows32(p_src), _rows32(p_dst)
        ctx.graph = g
        ctx.save_for_backward(ps, pd)
        return _edge_embed_fwd_raw(g._src, g._dst, ps, pd)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gh):
        ps, pd = ctx.saved_tensors
        g = ctx.graph
        gh = _rows32(gh)
        d_src = _edge_embed_bwd_raw(g.csr_t, ps, pd, gh) if ctx.needs_input_grad[0] else None
        d_dst = _edge_embed_bwd_raw(g.csr, pd, ps, gh) if ctx.needs_input_grad[1] else None
        return d_src, d_dst, None


def edge_embed(graph, p_src, p_dst):
    """SiLU(p_src[u] + p_dst[v]) for every edge u -> v of graph, [E, hidden] by edge id, from the two projected node
    tables [N, hidden] (unit column stride, any row stride).  edge_embed_why_not says when condition() takes it."""
    n = graph.number_of_nodes()
    if p_src.dim() != 2 or p_src.shape != p_dst.shape or p_src.shape[0] != n or p_src.shape[1] == 0:
        raise ValueError(f"edge_embed: two [{n}, hidden] tables, got {tuple(p_src.shape)} and {tuple(p_dst.shape)}")
    return _EdgeEmbed.apply(p_src, p_dst, graph)


# ---- the node block between two layers: BatchNorm1d (+ ReLU) (+ Dropout) on [N, D] rows as fused passes ---------------
# FeatOnlyLayer(Sequential(BatchNorm1d(hidden), ReLU(), Dropout(0.5))) of every arxiv script is eight torch launches
# forward and backward; here it is two small-output reductions and one elementwise pass forward, and the same again
# plus nothing saved but x backward.  With the switch on, the block's dropout mask comes from random.node_generator's
# counters (the project's Bernoulli draw), not from torch's generator: the same law, another mask for a given seed.
# tools/node_block_time.py holds the switch to the project's rule: max(f, f') <= mean(c, c') + |c - c'| in every case.
# MI355X, training block with Dropout(0.5), torch / fused (profiles/r26/node_block.txt): forward 255 / 126 us at
# [169,343, 128], 542 / 173 at [169,343, 256], 318 / 86 at [56,944, 256]; forward + backward 576 / 263, 1258 / 403, 690 / 177;
# peak allocation of a step 248 / 84, 498 / 169, 168 / 58 MiB; the arxiv GCN epoch 3.27 -> 2.62 ms, GraphSAGE 4.03 -> 3.39.
# The Cora-sized [2,708, 16] is bound by the host's calls, not the device, and misses the rule: 46 / 57 us forward, 115 /
# 135 forward + backward.  One missed case ships the switch off; turn it on for the arxiv- and PPI-sized models.
NODE_BLOCK_FUSED = False


def node_block_parts(module):
    """(BatchNorm1d, ReLU | None, Dropout | None) when module is exactly a Sequential of BatchNorm1d, then optionally
    ReLU, then optionally Dropout (the classes themselves: a subclass may compute anything), else None."""
    if type(module) is not torch.nn.Sequential:
        return None
    mods = list(module)
    if not mods or type(mods[0]) is not torch.nn.BatchNorm1d:
        return None
    bn, rest, relu, dropout = mods[0], mods[1:], None, None
    if rest and type(rest[0]) is torch.nn.ReLU:
        relu, rest = rest[0], rest[1:]
    if rest and type(rest[0]) is torch.nn.Dropout:
        dropout, rest = rest[0], rest[1:]
    if rest:
        return None
    if any(t is not None and t.dtype != torch.float32 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return None
    return bn, relu, dropout


def node_block_why_not(module, x):
    """The first reason FeatOnlyLayer keeps the torch route for `module` on x, or None: stag_node_norm_stats / _fwd and,
    under autograd, _bwd run the block.  One clause per case that has no fused form.  (A double backward cannot be seen
    from here: _NodeBlock is once_differentiable and raises in one; turn the switch off for it.)"""
    if not NODE_BLOCK_FUSED:
        return "switch"
    parts = node_block_parts(module)
    if parts is None:
        return "module"
    bn, _relu, dropout = parts
    if x.dim() != 2 or x.shape[1] != bn.num_features:       # ([N, C, L] is out of scope; a wrong width is torch's to refuse)
        return "shape"
    if x.dtype != torch.float32:
        return "dtype"
    if not x.is_cuda:
        return "device"
    if x.shape[0] < (2 if (bn.training or bn.running_mean is None) else 1):   # torch raises on one training row: let it
        return "rows"
    if dropout is not None and dropout.p >= 1:
        return "dropout"
    if torch.compiler.is_compiling():
        return "compiling"
    if torch.cuda.is_current_stream_capturing():            # the host counter of the mask's generator would freeze
        return "capturing"
    return None


def _node_drop_struct(drop):
    """(p, seed, offset, epoch tensor | None) -> stag_node_drop, or None"""
    if drop is None:
        return None
    d = _lib.NodeDrop()
    d.keep_prob = 1.0 - float(drop[0])
    d.seed, d.offset = int(drop[1]) & _MASK64, int(drop[2]) & _MASK64
    d.epoch = _lib.ptr(drop[3])
    return d


def _node_ws(n, D, dev):
    nbytes = _lib.lib().stag_node_norm_workspace_bytes(n, D)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev), nbytes


def _node_stats_raw(x, eps, running_mean=None, running_var=None, factor=0.0):
    """One stag_node_norm_stats: (mean, rstd) [D] of the columns of x; the running buffers are updated in place."""
    dev = _lib.require_device(x, running_mean, running_var)
    n, D = x.shape
    mean = torch.empty(D, dtype=torch.float32, device=dev)
    rstd = torch.empty(D, dtype=torch.float32, device=dev)
    ws, nbytes = _node_ws(n, D, dev)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_node_norm_stats(_lib.ptr(x), max(x.stride(0), D), n, D, eps, _lib.ptr(mean), _lib.ptr(rstd),
                                             _lib.ptr(running_mean), _lib.ptr(running_var), factor, _lib.ptr(ws), nbytes,
                                             _lib.stream_of(dev))
    _lib.check(rc, "stag_node_norm_stats")
    return mean, rstd


def _node_fwd_raw(x, mean, rstd, gamma, beta, relu, drop, out=None):
    """One stag_node_norm_fwd on fp32 rows (_rows32)."""
    dev = _lib.require_device(x, mean, rstd, gamma, beta)
    n, D = x.shape
    y = torch.empty((n, D), dtype=torch.float32, device=dev) if out is None else out
    d = _node_drop_struct(drop)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_node_norm_fwd(_lib.ptr(x), max(x.stride(0), D), n, D, _lib.ptr(mean), _lib.ptr(rstd),
                                           _lib.ptr(gamma), _lib.ptr(beta), int(relu), C.byref(d) if d is not None else None,
                                           _lib.ptr(y), max(y.stride(0), D), _lib.stream_of(dev))
    _lib.check(rc, "stag_node_norm_fwd")
    return y


def _node_bwd_raw(x, g, mean, rstd, gamma, beta, relu, drop, batch_stats, want_dx=True, want_dgamma=True, want_dbeta=True):
    """One stag_node_norm_bwd: (dx [N, D], dgamma [D], dbeta [D]), None for what was not asked for."""
    dev = _lib.require_device(x, g, mean, rstd, gamma, beta)
    n, D = x.shape
    dx = torch.empty((n, D), dtype=torch.float32, device=dev) if want_dx else None
    dgamma = torch.empty(D, dtype=torch.float32, device=dev) if want_dgamma else None
    dbeta = torch.empty(D, dtype=torch.float32, device=dev) if want_dbeta else None
    ws, nbytes = _node_ws(n, D, dev)
    d = _node_drop_struct(drop)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_node_norm_bwd(_lib.ptr(x), max(x.stride(0), D), _lib.ptr(g), max(g.stride(0), D), n, D,
                                           _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(beta), int(relu),
                                           C.byref(d) if d is not None else None, int(batch_stats), _lib.ptr(dx), D,
                                           _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), nbytes, _lib.stream_of(dev))
    _lib.check(rc, "stag_node_norm_bwd")
    return dx, dgamma, dbeta


class _NodeBlock(torch.autograd.Function):
    """y = dropout(relu(batch_norm(x))) from one elementwise pass over x (stag_node_norm_fwd) with the statistics handed
    over.  Saved: x, the [D] vectors mean, rstd, gamma, beta and the drop record (p, seed, offset, epoch) — nothing
    [N, D]-sized besides x: the backward (stag_node_norm_bwd) forms the pre-activation and draws the mask again."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, gamma, beta, mean, rstd, batch_stats, relu, drop):
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.batch_stats, ctx.relu, ctx.drop = batch_stats, relu, drop
        return _node_fwd_raw(x, mean, rstd, gamma, beta, relu, drop)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dgamma, dbeta = _node_bwd_raw(x, _rows32(g), mean, rstd, gamma, beta, ctx.relu, ctx.drop, ctx.batch_stats,
                                          want_dx=need[0], want_dgamma=gamma is not None and need[1],
                                          want_dbeta=beta is not None and need[2])
        return dx, dgamma, dbeta, None, None, None, None, None


def node_block(x, bn, relu=None, dropout=None, generator=None):
    """Dropout(ReLU(BatchNorm1d(x))) on x [N, D] with the modules' own parameters, buffers and modes: what
    Sequential(bn, relu, dropout)(x) computes (relu, dropout: the module or None), with torch.nn.BatchNorm1d's buffer
    updates.  A live dropout takes one offset of `generator` (random.node_generator) for its mask.
    node_block_why_not says when FeatOnlyLayer takes it."""
    from . import random as _random
    batch_stats = bn.training or bn.running_mean is None
    drop = None
    if dropout is not None and dropout.training and dropout.p > 0:
        gen = generator if generator is not None else _random.node_generator
        drop = (float(dropout.p), gen.seed ^ _random.NODE_DROP_DOMAIN, gen.next_offset(), gen.device_epoch)
    xr = _rows32(x)
    with torch.no_grad():
        if batch_stats:
            rm = rv = None
            factor = 0.0
            if bn.training and bn.running_mean is not None:
                rm, rv = bn.running_mean, bn.running_var
                if bn.num_batches_tracked is not None:
                    bn.num_batches_tracked.add_(1)
                factor = float(bn.momentum) if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            mean, rstd = _node_stats_raw(xr, float(bn.eps), rm, rv, factor)
        else:
            mean, rstd = bn.running_mean, torch.rsqrt(bn.running_var + bn.eps)
    return _NodeBlock.apply(xr, bn.weight, bn.bias, mean, rstd, batch_stats, relu is not None, drop)


class _NormalKlMean(torch.autograd.Function):
    """mean over all elements of KL(N(loc, exp(log_scale)) || N(p_loc, p_scale)) with one-element prior parameters
    (torch.distributions.kl._kl_normal_normal; stag/layers.py:132-145): one pass forward, one backward, against
    ~25 elementwise passes over the [E, out] tensors (stag_normal_kl_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, loc, log_scale, p_loc, p_scale):
        dev = _lib.require_device(loc, log_scale, p_loc, p_scale)
        loc, log_scale = _f32c(loc), _f32c(log_scale)
        p_loc, p_scale = _f32c(p_loc.reshape(1)), _f32c(p_scale.reshape(1))
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws, nbytes = _amort_ws(2, dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_normal_kl_fwd(_lib.ptr(loc), _lib.ptr(log_scale), loc.numel(), _lib.ptr(p_loc),
                                               _lib.ptr(p_scale), _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_of(dev))
        _lib.check(rc, "stag_normal_kl_fwd")
        ctx.save_for_backward(loc, log_scale, p_loc, p_scale)
        ctx.shapes = (loc.shape, log_scale.shape)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        loc, log_scale, p_loc, p_scale = ctx.saved_tensors
        dev = loc.device
        g = _f32c(g.reshape(1))
        need = ctx.needs_input_grad
        dloc = torch.empty_like(loc) if need[0] else None
        dls = torch.empty_like(log_scale) if need[1] else None
        dpl = torch.empty(1, dtype=torch.float32, device=dev) if need[2] else None
        dps = torch.empty(1, dtype=torch.float32, device=dev) if need[3] else None
        ws, nbytes = _amort_ws(2, dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_normal_kl_bwd(_lib.ptr(loc), _lib.ptr(log_scale), loc.numel(), _lib.ptr(p_loc),
                                               _lib.ptr(p_scale), _lib.ptr(g), _lib.ptr(dloc), _lib.ptr(dls),
                                               _lib.ptr(dpl), _lib.ptr(dps), _lib.ptr(ws), nbytes, _lib.stream_of(dev))
        _lib.check(rc, "stag_normal_kl_bwd")
        return dloc, dls, dpl, dps


def normal_kl_mean(loc, log_scale, p_loc, p_scale):
    """KL(N(loc, exp(log_scale)) || N(p_loc, p_scale)).mean(), loc / log_scale of one shape, the prior's two
    parameters one-element tensors (their original shapes get their gradients back)."""
    if loc.shape != log_scale.shape or p_loc.numel() != 1 or p_scale.numel() != 1 or loc.numel() == 0:
        raise ValueError("normal_kl_mean: same-shape loc / log_scale and a one-element prior")
    return _NormalKlMean.apply(loc, log_scale, p_loc, p_scale)


# ---- the likelihood end of the objective: the masked mean NLL of model.loss as fused passes (csrc/nll.hip) -------------
# -likelihood.log_prob(out, y) and models._masked_mean are ~12 torch launches forward over [N, C] (row sum, divide,
# clamp, log, gather, negate, where, sum, mask.sum, divide) and as many again backward, once per Monte-Carlo sample;
# stag_nll_categorical_fwd / _bwd and stag_nll_bernoulli_fwd / _bwd are two launches forward (slab partials, merge) and
# one backward, read only the rows inside the mask and keep nothing [N, C]-sized but the probabilities.
# tools/loss_head_time.py holds the switch to the project's rule: max(f, f') <= mean(c, c') + |c - c'| in every case.
# MI355X, composed / fused (profiles/r27/loss_head.txt), forward and forward + backward in us: Categorical [169,343, 40]
# with a 0.54 mask 98 / 29 and 307 / 97, without a mask 73 / 27 and 239 / 73; Cora [2,708, 7] with 140 masked rows 78 / 27
# and 274 / 80; Pubmed [19,717, 3] with 60 rows 80 / 27 and 283 / 80; a readout batch [128, 10] 45 / 25 and 210 / 75;
# Bernoulli [56,944, 121] 161 / 43 and 323 / 75 (the worse of two repeats of the fused route against the mean of two of
# the composed one, which differ by 0 - 8 us).  The small cases are bound by the host's calls on both routes: 3 launches
# against ~25.  Peak allocation of a step at the arxiv shape 105 / 0 MiB over the gradient, 131 / 0 at the PPI shape.
# Whole steps, switch off / on: the arxiv GCN epoch 3.26 / 3.00 ms, a Cora-sized two-layer GCN step 0.98 / 0.72 ms.
# Every case meets the rule: the switch ships on.
NLL_FUSED = True


def _nll_kind(likelihood):
    """"categorical" | "bernoulli" for exactly the two shipped classes over their original torch distribution (a
    subclass may compute anything), else None."""
    from . import likelihoods as _lk
    if type(likelihood) is _lk.CategoricalLikelihood and likelihood.distribution is torch.distributions.Categorical:
        return "categorical"
    if type(likelihood) is _lk.BernoulliLikelihood and likelihood.distribution is torch.distributions.Bernoulli:
        return "bernoulli"
    return None


def _nll_form_why_not(likelihood, feat, y, mask):
    from . import likelihoods as _lk
    kind = _nll_kind(likelihood)
    if kind is None:
        return "likelihood"
    if _lk.VALIDATE_ON_DEVICE:                                # torch's argument check is wanted: only torch runs it
        return "validating"
    if not torch.is_tensor(y) or not hasattr(feat, "dim"):
        return "labels"
    if not feat.is_cuda:
        return "device"
    if feat.dtype != torch.float32:
        return "dtype"
    if feat.dim() != 2 or feat.shape[0] == 0 or feat.shape[1] == 0:
        return "shape"
    n, C_ = feat.shape
    if feat.stride(1) != 1 or feat.stride(0) < C_:
        return "stride"
    if y.device != feat.device:
        return "labels"
    if kind == "categorical":
        if y.dtype != torch.int64 or tuple(y.shape) != (n,):             # (int32 or float labels: torch's to take)
            return "labels"
    elif y.dtype != torch.float32 or y.shape != feat.shape or y.stride(1) != 1 or y.stride(0) < C_:
        return "labels"
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (n,)):
        return "mask"                                         # (an index tensor, a weight: nll[mask] gives it a meaning)
    if y.requires_grad:
        return "label gradient"
    if torch.compiler.is_compiling():
        return "compiling"
    return None


def nll_why_not(likelihood, feat, y, mask=None):
    """The first reason Likelihood.mean_nll keeps the composed route (-log_prob, then models._masked_mean) for feat
    [N, C], labels y and mask, or None: one stag_nll_*_fwd gives the masked mean and, under autograd, one stag_nll_*_bwd
    its gradient.  One clause per case that has no fused form.  A host mask is fine: it is moved to the device, as
    _masked_mean moves it."""
    if not NLL_FUSED:
        return "switch"
    return _nll_form_why_not(likelihood, feat, y, mask)


def _nll_ws(n, C_, dev):
    nbytes = _lib.lib().stag_nll_workspace_bytes(n, C_)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev), nbytes


class _CategoricalNll(torch.autograd.Function):
    """mean over the masked rows of -Categorical(probs=probs).log_prob(y) (stag_nll_categorical_fwd / _bwd).  Saved:
    probs, y, mask and the one-element denom — nothing [N, C]-sized besides the input."""

    @staticmethod
    def forward(ctx, probs, y, mask):
        dev = _lib.require_device(probs, y, mask)
        n, C_ = probs.shape
        out = torch.empty(2, dtype=torch.float32, device=dev)     # value, denom
        ws, nbytes = _nll_ws(n, C_, dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_nll_categorical_fwd(_lib.ptr(probs), max(probs.stride(0), C_), n, C_, _lib.ptr(y),
                                                     _lib.ptr(mask), _lib.ptr(out), out.data_ptr() + 4, _lib.ptr(ws),
                                                     nbytes, _lib.stream_of(dev))
        _lib.check(rc, "stag_nll_categorical_fwd")
        ctx.save_for_backward(probs, y, mask, out)
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        probs, y, mask, out = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dev = probs.device
        n, C_ = probs.shape
        g = _f32c(g.reshape(1))
        dprobs = torch.empty((n, C_), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_nll_categorical_bwd(_lib.ptr(probs), max(probs.stride(0), C_), n, C_, _lib.ptr(y),
                                                     _lib.ptr(mask), _lib.ptr(g), out.data_ptr() + 4, _lib.ptr(dprobs),
                                                     C_, _lib.stream_of(dev))
        _lib.check(rc, "stag_nll_categorical_bwd")
        return dprobs, None, None


class _BernoulliNll(torch.autograd.Function):
    """mean over the elements of the masked rows of -Bernoulli(probs=probs).log_prob(y) (stag_nll_bernoulli_fwd /
    _bwd).  Saved: probs, y, mask and the one-element denom."""

    @staticmethod
    def forward(ctx, probs, y, mask):
        dev = _lib.require_device(probs, y, mask)
        n, C_ = probs.shape
        out = torch.empty(2, dtype=torch.float32, device=dev)     # value, denom
        ws, nbytes = _nll_ws(n, C_, dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_nll_bernoulli_fwd(_lib.ptr(probs), max(probs.stride(0), C_), _lib.ptr(y),
                                                   max(y.stride(0), C_), n, C_, _lib.ptr(mask), _lib.ptr(out),
                                                   out.data_ptr() + 4, _lib.ptr(ws), nbytes, _lib.stream_of(dev))
        _lib.check(rc, "stag_nll_bernoulli_fwd")
        ctx.save_for_backward(probs, y, mask, out)
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        probs, y, mask, out = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dev = probs.device
        n, C_ = probs.shape
        g = _f32c(g.reshape(1))
        dprobs = torch.empty((n, C_), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_nll_bernoulli_bwd(_lib.ptr(probs), max(probs.stride(0), C_), _lib.ptr(y),
                                                   max(y.stride(0), C_), n, C_, _lib.ptr(mask), _lib.ptr(g),
                                                   out.data_ptr() + 4, _lib.ptr(dprobs), C_, _lib.stream_of(dev))
        _lib.check(rc, "stag_nll_bernoulli_bwd")
        return dprobs, None, None


def nll_mean(likelihood, feat, y, mask=None):
    """_masked_mean(-likelihood.log_prob(feat, y), mask) for a CategoricalLikelihood (y int64 [N]) or a
    BernoulliLikelihood (y fp32 [N, C]) on device probabilities feat [N, C]; mask None or bool [N] (on the host: moved).
    No masked row gives NaN, as the mean of nothing.  nll_why_not says when Likelihood.mean_nll takes it."""
    why = _nll_form_why_not(likelihood, feat, y, mask)
    if why is not None:
        raise ValueError(f"nll_mean: no fused form ({why})")
    if mask is not None:
        if mask.device != feat.device:
            mask = mask.to(feat.device)
        mask = mask.contiguous()
    if _nll_kind(likelihood) == "categorical":
        return _CategoricalNll.apply(feat, y.contiguous(), mask)
    return _BernoulliNll.apply(feat, y, mask)


# ---- the sample-based KL fallback against a mixture prior (stag/layers.py:141-143) -----------------------------------
# stag_sample_kl | the composed route (EdgeNoise.materialize(), both log_probs as eager torch over [E, Dn] and, for the
# mixture, [E, Dn, K]).  The value is the same within tolerance either way: a speed and memory decision only.  True
# because the fused training step measures faster at the arxiv shape (GCN 128 -> 128, 2-component prior,
# profiles/r11/sample_kl.txt): 1.41 against 19.06 ms with learned scalars, 1.78 against 19.46 ms with [E, 1] amortised
# heads (two repeats of the composed step differ by 0.01-0.04 ms); peak allocation of a step 0.5 against 8.8 GB.
SAMPLED_KL_FUSED = True


def sampled_kl_why_not(noise, prior):
    """The first reason StagLayer.kl_divergence keeps the composed route for its sample-based estimate, or None: the
    estimate and its gradients come from one stag_sample_kl launch and `noise` stays a descriptor.  One clause per
    refusal of the entry point (include/stag_hip.h) and per case that has no fused form."""
    if not SAMPLED_KL_FUSED:
        return "switch"
    if not isinstance(noise, EdgeNoise) or noise.kind != _lib.NOISE_NORMAL:
        return "noise kind"
    if noise.in_norm:
        return "in-norm"
    if noise.param_mode == _lib.PARAM_PER_EDGE:
        return "per-edge parameters"
    if noise.deriv:
        return "derivative selector"
    if noise.n_samples != 1:
        return "monte-carlo"
    graph = noise.graph
    if getattr(graph, "is_shard", False):
        return "shard"
    if graph.number_of_edges() == 0:
        return "no edges"
    if torch.compiler.is_compiling():
        return "compiling"
    D = torch.distributions
    if not isinstance(prior, D.MixtureSameFamily) or type(prior.component_distribution) is not D.Normal:
        return "prior"
    comp = prior.component_distribution
    tensors = (prior.mixture_distribution.logits, comp.loc, comp.scale)
    if len(comp.batch_shape) != 1 or not 1 <= comp.batch_shape[0] <= _lib.KL_MAX_COMPONENTS:
        return "prior"
    if any(t.shape != comp.batch_shape for t in tensors):
        return "prior"
    dev = torch.device(graph.device)
    if any(t.device != dev for t in tensors):
        return "prior device"
    if any(t.requires_grad for t in tensors):
        return "prior gradients"
    if dev.type != "cuda":
        return "device"
    return None


def _sample_kl_raw(noise, mixture, want_grad):
    """One stag_sample_kl: (kl_mean [1], d kl_mean / d p0, d kl_mean / d p1), the gradients in the layout of the
    descriptor's parameters ([1], [Dn] or [E, 1]) or None."""
    csrv = noise.graph.csr
    dev = _lib.require_device(csrv.indptr)
    E, dn = csrv.n_edges, noise.dn
    comp = mixture.component_distribution
    logw = _f32c(mixture.mixture_distribution.logits.detach())
    mloc, mscale = _f32c(comp.loc.detach()), _f32c(comp.scale.detach())
    _lib.require_device(logw, mloc, mscale, csrv.indptr)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    d0 = d1 = None
    if want_grad:
        shape = {_lib.PARAM_SCALAR: (1,), _lib.PARAM_PER_CHANNEL: (dn,), _lib.PARAM_PER_EDGE1: (E, 1)}[noise.param_mode]
        d0 = torch.empty(shape, dtype=torch.float32, device=dev)
        d1 = torch.empty(shape, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().stag_sample_kl_workspace_bytes(E, dn)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    spec, cs = noise.spec(), csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_sample_kl(C.byref(cs), C.byref(spec), dn, _lib.ptr(logw), _lib.ptr(mloc), _lib.ptr(mscale),
                                       logw.numel(), _lib.ptr(out), _lib.ptr(d0), _lib.ptr(d1), _lib.ptr(ws), nbytes,
                                       _lib.stream_of(dev))
    _lib.check(rc, "stag_sample_kl")
    return out, d0, d1


class _SampledKlMean(torch.autograd.Function):
    """q.log_prob(w).sum(-1).mean() - mixture.log_prob(w).sum(-1).mean() on the sample a descriptor stands for
    (stag/layers.py:141-143), differentiated through the reparameterised draw as the reference's `rsample` is.  The
    forward launch returns the value AND both parameter gradients (two tensors of the parameters' size, never [E, Dn]);
    the backward scales them by the incoming gradient: no second launch."""

    @staticmethod
    def forward(ctx, p0, p1, noise, mixture):
        out, d0, d1 = _sample_kl_raw(noise, mixture, True)
        ctx.save_for_backward(d0, d1)
        ctx.shapes = (p0.shape, p1.shape)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        grads = [None, None]
        for i, d in enumerate(ctx.saved_tensors):
            if not ctx.needs_input_grad[i]:
                continue
            d, shape = d * g, ctx.shapes[i]
            if d.numel() == shape.numel():
                grads[i] = d.reshape(shape)
            elif shape.numel() == 1:                 # a one-element parameter that travelled as a row
                grads[i] = d.sum().reshape(shape)
            else:
                grads[i] = d.sum_to_size(shape)
        return grads[0], grads[1], None, None


def sampled_kl_mean(noise, mixture):
    """The sample-based KL estimate of a Normal `noise` descriptor against a MixtureSameFamily of Normals, from the
    counters (stag_sample_kl): an autograd function over noise.grad_params as they are, the plain value when there are
    none.  sampled_kl_why_not(noise, mixture) says when it applies."""
    why = sampled_kl_why_not(noise, mixture)
    if why is not None and why != "switch":
        raise ValueError(f"sampled_kl_mean does not apply: {why}")
    if noise.grad_params is not None and torch.is_grad_enabled():
        dev = noise.graph.device
        p0, p1 = (torch.as_tensor(p, dtype=torch.float32, device=dev) for p in noise.grad_params)
        if p0.requires_grad or p1.requires_grad:
            return _SampledKlMean.apply(p0, p1, noise, mixture)
    return _sample_kl_raw(noise, mixture, False)[0].reshape(())


# ---- the contrastive NLL of amortised edge noise (stag/models.py:7-25; csrc/contrastive.hip) ---------------------------
# stag_contrastive_nll | the composed route (models.nll_contrastive as the reference wrote it: an [E, 2 in] concatenation of
# the fake endpoints' features, the MLP over its E rows, two Normal objects).  The value is the same within tolerance
# either way: a speed and memory decision only.  True because the fused training step of the reference script's model
# (two StagLayer(GCN) over AmortizedDistribution(in, 1), StagModelContrastive) measures faster at all three shapes
# (profiles/r13/contrastive.txt): 3.68 against 4.81 ms Cora-sized, 3.18 against 5.09 ms Pubmed-sized, 3.66 against 15.15 ms
# at the arxiv shape (two repeats of the composed step differ by 0.03-0.05 ms); peak allocation of a step 30 / 80 / 302
# against 306 / 869 / 2400 MiB.  The backward's two CSR views of the fake graph cost 0.11 / 0.16 / 0.41 ms of that.
CONTRASTIVE_FUSED = True


def contrastive_why_not(q_a, graph, feat):
    """The first reason models.nll_contrastive keeps the composed route, or None: the term and its gradients come from
    one stag_contrastive_nll launch on the projected tables of q_a._narrow_tables(feat).  One clause per case that has no
    fused form."""
    if not CONTRASTIVE_FUSED:
        return "switch"
    if not getattr(feat, "is_cuda", False) or feat.dim() != 2:
        return "features"
    mlp = getattr(q_a, "embedding_mlp", None)
    lin = mlp[0] if mlp is not None and len(mlp) else None
    if not isinstance(lin, torch.nn.Linear) or not q_a._narrow(graph, lin):
        return "not narrow"
    if q_a.base_distribution_class is not torch.distributions.Normal or list(q_a.new_parameter_names) != ["loc", "log_scale"]:
        return "base distribution"
    E = graph.number_of_edges()
    par = q_a.new_parameters
    if not isinstance(par, dict) or list(par) != ["loc", "log_scale"] or not all(
            torch.is_tensor(t) and tuple(t.shape) == (E, 1) and t.device == feat.device for t in par.values()):
        return "parameters"
    if getattr(graph, "is_shard", False):
        return "shard"
    if E == 0:
        return "no edges"
    if torch.compiler.is_compiling():
        return "compiling"
    return None


def _contrastive_raw(loc, log_scale, fake_src, fake_dst, P, hidden, wh, bh, want=(False,) * 5, pos=1.0, neg=0.0):
    """One stag_contrastive_nll on fp32 contiguous tensors: (nll_mean [1], dloc, dlog_scale, dpre, dwh, dbh), a gradient
    None where `want` does not ask for it.  P [N, >= 2 hidden]: source half | destination half, any row stride."""
    dev = _lib.require_device(loc, log_scale, fake_src, fake_dst, P, wh, bh)
    E = fake_src.shape[0]
    out = torch.empty(1, dtype=torch.float32, device=dev)
    shapes = ((E,), (E,), (E, hidden), (hidden, 2), (2,))
    grads = [torch.empty(sh, dtype=torch.float32, device=dev) if w else None for sh, w in zip(shapes, want)]
    nbytes = _lib.lib().stag_contrastive_nll_workspace_bytes(hidden)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_contrastive_nll(_lib.ptr(loc), _lib.ptr(log_scale), E, _lib.ptr(fake_src), _lib.ptr(fake_dst),
                                             _lib.ptr(P), _lib.ptr(P[:, hidden:]), P.stride(0), hidden, _lib.ptr(wh),
                                             _lib.ptr(bh), pos, neg, _lib.ptr(out), *[_lib.ptr(t) for t in grads],
                                             _lib.ptr(ws), nbytes, _lib.stream_of(dev))
    _lib.check(rc, "stag_contrastive_nll")
    return (out, *grads)


class _ContrastiveNll(torch.autograd.Function):
    """mean_e [-N(loc_e, exp(log_scale_e)).log_prob(1) - N(m'_e, exp(l'_e)).log_prob(0)] with (m', l') the heads of the
    narrow MLP on the fake edge (fake_src_e, fake_dst_e) of the projected tables P (stag/models.py:7-25).  The forward
    launch returns the value and, for the inputs that need one, the gradient (loc, log_scale: [E]; P: dpre [E, hidden];
    wh, bh); the backward scales them by the incoming gradient and — only if P needs a gradient — sums dpre over the
    fake graph's out- and in-edges (two CSR views built for this one use, a stable sort each: a deterministic
    scatter).  Nothing [E, 2 in]-sized exists on either pass."""

    @staticmethod
    def forward(ctx, loc, log_scale, P, wh, bh, fake_src, fake_dst):
        E, hidden = fake_src.shape[0], wh.shape[0]
        need = ctx.needs_input_grad[:5]
        want = (need[0], need[1], need[2], need[3], need[4] and bh is not None)
        out, *grads = _contrastive_raw(_f32c(loc).reshape(E), _f32c(log_scale).reshape(E), fake_src, fake_dst, _f32c(P),
                                       hidden, _f32c(wh), _f32c(bh), want)
        ctx.save_for_backward(*grads, fake_src, fake_dst)
        ctx.shapes = (loc.shape, log_scale.shape, P.shape[0])
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        dloc, dls, dpre, dwh, dbh, fake_src, fake_dst = ctx.saved_tensors
        dP = None
        if dpre is not None:
            fake = Graph(fake_src, fake_dst, ctx.shapes[2], _trusted=True)
            dP = torch.cat(_pre_grad_tables(fake, dpre), 1) * g
        return (None if dloc is None else (dloc * g).reshape(ctx.shapes[0]),
                None if dls is None else (dls * g).reshape(ctx.shapes[1]),
                dP, None if dwh is None else dwh * g, None if dbh is None else dbh * g, None, None)


def contrastive_nll(q_a, graph, feat, fake_src, fake_dst):
    """The contrastive term of models.nll_contrastive for a narrow AmortizedDistribution over a Normal whose
    condition(graph, feat) has run, on the given fake edges (node ids, one per real edge), from one
    stag_contrastive_nll launch.  contrastive_why_not(q_a, graph, feat) says when it applies."""
    why = contrastive_why_not(q_a, graph, feat)
    if why is not None and why != "switch":
        raise ValueError(f"contrastive_nll does not apply: {why}")
    P, wh, bh = q_a._narrow_tables(feat)
    par = q_a.new_parameters
    return _ContrastiveNll.apply(par["loc"], par["log_scale"], P, wh, bh, fake_src.to(torch.int32).contiguous(),
                                 fake_dst.to(torch.int32).contiguous())


def _bwd_w_raw(csrv, x, g, D, src_scale, broadcast_x=False, spec=None, reduce_k=False, both=False,
               seg_len=DEFAULT_SEG_LEN):
    """stag_agg_bwd_w over the plan's units.  both=True: (d/dp0, d/dp1) of a Normal | Uniform spec
    from one pass; else the single tensor selected by spec.deriv (or the plain dw)."""
    dev = _lib.require_device(x, g)
    cols = 1 if reduce_k else D
    dw = torch.empty((csrv.n_edges, cols), dtype=torch.float32, device=dev)
    dw1 = torch.empty_like(dw) if both else None
    plan_c, _keep = _plan_struct(csrv, seg_len, 1, 0, dev)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_bwd_w(C.byref(cs), C.byref(plan_c) if plan_c is not None else None,
                                       _lib.ptr(x), 0 if broadcast_x else x.stride(0),
                                       _lib.ptr(g), g.stride(0), D, _lib.ptr(src_scale),
                                       C.byref(spec) if spec is not None else None, int(reduce_k),
                                       _lib.ptr(dw), _lib.ptr(dw1), cols, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd_w")
    return (dw, dw1) if both else dw


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, graph, noise, reduce, src_scale, dst_scale, seg_len, broadcast_x):
        if half_rows_ok(x, w, noise, broadcast_x, graph):
            # fp16 / bf16 rows as they are (stag_agg_fwd_half).  The backward is the fp32 launch on csr_t below: grad_out
            # is fp32, autograd casts dx to x.dtype, and nothing half-typed is saved
            D = x.shape[1]
            out = _agg_half_raw(graph.csr, x, D, _noise_spec(noise) if noise is not None else _none_spec(), reduce,
                                src_scale, dst_scale, seg_len)
            ctx.graph, ctx.noise, ctx.reduce, ctx.seg_len = _owner(graph), noise, reduce, seg_len
            ctx.broadcast_x, ctx.D = False, D
            ctx.save_for_backward(None, None, src_scale, dst_scale, None)
            return out
        x = _f32c(x)
        D = x.shape[1]
        csrv = graph.csr
        if noise is not None:
            spec = _noise_spec(noise)  # ctx.noise keeps the parameter tensors alive
        elif w is not None:
            w = _f32c(w)
            spec = _explicit_spec(w)
        else:
            spec = _none_spec()
        # the in-norm factor is only kept (one more [N, D] store) when a backward can follow
        want_ns = _spec_in_norm(spec) and any(ctx.needs_input_grad[:2])
        out, ns = _agg_raw(csrv, x, D, spec, reduce, src_scale, dst_scale, seg_len,
                           want_norm_scale=want_ns, broadcast_x=broadcast_x)
        ctx.graph, ctx.noise, ctx.reduce, ctx.seg_len = _owner(graph), noise, reduce, seg_len
        ctx.broadcast_x = broadcast_x
        ctx.D = D
        need_x = w is not None and ctx.needs_input_grad[1]   # x is only read by dw
        ctx.save_for_backward(x if need_x else None, w, src_scale, dst_scale, ns)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, w, src_scale, dst_scale, ns = ctx.saved_tensors
        graph, noise = ctx.graph, ctx.noise
        D = ctx.D
        g = _f32c(grad_out)
        if ns is not None:                      # in-norm factor is a constant of the backward
            g = g * ns
        dvec = dst_scale
        if ctx.reduce == _lib.REDUCE_MEAN:
            inv = 1.0 / graph.csr.degrees.clamp(min=1).to(torch.float32)
            dvec = inv if dvec is None else dvec * inv
        dx = dw = None
        if ctx.needs_input_grad[0] and not ctx.broadcast_x:
            if noise is not None:
                spec = _noise_spec(noise, in_norm=0)
            elif w is not None:
                spec = _explicit_spec(w)
            else:
                spec = _none_spec()
            # dx[u,:] = ss[u] * sum_{p: src_p = u} w[p,:] * dvec[v_p] * g[v_p,:]
            dx, _ = _agg_raw(graph.csr_t, g, D, spec, _lib.REDUCE_SUM, dvec, src_scale, ctx.seg_len)
        if w is not None and ctx.needs_input_grad[1]:
            gg = g if dvec is None else g * dvec.unsqueeze(1)
            dw = _bwd_w_raw(graph.csr, x, gg.contiguous(), D, src_scale, broadcast_x=ctx.broadcast_x,
                            seg_len=ctx.seg_len)
        return dx, dw, None, None, None, None, None, None, None


class _AggregateVI(torch.autograd.Function):
    """Fused aggregation whose noise parameters carry gradients (`vi=True`, reparameterised
    draw w = p0 + p1 * z | low + (high-low) u; stag/layers.py:123-124).  Nothing [E, D]-sized
    is saved: the backward (stag_agg_bwd) redraws z from the counters and returns dx together with
    the two parameter-derivative aggregates from one pass."""

    @staticmethod
    def forward(ctx, x, p0, p1, graph, noise, reduce, src_scale, dst_scale, seg_len):
        x = _f32c(x)
        D = x.shape[1]
        spec = _noise_spec(noise)
        out, ns = _agg_raw(graph.csr, x, D, spec, reduce, src_scale, dst_scale, seg_len,
                           want_norm_scale=_spec_in_norm(spec))
        ctx.graph, ctx.noise, ctx.reduce, ctx.seg_len, ctx.D = _owner(graph), noise, reduce, seg_len, D
        ctx.shapes = (p0.shape, p1.shape)
        # in-norm (stag/layers.py:8-36) is differentiated too: its factor s = indeg / sum_in(w) and the
        # output are kept ([N, D] each; nothing [E, D]-sized)
        ctx.save_for_backward(x, src_scale, dst_scale, ns, out if ns is not None else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, src_scale, dst_scale, ns, out = ctx.saved_tensors
        graph, noise, D = ctx.graph, ctx.noise, ctx.D
        g = _f32c(grad_out)
        dvec = dst_scale
        if ctx.reduce == _lib.REDUCE_MEAN:
            inv = 1.0 / graph.csr.degrees.clamp(min=1).to(torch.float32)
            dvec = inv if dvec is None else dvec * inv
        spec = _noise_spec(noise, in_norm=0)     # the backward redraws the RAW weights; the factor rides in g
        spec_c = spec if not isinstance(spec, tuple) else _targs_to_ctypes(spec)   # stag_agg_bwd_w goes through ctypes
        q = None
        if ns is not None:
            # out = dv * s * A, A = sum_e w x', s = indeg / W, W = sum_e w  =>  with g' = g * s (dv applied by
            # the kernel):  dL/dw[e,k] = dv g'[v,k] (x'[u,k] - A/W),  A/W = out / (dv * indeg).
            # The x' part is the usual pass with g'; the other part is the same aggregate of dw/dp with
            #   q[v,k] = dv g' A/W = g[v,k] s[v,k] out[v,k] / indeg[v]   in the place of g and no x.
            deg = graph.csr.degrees.clamp(min=1).to(torch.float32).unsqueeze(1)
            q = (g * ns * out / deg).contiguous()
            g = (g * ns).contiguous()
        dx = dp0 = dp1 = None
        per_edge = noise.param_mode >= _lib.PARAM_PER_EDGE1
        need_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not per_edge and need_p and _AGG_BWD_DP_ONE_PASS:
            # scalar / per-channel parameters: ONE transposed pass yields dx AND the finished gradients
            #   dp_i[k] = sum_e dw/dp_i[e,k] dv g'[v,k] s_u x[u,k]   (x[u] is the unit's own row there)
            dx, c0, c1 = _agg_bwd_dp_raw(graph.csr_t, g, x, D, spec, dvec, src_scale, ctx.seg_len,
                                         want_dx=ctx.needs_input_grad[0])
            if q is not None:       # in-norm: minus sum_e dw/dp_i[e,k] q[v,k], the same pass over q without x
                _, n0, n1 = _agg_bwd_dp_raw(graph.csr_t, q, None, D, spec, None, None, ctx.seg_len, want_dx=False)
                c0, c1 = c0 - n0, c1 - n1
            rows = {1: c0, 2: c1}
        elif not per_edge:
            # the two-step form: the two derivative aggregates T_i[u,k] = ss[u] sum_p dw/dp_i[p,k] g'[v_p,k], then
            # dp_i[k] = sum_u x[u,k] T_i[u,k]   (sum_e D[e,k] s_u x[u,k] g'[v,k] regrouped by u)
            dx, t0, t1 = _agg_bwd_raw(graph.csr_t, g, D, spec, dvec, src_scale, ctx.seg_len, need_p)
            if not ctx.needs_input_grad[0]:
                dx = None
            if need_p:      # dp_i[k] = sum_u x[u,k] T_i[u,k], both in one pass over x
                c0, c1 = coldot(x, t0, t1)
                if q is not None:   # in-norm: minus sum_e dw/dp_i[e,k] q[v,k], the same pass over q
                    _, n0, n1 = _agg_bwd_raw(graph.csr_t, q, D, spec, None, None, ctx.seg_len, True)
                    c0, c1 = c0 - n0.sum(0), c1 - n1.sum(0)
                rows = {1: c0, 2: c1}
        elif need_p and q is None and noise.param_mode == _lib.PARAM_PER_EDGE1 and D <= 256:
            # [E, 1] (amortised) parameters: dx and both per-edge gradients from ONE transposed pass — the
            # row of x an edge's gradient needs is the unit's own row there
            dx, e0, e1 = _agg_bwd_edge_raw(graph.csr_t, g, x, D, spec_c, dvec, src_scale, ctx.seg_len,
                                           want_dx=ctx.needs_input_grad[0])
            rows = {1: e0, 2: e1}
            need_p = False
        elif (need_p and q is None and noise.param_mode == _lib.PARAM_PER_EDGE
              and pedge_bwd_why_not(x, noise, graph, ctx.needs_input_grad[0]) is None):
            # [E, D] (amortised) parameters: dx and both gradient tables from ONE transposed pass (stag_agg_bwd_pedge);
            # dvec rides along as g_scale, so no [N, D] product is formed
            dx, e0, e1 = _agg_bwd_pedge_raw(graph.csr_t, g, x, D, spec_c, dvec, src_scale, ctx.seg_len,
                                            want_p1=ctx.needs_input_grad[2])
            rows = {1: e0, 2: e1}
            need_p = False
        elif ctx.needs_input_grad[0]:
            dx, _, _ = _agg_bwd_raw(graph.csr_t, g, D, spec, dvec, src_scale, ctx.seg_len, False)
        if per_edge and need_p:
            # per-edge (amortised) parameters: both derivatives from ONE pass over the edges
            gg = (g if dvec is None else g * dvec.unsqueeze(1)).contiguous()
            rk = noise.param_mode == _lib.PARAM_PER_EDGE1
            e0, e1 = _bwd_w_raw(graph.csr, x, gg, D, src_scale, spec=spec_c, reduce_k=rk, both=True,
                                seg_len=ctx.seg_len)
            if q is not None:
                ones = torch.ones(D, dtype=torch.float32, device=q.device)
                m0, m1 = _bwd_w_raw(graph.csr, ones, q, D, None, broadcast_x=True, spec=spec_c, reduce_k=rk,
                                    both=True, seg_len=ctx.seg_len)
                e0, e1 = e0 - m0, e1 - m1
            rows = {1: e0, 2: e1}
        for which, need in ((1, ctx.needs_input_grad[1]), (2, ctx.needs_input_grad[2])):
            if not need:
                continue
            d = rows[which]
            shape = ctx.shapes[which - 1]
            d = d.sum_to_size(shape) if d.dim() >= len(shape) and shape != d.shape else d.reshape(shape)
            if which == 1:
                dp0 = d
            else:
                dp1 = d
        return dx, dp0, dp1, None, None, None, None, None, None


# ---- constant inputs of a width that is not a multiple of 4 (PPI's 50 input features: BASELINE configs[2], layer 1) ------
# With D % 4 != 0 the kernels take their scalar row forms (4 bounds-checked stores per lane, more registers: 83 against 79
# VGPRs at 16 lanes per row = 5 against 6 waves per SIMD).  A tensor that is a CONSTANT of the run — it carries no gradient
# and the same object comes back unchanged, as dataset features do on every epoch — is zero-padded to the next multiple
# of 4 ONCE (on its second sighting: a fresh tensor per step, e.g. a freshly batched minibatch's features, would pay the
# copy the vector forms save — measured in round 1) and the launch runs at the padded width: the first D channels of the
# result are the same bits (a Philox block covers 4 channels either way; the padded channels gather zeros), returned as a
# view [:, :D] of the padded result, which the dense transform behind it reads through its row stride (node_linear).
PAD_CONSTANT_INPUTS = True
PAD_MIN_WIDTH = 32        # narrower rows (molhiv's 9 atom features) are launch-bound: the slice of the padded result and the
                          # second descriptor cost the host more than the vector forms save the kernel (D = 9: 13 -> 24 us)
_const_pads = {}          # id(tensor) -> [weakref, _version, data_ptr, sightings, padded | None]


def _padded_constant(x):
    """The cached zero-padded copy [N, ceil4(D)] of a constant x [N, D], or None (first sighting, or it changed)."""
    import weakref
    key = id(x)
    ent = _const_pads.get(key)
    if ent is None or ent[0]() is not x or ent[1] != x._version or ent[2] != x.data_ptr():
        if len(_const_pads) >= 64:
            _const_pads.clear()
        _const_pads[key] = [weakref.ref(x, lambda _r, key=key: _const_pads.pop(key, None)), x._version, x.data_ptr(), 1, None]
        return None
    ent[3] += 1
    if ent[4] is None:
        D = x.shape[1]
        Dp = (D + 3) // 4 * 4
        xp = torch.zeros((x.shape[0], Dp), dtype=torch.float32, device=x.device)
        xp[:, :D].copy_(x)
        ent[4] = xp
    return ent[4]


_row_pads = {}            # id(row) -> (weakref, _version, {Dp: padded row})


def _padded_noise(noise, Dp):
    """The descriptor for a launch at the padded width: scalar parameters as they are; per-channel rows [D] extended to
    [Dp] with their last entry (the padded channels' draws are multiplied by zeros), kept per row tensor — the rows a
    layer hands over come from noise._expanded's own cache, so this costs nothing from the second call on.  None when
    the descriptor has per-edge parameters (the plain path then)."""
    if noise is None or noise.param_mode == _lib.PARAM_SCALAR:
        return noise
    if noise.param_mode != _lib.PARAM_PER_CHANNEL:
        return None
    import copy
    import weakref
    out = copy.copy(noise)
    out.dn = Dp
    for name in ("p0", "p1"):
        row = getattr(noise, name)
        if row is None:
            continue
        ent = _row_pads.get(id(row))
        if ent is None or ent[0]() is not row or ent[1] != row._version:
            if len(_row_pads) > 256:
                _row_pads.clear()
            ent = _row_pads[id(row)] = (weakref.ref(row, lambda _r, k=id(row): _row_pads.pop(k, None)), row._version, {})
        pad = ent[2].get(Dp)
        if pad is None:
            pad = ent[2][Dp] = torch.cat([row, row[-1:].expand(Dp - row.shape[0])]).contiguous()
        setattr(out, name, pad)
    return out


def aggregate_into(csrv, x, out, weight, reduce, src_scale, dst_scale, plan_t):
    """The rows of ONE sub-plan of csrv (CsrView.subplan) written into `out` [n_dst, D]; no autograd.
    How a node-range shard launches its local-source rows while the halo exchange is in flight and
    the other rows behind it (partition.GraphShard.aggregate); every row is reduced exactly as
    a whole-plan launch would reduce it."""
    x = _f32c(x)
    if weight is None:
        spec = _none_spec()
    elif isinstance(weight, EdgeNoise):
        if weight.dn != x.shape[1]:
            raise ValueError(f"noise width {weight.dn} != feature width {x.shape[1]}")
        spec = _noise_spec(weight)
    else:
        raise TypeError("aggregate_into takes None or an EdgeNoise")
    _agg_raw(csrv, x, x.shape[1], spec, _REDUCE[reduce], _f32c(src_scale), _f32c(dst_scale),
             plan_t["seg_len"], out=out, plan_t=plan_t)
    return out


# ---- one weight per edge, shared by all channels (base_layer.sample_dimension = 1; an explicit [E] / [E, 1] weight) --------
# stag_agg_fwd_w1 (one launch: the weight is drawn by one lane per edge and a row whose weight is exactly 0 is NOT READ) |
# the two-launch route on the older kernels: EdgeNoise.materialize() at width 1, then stag_agg_fwd with EXPLICIT weights and
# spec.group = D (the form GAT's d ft uses), the same on csr_t for dx.  The two-launch route MULTIPLIES by a zero weight
# where the fused launch skips the row: on finite x the two agree to rounding, on a non-finite row whose edges are all
# dropped the fused launch gives 0 and the two-launch route NaN.
# False, by the usual rule — True only if the new launch is not slower than the route beside it, beyond the spread of two
# repeats, for EVERY kind timed — because EXPLICIT weights miss it (profiles/r15/edge_weight.txt; us per call, fused against
# two-launch, arxiv shape D = 128 | PPI batch D = 256; two repeats of the two-launch route differ by 0.1-0.6):
#   Normal 113.9 / 178.9 | 126.7 / 172.9     Uniform 113.9 / 176.8 | 127.1 / 171.4     Bernoulli 0.9: 107.0 / 176.6 | 118.3 / 171.0
#   Bernoulli 0.5: 79.1 / 176.4 | 74.9 / 170.2     Bernoulli 0.1: 62.2 / 174.7 | 50.5 / 170.0     EXPLICIT 130.8 / 119.0 | 139.3 / 116.3
# Every drawn kind wins 44-120 us (no materialise launch, one Philox block per edge, dropped rows not gathered: Bernoulli(0.5)
# runs below the 94.4 us of the launch without noise).  Dense explicit weights lose 12-23 us: a weight has to arrive
# (eid, then w[eid]) before its row may be requested, where stag_agg_fwd requests the row and the weight together.
# (The expanded [E, D] copy this replaces for tensors: 375.7 | 484.5 us.)  The skip itself costs nothing where nothing is
# dropped: the same kernel built with -DSTAG_W1_NO_SKIP=1 reads 113.1 against 113.9 (Normal), 130.7 against 130.8 (EXPLICIT).
EDGE_WEIGHT_FUSED = False
EDGE_WEIGHT_TENSORS = True    # an explicit [E] / [E, 1] tensor takes the width-1 routes | is expanded to [E, D] first (A/B)


def edge_weight_why_not(x, weight, graph, broadcast_x):
    """The first reason ops.aggregate does not hand this call — x [N, D] with a weight of width 1: an EdgeNoise with
    dn = 1, or a tensor [E] / [E, 1] — to stag_agg_fwd_w1 as it is, or None.  One clause per refusal of the entry point
    (include/stag_hip.h) and per path without a form there.  A descriptor with in-norm or live parameters is
    materialised first ([E, 1], differentiable) and asked about again as a tensor; everything else that gets a reason
    takes the two-launch route (see EDGE_WEIGHT_FUSED)."""
    if not EDGE_WEIGHT_FUSED:
        return "switch"
    if x.dim() != 2:
        return "shape"
    if broadcast_x or x.stride(0) == 0:
        return "broadcast row"
    if x.dtype != torch.float32:
        return "dtype"
    noise = weight if isinstance(weight, EdgeNoise) else None
    if noise is not None:
        if noise.dn != 1:
            return "noise width"
        if noise.kind < _lib.NOISE_NORMAL or noise.param_mode == _lib.PARAM_PER_EDGE:
            return "noise parameters"
        if noise.in_norm:
            return "in-norm"
        if noise.deriv:
            return "derivative selector"
        if noise.chunk_base:
            return "channel shard"
        if noise.n_samples != 1:
            return "monte-carlo"
        if noise.grad_params is not None and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params):
            return "parameter gradients"
        if (noise.pos_base & 0xFFFFFFFF) + noise.graph.number_of_edges() > (1 << 32):
            return "position range"
    elif torch.is_tensor(weight):
        if weight.dim() not in (1, 2) or (weight.dim() == 2 and weight.shape[1] != 1):
            return "weight width"
    else:
        return "no weight"
    if getattr(graph, "is_shard", False) or (noise is not None and getattr(noise.graph, "is_shard", False)):
        return "shard"
    if torch.compiler.is_compiling():
        return "compiling"
    if not x.is_cuda or (torch.is_tensor(weight) and not weight.is_cuda):
        return "device"
    return None


def _w1_forward(csrv, x, D, noise, w1, fused, reduce, src_scale, dst_scale, seg_len, broadcast_x=False):
    """One width-1 aggregation on csrv (csr: the forward; csr_t: dx): the fused launch on the descriptor or on explicit
    w[E], or stag_agg_fwd on explicit [E, 1] weights with group = D (w1: the materialised weights of a descriptor)."""
    if fused:
        spec = _noise_spec(noise) if noise is not None else _explicit_spec(w1)
        return _agg_w1_raw(csrv, x, D, spec, reduce, src_scale, dst_scale, seg_len)
    return _agg_raw(csrv, x, D, _explicit_spec(w1, group=D), reduce, src_scale, dst_scale, seg_len,
                    broadcast_x=broadcast_x)[0]


class _AggregateW1(torch.autograd.Function):
    """aggregate with one weight per edge under autograd: x and / or an explicit w [E, 1] carry gradients (a descriptor's
    parameters do not: live ones arrive materialised).  dx is the forward's launch on csr_t with g (the fused launch
    redraws the weights from the counters: nothing is saved); dw [E, 1] is stag_agg_bwd_w summed over the channels.
    Nothing [E, D]-sized exists on either route."""

    @staticmethod
    def forward(ctx, x, w, graph, noise, reduce, src_scale, dst_scale, seg_len, broadcast_x):
        fused = edge_weight_why_not(x, noise if noise is not None else w, graph, broadcast_x) is None
        x = _f32c(x)
        D = x.shape[1]
        w1 = _f32c(w) if w is not None else (None if fused else noise.materialize())
        out = _w1_forward(graph.csr, x, D, noise, w1, fused, reduce, src_scale, dst_scale, seg_len, broadcast_x)
        ctx.graph, ctx.noise, ctx.reduce, ctx.seg_len = _owner(graph), noise, reduce, seg_len
        ctx.broadcast_x, ctx.D, ctx.fused = broadcast_x, D, fused
        need_x = w is not None and ctx.needs_input_grad[1]   # x is only read by dw
        ctx.save_for_backward(x if need_x else None, w1, src_scale, dst_scale)     # (w1: E floats, or None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, w1, src_scale, dst_scale = ctx.saved_tensors
        graph, D = ctx.graph, ctx.D
        g = _f32c(grad_out)
        dvec = dst_scale
        if ctx.reduce == _lib.REDUCE_MEAN:
            inv = 1.0 / graph.csr.degrees.clamp(min=1).to(torch.float32)
            dvec = inv if dvec is None else dvec * inv
        dx = dw = None
        if ctx.needs_input_grad[0] and not ctx.broadcast_x:
            # dx[u,:] = ss[u] * sum_{p: src_p = u} w1[p] * dvec[v_p] * g[v_p,:]
            dx = _w1_forward(graph.csr_t, g, D, ctx.noise, w1, ctx.fused, _lib.REDUCE_SUM, dvec, src_scale, ctx.seg_len)
        if ctx.needs_input_grad[1]:
            gg = g if dvec is None else g * dvec.unsqueeze(1)
            dw = _bwd_w_raw(graph.csr, x, gg.contiguous(), D, src_scale, broadcast_x=ctx.broadcast_x, reduce_k=True,
                            seg_len=ctx.seg_len)
        return dx, dw, None, None, None, None, None, None, None


def _aggregate_w1(graph, x, noise, w, reduce, src_scale, dst_scale, seg_len, broadcast_x):
    """ops.aggregate with a weight of width 1 on rows of width D > 1 (noise: an EdgeNoise with dn = 1 | w: [E, 1])."""
    if noise is not None:
        if noise.n_samples > 1:
            raise ValueError("Monte-Carlo batching does not apply to a noise width of 1: loop over the samples")
        live = (noise.grad_params is not None and torch.is_grad_enabled()
                and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params))
        if live or noise.in_norm:
            # [E, 1]: the reparameterised sample (autograd reaches loc / log_scale through it), in-norm applied
            w, noise = noise.materialize(), None
    src_scale, dst_scale = _f32c(src_scale), _f32c(dst_scale)
    if torch.is_grad_enabled() and (x.requires_grad or (w is not None and w.requires_grad)):
        return _AggregateW1.apply(x, w, graph, noise, _REDUCE[reduce], src_scale, dst_scale, seg_len, broadcast_x)
    fused = edge_weight_why_not(x, noise if noise is not None else w, graph, broadcast_x) is None
    x = _f32c(x)
    w1 = _f32c(w) if w is not None else (None if fused else noise.materialize())
    return _w1_forward(graph.csr, x, x.shape[1], noise, w1, fused, _REDUCE[reduce], src_scale, dst_scale, seg_len,
                       broadcast_x)


def aggregate(graph, x, weight=None, reduce="sum", src_scale=None, dst_scale=None,
              seg_len=DEFAULT_SEG_LEN, _broadcast_x=False, _gathered=False):
    """out[v,:] = dscale[v] * sum|mean_{e=(u->v)} w[e,:] * sscale[u] * x[u,:]

    weight: None (plain copy_u), a tensor [E, D] indexed by edge id (explicit
    `edge_weight`, stag/zoo/gcn.py:60-63), or an EdgeNoise (fused sampling).  A tensor [E] / [E, 1] or an
    EdgeNoise of width 1 is one weight per edge shared by all channels (edge_weight_why_not): no [E, D] tensor.
    On a node-range shard (partition.GraphShard) x holds this rank's rows and the call includes
    the halo exchange."""
    if x.dim() != 2:
        raise ValueError("aggregate expects x of shape [N, D]")
    if getattr(graph, "is_shard", False) and not _gathered and not _broadcast_x:
        # (a source-side scale indexes COLUMNS: on a shard, the rows of the exchanged buffer — shard.out_degrees())
        return graph.aggregate(x, weight, reduce=reduce, src_scale_buf=src_scale,
                               dst_scale_local=dst_scale, seg_len=seg_len)
    noise = weight if isinstance(weight, EdgeNoise) else None
    w = weight if torch.is_tensor(weight) else None
    D = x.shape[1]
    if w is not None:
        if w.shape[0] != graph.number_of_edges():
            raise AssertionError("edge_weight.shape[0] != number_of_edges")   # zoo/gcn.py:61
        if w.dim() == 1:
            w = w.unsqueeze(1)
        if w.shape[1] != D:
            if w.dim() == 2 and w.shape[1] == 1 and EDGE_WEIGHT_TENSORS:      # one weight per edge: no [E, D] copy
                return _aggregate_w1(graph, x, None, w, reduce, src_scale, dst_scale, seg_len, _broadcast_x)
            w = w.expand(w.shape[0], D)
    if noise is not None and noise.dn != D:
        if noise.dn == 1:          # base_layer.sample_dimension = 1: one weight per edge, shared by all channels
            return _aggregate_w1(graph, x, noise, None, reduce, src_scale, dst_scale, seg_len, _broadcast_x)
        raise ValueError(f"noise width {noise.dn} != feature width {D}")
    if noise is not None and noise.n_samples > 1:
        if _broadcast_x:
            raise ValueError("Monte-Carlo batching does not apply to a broadcast row")
        import copy
        one = copy.copy(noise)
        one.n_samples = 1
        return aggregate_mc(graph, x, one, noise.n_samples, noise.offset_stride, reduce=reduce,
                            src_scale=src_scale, dst_scale=dst_scale, seg_len=seg_len, _gathered=_gathered)
    if noise is not None and noise.grad_params is not None and torch.is_grad_enabled():
        p0, p1 = (torch.as_tensor(p, dtype=torch.float32, device=x.device) for p in noise.grad_params)
        if p0.requires_grad or p1.requires_grad:
            return _AggregateVI.apply(x, p0, p1, graph, noise, _REDUCE[reduce], _f32c(src_scale),
                                      _f32c(dst_scale), seg_len)
    if not (torch.is_grad_enabled() and (x.requires_grad or (w is not None and w.requires_grad))):
        # nothing to differentiate: straight to the library (no autograd node; host time of a call matters on
        # launch-bound graphs)
        if half_rows_ok(x, w, noise, _broadcast_x, graph):     # fp16 / bf16 rows as they are: no widened copy
            return _agg_half_raw(graph.csr, x, D, _noise_spec(noise) if noise is not None else _none_spec(),
                                 _REDUCE[reduce], _f32c(src_scale), _f32c(dst_scale), seg_len)
        xin, x = x, _f32c(x)
        if (PAD_CONSTANT_INPUTS and D % 4 and D >= PAD_MIN_WIDTH and w is None and not _broadcast_x and x is xin and x.is_cuda
                and not x.requires_grad and (noise is None or noise.param_mode <= _lib.PARAM_PER_CHANNEL)):
            xp = _padded_constant(x)
            noise_p = _padded_noise(noise, (D + 3) // 4 * 4) if xp is not None else None
            if xp is not None and (noise is None or noise_p is not None):
                spec_p = _noise_spec(noise_p) if noise_p is not None else _none_spec()
                return _agg_raw(graph.csr, xp, xp.shape[1], spec_p, _REDUCE[reduce], _f32c(src_scale), _f32c(dst_scale),
                                seg_len)[0][:, :D]
        if noise is not None:
            spec = _noise_spec(noise)
        elif w is not None:
            spec = _explicit_spec(_f32c(w))
        else:
            spec = _none_spec()
        return _agg_raw(graph.csr, x, D, spec, _REDUCE[reduce], _f32c(src_scale), _f32c(dst_scale), seg_len,
                        broadcast_x=_broadcast_x)[0]
    return _Aggregate.apply(x, w, graph, noise, _REDUCE[reduce], _f32c(src_scale),
                            _f32c(dst_scale), seg_len, _broadcast_x)


# ---- the max reducer (DGL's fn.max; GraphSAGE 'pool', stag/zoo/graph_sage.py:90-93) --------------------------------
FUSED_MAX = True          # stag_agg_max_fwd / _bwd | the composed route (messages formed, scatter-amax): tests compare both
# stag_agg_fwd_half on fp16 / bf16 rows | x.float() + stag_agg_fwd.  True because, at the arxiv shape (D = 128, bf16 rows,
# us per call, profiles/r07/half_rows.txt), it is not slower than the cast route for any kind — none 68.8 against 117.4,
# Bernoulli 106.7 / 118.1, Uniform 102.5 / 118.6, Normal 115.5 / 117.8; two repeats of the cast route differ by 0.4-0.7.
# (On the L2-resident PPI batch at D = 256 the drawn kinds lose 12-13 us to the cast route's XCD-aware walk: DESIGN.md 4.5, 5.)
HALF_ROWS = True


def half_rows_why_not(x, w, noise, broadcast_x, graph=None):
    """The first reason ops.aggregate keeps the cast route (x.float(), stag_agg_fwd) for this call, or None: the launch
    goes to stag_agg_fwd_half on x as it is.  One clause per refusal of the entry point (include/stag_hip.h) and per
    path that has no half form (Monte-Carlo batches, parameter gradients, shards, a traced graph)."""
    if not HALF_ROWS:
        return "switch"
    if x.dtype not in _HALF_DTYPES:
        return "dtype"
    if broadcast_x:
        return "broadcast row"
    if w is not None:
        return "explicit weights"
    if x.dim() != 2 or x.shape[1] % 8 != 0:
        return "width"
    if x.stride(1) != 1 or x.stride(0) % 8 != 0 or x.stride(0) == 0:
        return "strides"
    if noise is not None:
        if noise.kind < _lib.NOISE_NORMAL or noise.param_mode > _lib.PARAM_PER_CHANNEL:
            return "noise parameters"
        if noise.in_norm:
            return "in-norm"
        if noise.p1_log or noise.deriv:
            return "log-scale"
        if noise.n_samples != 1:
            return "monte-carlo"
        if noise.grad_params is not None and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params):
            return "parameter gradients"
    if getattr(graph, "is_shard", False) or (noise is not None and getattr(noise.graph, "is_shard", False)):
        return "shard"
    if torch.compiler.is_compiling():
        return "compiling"
    if not x.is_cuda:
        return "device"
    if x.data_ptr() % 16 != 0:
        return "alignment"
    return None


def half_rows_ok(x, w, noise, broadcast_x, graph=None):
    return half_rows_why_not(x, w, noise, broadcast_x, graph) is None


def _max_fwd_raw(csrv, x, D, spec, seg_len, want_cnt, broadcast_x=False):
    """One stag_agg_max_fwd on csrv: (out [n_dst, D], cnt [n_dst, D] int32 or None)."""
    dev = _lib.require_device(x, csrv.indptr)
    drawn = (spec[0][0] if isinstance(spec, tuple) else spec.kind) >= _lib.NOISE_NORMAL
    plan_t = csrv.plan(seg_len)
    if isinstance(spec, tuple):
        out, cnt = torch.ops.stag.agg_max_fwd(*csrv.torch_args(), *_plan_args(csrv, plan_t, (D + 255) // 256, dev, width=D,
                                                                               drawn=drawn, share=D),
                                              x, broadcast_x, *spec, bool(want_cnt))
        return out, (cnt if want_cnt else None)
    out = torch.empty((csrv.n_dst, D), dtype=torch.float32, device=dev)
    cnt = torch.empty((csrv.n_dst, D), dtype=torch.int32, device=dev) if want_cnt else None
    if csrv.n_dst == 0:
        return out, cnt
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], 2 * D, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv, seg_len, (D + 255) // 256, nbytes, dev, plan_t, width=D, drawn=drawn, share=D)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_max_fwd(C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x),
                                         0 if broadcast_x else x.stride(0), D, C.byref(spec), _lib.ptr(out), D,
                                         _lib.ptr(cnt), D, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_max_fwd")
    return out, cnt


def _max_bwd_raw(csrv_t, x, out, cnt, g, D, spec, seg_len, want_dx, want_dw, want_dp, broadcast_x=False):
    """One stag_agg_max_bwd on the source-major CSR: (dx, dw, dp0_rows, dp1_rows), None where not wanted."""
    dev = _lib.require_device(x, out, g, csrv_t.indptr)
    drawn = (spec[0][0] if isinstance(spec, tuple) else spec.kind) >= _lib.NOISE_NORMAL
    plan_t = csrv_t.plan(seg_len)
    if isinstance(spec, tuple):
        dx, dw, t0, t1 = torch.ops.stag.agg_max_bwd(
            *csrv_t.torch_args(), *_plan_args(csrv_t, plan_t, (D + 255) // 256, dev, width=D, drawn=drawn), x, broadcast_x,
            out, cnt, g, *spec, bool(want_dx), bool(want_dw), bool(want_dp))
        return (dx if want_dx else None), (dw if want_dw else None), (t0 if want_dp else None), (t1 if want_dp else None)
    n = csrv_t.n_dst
    dx = torch.empty((n, D), dtype=torch.float32, device=dev) if want_dx else None
    dw = torch.empty((csrv_t.n_edges, D), dtype=torch.float32, device=dev) if want_dw else None
    t0 = torch.empty((n, D), dtype=torch.float32, device=dev) if want_dp else None
    t1 = torch.empty((n, D), dtype=torch.float32, device=dev) if want_dp else None
    if n == 0:
        return dx, dw, t0, t1
    nbytes = (_lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], (3 if want_dp else 1) * D, 0)
              if plan_t is not None else 0)
    plan_c, _keep = _plan_struct(csrv_t, seg_len, (D + 255) // 256, nbytes, dev, plan_t, width=D, drawn=drawn)
    sbytes = _lib.lib().stag_agg_max_bwd_scratch_bytes(csrv_t.n_src, D)
    scratch = torch.empty(sbytes // 4 + 4, dtype=torch.float32, device=dev)
    cs = csrv_t.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_max_bwd(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x), 0 if broadcast_x else x.stride(0),
            _lib.ptr(out), _lib.ptr(cnt), _lib.ptr(g), D, D, C.byref(spec), _lib.ptr(dx), _lib.ptr(dw), D,
            _lib.ptr(t0), _lib.ptr(t1), D, _lib.ptr(scratch), sbytes, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_max_bwd")
    return dx, dw, t0, t1


class _AggregateMax(torch.autograd.Function):
    """out[v,:] = max over the in-edges of w[e,:] * x[u,:] in one pass (stag_agg_max_fwd); nothing [E, D]-sized is
    formed or saved.  The backward (stag_agg_max_bwd) walks the source-major CSR, redraws w from its counters and sends
    g / cnt to every message equal to the maximum; dx, dw (explicit weights) and the parameter gradients of a live
    Normal / Uniform draw (vi=True; scalar | per-channel) come from that one pass, the latter finished by coldot."""

    @staticmethod
    def forward(ctx, x, w, p0, p1, graph, noise, seg_len, broadcast_x):
        x = _f32c(x)
        D = x.numel() if broadcast_x else x.shape[1]
        if noise is not None:
            spec = _noise_spec(noise)
        elif w is not None:
            w = _f32c(w)
            spec = _explicit_spec(w)
        else:
            spec = _none_spec()
        out, cnt = _max_fwd_raw(graph.csr, x, D, spec, seg_len, True, broadcast_x)
        ctx.graph, ctx.noise, ctx.seg_len, ctx.broadcast_x, ctx.D = _owner(graph), noise, seg_len, broadcast_x, D
        ctx.shapes = (None if p0 is None else p0.shape, None if p1 is None else p1.shape)
        ctx.save_for_backward(x, w, out, cnt)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, w, out, cnt = ctx.saved_tensors
        graph, noise, D = ctx.graph, ctx.noise, ctx.D
        want_dx = ctx.needs_input_grad[0] and not ctx.broadcast_x
        want_dw = w is not None and ctx.needs_input_grad[1]
        want_dp = noise is not None and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        if not (want_dx or want_dw or want_dp):
            return None, None, None, None, None, None, None, None
        spec = _noise_spec(noise) if noise is not None else (_explicit_spec(w) if w is not None else _none_spec())
        dx, dw, t0, t1 = _max_bwd_raw(graph.csr_t, x, out, cnt, _f32c(grad_out), D, spec, ctx.seg_len, want_dx, want_dw,
                                      want_dp, ctx.broadcast_x)
        dp = [None, None]
        if want_dp:
            xs = x if not ctx.broadcast_x else x.reshape(1, D).expand(t0.shape[0], D).contiguous()
            c0, c1 = coldot(xs, t0, t1)
            for i, (d, shape) in enumerate(((c0, ctx.shapes[0]), (c1, ctx.shapes[1]))):
                if ctx.needs_input_grad[2 + i]:
                    dp[i] = d.sum_to_size(shape) if d.dim() >= len(shape) and shape != d.shape else d.reshape(shape)
        return dx, dw, dp[0], dp[1], None, None, None, None


def _max_fused_route(graph, x, noise, w, grad):
    """Whether aggregate_max takes stag_agg_max_fwd / _bwd (see aggregate_max)."""
    if not FUSED_MAX or not x.is_cuda or getattr(graph, "is_shard", False):
        return False
    if w is not None and not w.is_cuda:
        return False
    if noise is None:
        return True
    if noise.in_norm or noise.n_samples != 1 or (noise.kind == _lib.NOISE_EXPLICIT and getattr(noise, "group", 0) > 1):
        return False
    live = (noise.grad_params is not None and torch.is_grad_enabled()
            and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params))
    if live and noise.param_mode > _lib.PARAM_PER_CHANNEL:
        return False
    if grad and noise.param_mode == _lib.PARAM_PER_EDGE1:      # (stag_agg_max_bwd: STAG_ENOSYS)
        return False
    return True


def aggregate_max(graph, x, weight=None, seg_len=DEFAULT_SEG_LEN, _broadcast_x=False):
    """out[v,:] = max_{e=(u->v)} w[e,:] * x[u,:], 0 for rows without in-edges (DGL's `fn.max`;
    GraphSAGE 'pool', stag/zoo/graph_sage.py:90-93).

    On the GPU one fused pass (stag_agg_max_fwd): the noise is drawn in the kernel, no message tensor exists, and the
    backward walks the source-major CSR (stag_agg_max_bwd).  Every maximal message of a row gets an equal share of
    its gradient, as torch.scatter_reduce(amax) gives (except where a maximum is exactly +-0: include_self=False
    counts the zero start there too, the fused route does not).  Node-range shards, in-norm noise, Monte-Carlo
    batches, live per-edge parameters and CPU tensors take the composed route: the messages are formed ([E, D]: a
    kernel-backed gather, the noise materialised) and reduced with scatter-amax.
    _broadcast_x: x is one row [1, D] (or [D]) gathered for every edge (update_all(copy_e, max))."""
    if x.dim() != 2 and not _broadcast_x:
        raise ValueError("aggregate_max expects x of shape [N, D]")
    noise = weight if isinstance(weight, EdgeNoise) else None
    w = weight if torch.is_tensor(weight) else None
    D = x.numel() if _broadcast_x else x.shape[1]
    if w is not None:
        if w.shape[0] != graph.number_of_edges():
            raise AssertionError("edge_weight.shape[0] != number_of_edges")
        if w.dim() == 1:
            w = w.unsqueeze(1)
    if noise is not None and noise.dn != D:
        if noise.dn != 1:
            raise ValueError(f"noise width {noise.dn} != feature width {D}")
        # one weight per edge: the [E, 1] tensor (differentiable with live parameters), then the tensor path below
        weight = w = noise.materialize()
        noise = None
    grad_on = torch.is_grad_enabled()
    live = (noise is not None and noise.grad_params is not None and grad_on
            and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params))
    grad = grad_on and (x.requires_grad or (w is not None and w.requires_grad) or live)
    if _max_fused_route(graph, x, noise, w, grad):
        if w is not None and w.shape[1] != D:
            w = w.expand(w.shape[0], D)
        if not grad:
            # nothing to differentiate: straight to the library (no autograd node)
            if noise is not None:
                spec = _noise_spec(noise)
            elif w is not None:
                spec = _explicit_spec(_f32c(w))
            else:
                spec = _none_spec()
            return _max_fwd_raw(graph.csr, _f32c(x), D, spec, seg_len, False, _broadcast_x)[0]
        p0 = p1 = None
        if live:
            p0, p1 = (torch.as_tensor(p, dtype=torch.float32, device=x.device) for p in noise.grad_params)
        return _AggregateMax.apply(x, w, p0, p1, graph, noise, seg_len, _broadcast_x)
    if _broadcast_x:
        x = x.reshape(1, D).expand(graph.number_of_src_nodes() if hasattr(graph, "number_of_src_nodes")
                                   else graph.number_of_nodes(), D).contiguous()
    m = gather_rows(graph, x, "src")
    if isinstance(weight, EdgeNoise):
        weight = weight.materialize()
    if weight is not None:
        if weight.shape[0] != graph.number_of_edges():
            raise AssertionError("edge_weight.shape[0] != number_of_edges")
        m = m * (weight if weight.dim() == 2 else weight.unsqueeze(1))
    _, dst = graph.edges()
    n = graph.number_of_dst_nodes() if hasattr(graph, "number_of_dst_nodes") else graph.number_of_nodes()
    out = torch.zeros((n, x.shape[1]), dtype=m.dtype, device=m.device)
    return out.scatter_reduce(0, dst.long().unsqueeze(1).expand(-1, x.shape[1]), m, reduce="amax", include_self=False)


def aggregate_mc(graph, x, noise, n_samples, offset_stride=1, reduce="sum", src_scale=None,
                 dst_scale=None, seg_len=DEFAULT_SEG_LEN, _gathered=False):
    """[n_samples, N, D]: sample s == aggregate(graph, x, noise at offset + s * offset_stride), bit for
    bit, from one pass over the gathered rows per 4 samples (2 with in-norm: every sample carries its own weight
    sums) (stag_agg_fwd_mc).  The reference's Monte-Carlo loops — inference, stag/models.py:45-55, and training,
    stag/models.py:67-68 with `--n_samples_training` > 1 — on a layer whose input is the same for every sample.
    It needs no backward of its own when neither x nor the noise parameters carry a gradient (every `*_mle` script:
    the first layer's input is the data, the noise is fixed): the dense transform that follows differentiates
    through the S outputs.  When something here does need a gradient, or for noise the fused sampler does not
    cover, it is the stack of n_samples ordinary calls."""
    def one(s):
        import copy
        nz = copy.copy(noise)
        nz.offset = (noise.offset + s * offset_stride) & _MASK64
        return aggregate(graph, x, nz, reduce=reduce, src_scale=src_scale, dst_scale=dst_scale, seg_len=seg_len,
                         _gathered=_gathered)
    if getattr(graph, "is_shard", False) and not _gathered:
        return torch.stack([one(s) for s in range(n_samples)], 0)
    fusable_mc = (isinstance(noise, EdgeNoise) and noise.kind >= _lib.NOISE_NORMAL
                  and noise.param_mode <= _lib.PARAM_PER_CHANNEL)
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or (noise is not None and noise.grad_params is not None
                                                                  and any(torch.is_tensor(p) and p.requires_grad
                                                                          for p in noise.grad_params)))
    if (n_samples > 1 and isinstance(noise, EdgeNoise) and noise.param_mode == _lib.PARAM_PER_EDGE1
            and mc_edge_why_not(x, noise, graph) is None):
        # amortised [E, 1] parameters: the samples share the gather, the parameter loads and the unit walk
        # (stag_agg_fwd_mc_edge); under autograd the backward is the loop's per-sample passes (_AggregateMCEdge)
        if needs_grad:
            if noise.grad_params is not None:
                p0, p1 = (torch.as_tensor(p, dtype=torch.float32, device=x.device) for p in noise.grad_params)
            else:
                p0 = p1 = None
            return _AggregateMCEdge.apply(x, p0, p1, graph, noise, int(n_samples), int(offset_stride), _REDUCE[reduce],
                                          _f32c(src_scale), _f32c(dst_scale), seg_len)
        return _agg_fwd_mc_edge_raw(graph.csr, _f32c(x), noise, n_samples, offset_stride, _REDUCE[reduce],
                                    _f32c(src_scale), _f32c(dst_scale), seg_len)
    if (n_samples > 1 and isinstance(noise, EdgeNoise) and noise.param_mode == _lib.PARAM_PER_EDGE
            and mc_pedge_why_not(x, noise, graph) is None):
        # amortised [E, D] parameters: the samples share the gather, both parameter rows (one exp of the log-scale) and
        # the unit walk (stag_agg_fwd_mc_pedge); under autograd the backward is the loop's per-sample passes
        # (_AggregateMCPEdge)
        if needs_grad:
            if noise.grad_params is not None:
                p0, p1 = (torch.as_tensor(p, dtype=torch.float32, device=x.device) for p in noise.grad_params)
            else:
                p0 = p1 = None
            return _AggregateMCPEdge.apply(x, p0, p1, graph, noise, int(n_samples), int(offset_stride), _REDUCE[reduce],
                                           _f32c(src_scale), _f32c(dst_scale), seg_len)
        return _agg_fwd_mc_pedge_raw(graph.csr, _f32c(x), noise, n_samples, offset_stride, _REDUCE[reduce],
                                     _f32c(src_scale), _f32c(dst_scale), seg_len)
    if not fusable_mc or n_samples == 1:
        return torch.stack([one(s) for s in range(n_samples)], 0)
    if noise.dn != x.shape[1]:
        raise ValueError(f"noise width {noise.dn} != feature width {x.shape[1]}")
    if needs_grad:
        # the batched FORWARD under autograd (x or the noise parameters carry a gradient): the gathers of the S samples
        # are shared, the backward is the S per-sample transposed passes the loop would run (_AggregateMC).  Not with
        # in-norm (its factor has a derivative of its own: ops._AggregateVI) or explicit / per-edge parameters.
        live = noise.grad_params is not None and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params)
        if noise.in_norm or (live and noise.kind not in (_lib.NOISE_NORMAL, _lib.NOISE_UNIFORM)):
            return torch.stack([one(s) for s in range(n_samples)], 0)
        if live:
            p0, p1 = (torch.as_tensor(p, dtype=torch.float32, device=x.device) for p in noise.grad_params)
        else:
            p0 = p1 = None
        return _AggregateMC.apply(x, p0, p1, graph, noise, int(n_samples), int(offset_stride), _REDUCE[reduce],
                                  _f32c(src_scale), _f32c(dst_scale), seg_len)
    return _agg_fwd_mc_raw(graph.csr, _f32c(x), noise, n_samples, offset_stride, _REDUCE[reduce], _f32c(src_scale),
                           _f32c(dst_scale), seg_len)


def _agg_fwd_mc_raw(csrv, x, noise, n_samples, offset_stride, reduce, src_scale, dst_scale, seg_len):
    """One stag_agg_fwd_mc call: [n_samples, n_dst, D]."""
    D = x.shape[1]
    dev = _lib.require_device(x, csrv.indptr, src_scale, dst_scale)
    if _torch_ext.available():      # the dispatcher op (csrc/torch_ext.cpp): same library call, visible to a compiled graph
        plan_t = csrv.plan(seg_len)
        return torch.ops.stag.agg_fwd_mc(*csrv.torch_args(), *_plan_args(csrv, plan_t, (D + 255) // 256, dev, width=D, drawn=True, share=D),
                                         x, *noise.torch_args(), int(n_samples), int(offset_stride), reduce, src_scale, dst_scale)
    out = torch.empty((n_samples, csrv.n_dst, D), dtype=torch.float32, device=dev)
    plan_t = csrv.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], 4 * D, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv, seg_len, (D + 255) // 256, nbytes, dev, plan_t=plan_t, width=D, share=D)
    cs, spec = csrv.struct(), noise.spec()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_fwd_mc(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x), x.stride(0), D,
            C.byref(spec), n_samples, offset_stride, reduce, _lib.ptr(src_scale), _lib.ptr(dst_scale),
            _lib.ptr(out), D, csrv.n_dst * D, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_fwd_mc")
    return out


class _AggregateMC(torch.autograd.Function):
    """S Monte-Carlo samples of one aggregation (stag/models.py:67-68 on a layer whose input is the same for every
    sample) with gradients: the forward is ONE batched pass (stag_agg_fwd_mc: the gathers are shared), the backward
    the per-sample transposed passes of the sequential loop — d x summed over the samples, and for a reparameterised
    draw (`vi=True`) the finished parameter gradients of every sample (stag_agg_bwd_dp), summed.  Sample s draws at
    offset + s * stride, so values and gradients are those of the loop."""

    @staticmethod
    def forward(ctx, x, p0, p1, graph, noise, n_samples, stride, reduce, src_scale, dst_scale, seg_len):
        x = _f32c(x)
        out = _agg_fwd_mc_raw(graph.csr, x, noise, n_samples, stride, reduce, src_scale, dst_scale, seg_len)
        ctx.graph, ctx.noise, ctx.S, ctx.stride, ctx.reduce, ctx.seg_len = _owner(graph), noise, n_samples, stride, reduce, seg_len
        ctx.pshapes = None if p0 is None else (p0.shape, p1.shape)
        ctx.save_for_backward(x, src_scale, dst_scale)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        import copy
        x, src_scale, dst_scale = ctx.saved_tensors
        graph, D = ctx.graph, x.shape[1]
        g_all = _f32c(grad_out)
        dvec = dst_scale
        if ctx.reduce == _lib.REDUCE_MEAN:
            inv = 1.0 / graph.csr.degrees.clamp(min=1).to(torch.float32)
            dvec = inv if dvec is None else dvec * inv
        need_x = ctx.needs_input_grad[0]
        need_p = ctx.pshapes is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx = d0 = d1 = None
        for s_i in range(ctx.S):
            nz = copy.copy(ctx.noise)
            nz.offset = ctx.noise.offset + s_i * ctx.stride
            spec = _targs_or_c(_noise_spec(nz, in_norm=0))
            g = g_all[s_i]
            if need_p:
                dxs, c0, c1 = _agg_bwd_dp_raw(graph.csr_t, g, x, D, spec, dvec, src_scale, ctx.seg_len, want_dx=need_x)
                d0 = c0 if d0 is None else d0 + c0
                d1 = c1 if d1 is None else d1 + c1
            else:
                dxs, _ = _agg_raw(graph.csr_t, g, D, spec, _lib.REDUCE_SUM, dvec, src_scale, ctx.seg_len)
            if need_x:
                dx = dxs if dx is None else dx + dxs
        dp = [None, None]
        if need_p:
            for i, d in enumerate((d0, d1)):
                if ctx.needs_input_grad[1 + i]:
                    shape = ctx.pshapes[i]
                    dp[i] = d.sum().reshape(shape) if d.numel() != int(torch.Size(shape).numel()) else d.reshape(shape)
        return dx, dp[0], dp[1], None, None, None, None, None, None, None, None


# ---- Monte-Carlo samples of amortised [E, 1] edge noise (STAG_PARAM_PER_EDGE1) from one row gather ----------------------
# stag_agg_fwd_mc_edge: S samples of a layer whose q_a is an AmortizedDistribution(in, 1) — the first layer of every
# `*_rec` script, evaluated and trained through model.forward / model.loss with n_samples > 1 (stag/models.py:45-55,
# 67-68) — from one walk of the plan: per edge the ids, the two parameters and the row are read once, and only the Philox
# block is drawn per sample.  The switch ships True by the usual rule: the batched launch is not slower than the loop of
# S stag_agg_fwd launches, beyond the spread of two repeats, for EVERY case timed (profiles/r17/mc_edge.txt; us per S
# samples, batched / loop, S = 2 | 4 | 8; two repeats of the loop differ by 0.1-4.9, of the batched launch by 0.3-11.6):
#   arxiv D = 128      Normal + log-scale 227 / 358 | 383 / 707 | 762 / 1403     Uniform 198 / 355 | 323 / 699 | 641 / 1384
#   PPI batch D = 50   Normal + log-scale 107 / 115 | 146 / 220 | 288 / 433      Uniform  95 / 115 | 124 / 219 | 244 / 429
#   PPI batch D = 256  Normal + log-scale 268 / 338 | 462 / 683 | 923 / 1352     Uniform 218 / 312 | 372 / 639 | 743 / 1259
# The narrowest win is S = 2 at D = 50 (8 us); at S = 4 a pass costs 0.54-0.68 of the four launches.  An inference
# StagModel.forward(n_samples = 4) of the arxiv_rec/gcn model: 3.47 ms against 3.80.  With the switch off, PER_EDGE1
# descriptors with n_samples > 1 take the loop.
MC_EDGE_FUSED = True


def mc_edge_why_not(x, noise, graph):
    """The first reason ops.aggregate_mc does not hand x [N, D] with this descriptor ([E, 1] parameters, n_samples > 1)
    to stag_agg_fwd_mc_edge, or None.  One clause per refusal of the entry point (include/stag_hip.h) and per path
    without a form there; whatever gets a reason takes the stack of single calls."""
    if not MC_EDGE_FUSED:
        return "switch"
    if x.dim() != 2:
        return "shape"
    if x.stride(0) == 0:
        return "broadcast row"
    if x.dtype != torch.float32:
        return "dtype"
    if not isinstance(noise, EdgeNoise):
        return "no descriptor"
    if noise.param_mode != _lib.PARAM_PER_EDGE1:
        return "noise parameters"
    if noise.dn != x.shape[1]:
        return "noise width"
    if noise.in_norm:
        return "in-norm"
    if noise.kind not in (_lib.NOISE_NORMAL, _lib.NOISE_UNIFORM):
        return "kind"
    if noise.deriv:
        return "derivative selector"
    if noise.chunk_base:
        return "channel shard"
    if (noise.pos_base & 0xFFFFFFFF) + noise.graph.number_of_edges() > (1 << 32):
        return "position range"
    if getattr(graph, "is_shard", False) or getattr(noise.graph, "is_shard", False):
        return "shard"
    if torch.compiler.is_compiling():
        return "compiling"
    if not x.is_cuda:
        return "device"
    return None


def _agg_fwd_mc_edge_raw(csrv, x, noise, n_samples, offset_stride, reduce, src_scale, dst_scale, seg_len):
    """One stag_agg_fwd_mc_edge call: [n_samples, n_dst, D].  Bound through ctypes only; the plan is walked in plan order, or in
    the view's share order."""
    D = x.shape[1]
    dev = _lib.require_device(x, csrv.indptr, src_scale, dst_scale)
    out = torch.empty((n_samples, csrv.n_dst, D), dtype=torch.float32, device=dev)
    if csrv.n_dst == 0:
        return out
    plan_t = csrv.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], 4 * D, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv, seg_len, (D + 255) // 256, nbytes, dev, plan_t=plan_t, width=None, share=D)
    cs, spec = csrv.struct(), noise.spec()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_fwd_mc_edge(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x), x.stride(0), D,
            C.byref(spec), n_samples, offset_stride, reduce, _lib.ptr(src_scale), _lib.ptr(dst_scale),
            _lib.ptr(out), D, csrv.n_dst * D, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_fwd_mc_edge")
    return out


class _AggregateMCEdge(torch.autograd.Function):
    """S Monte-Carlo samples of one aggregation with [E, 1] noise parameters, with gradients: the forward is ONE batched
    pass (stag_agg_fwd_mc_edge), the backward the per-sample transposed passes of the sequential loop, on the kernels
    _AggregateVI chooses for [E, 1] parameters — stag_agg_bwd_edge (dx and both per-edge gradients from one pass) for
    D <= 256, else stag_agg_bwd + stag_agg_bwd_w.  dx and the [E, 1] gradients are summed over the samples.  Sample s
    draws at offset + s * stride, so values and gradients are those of the loop.  Nothing [E, D]-sized is saved.
    Where mc_bwd_why_not allows (MC_BWD_FUSED; x without a gradient, or D > 256) both [E, 1] gradients of all samples
    come from one stag_agg_bwd_w_mc call instead; dx stays the loop's."""

    @staticmethod
    def forward(ctx, x, p0, p1, graph, noise, n_samples, stride, reduce, src_scale, dst_scale, seg_len):
        x = _f32c(x)
        out = _agg_fwd_mc_edge_raw(graph.csr, x, noise, n_samples, stride, reduce, src_scale, dst_scale, seg_len)
        ctx.graph, ctx.noise, ctx.S, ctx.stride, ctx.reduce, ctx.seg_len = _owner(graph), noise, n_samples, stride, reduce, seg_len
        ctx.pshapes = None if p0 is None else (p0.shape, p1.shape)
        ctx.save_for_backward(x, src_scale, dst_scale)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        import copy
        x, src_scale, dst_scale = ctx.saved_tensors
        graph, D = ctx.graph, x.shape[1]
        g_all = _f32c(grad_out)
        dvec = dst_scale
        if ctx.reduce == _lib.REDUCE_MEAN:
            inv = 1.0 / graph.csr.degrees.clamp(min=1).to(torch.float32)
            dvec = inv if dvec is None else dvec * inv
        need_x = ctx.needs_input_grad[0]
        need_p = ctx.pshapes is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx = d0 = d1 = None
        # both [E, 1] gradients of all S samples from one pass (stag_agg_bwd_w_mc) where x needs no gradient or D > 256;
        # with dx at D <= 256 stag_agg_bwd_edge already takes all three from one gather per sample
        fused = need_p and mc_bwd_why_not(x, ctx.noise, graph, need_x) is None
        if fused:
            d0, d1 = _bwd_w_mc_raw(graph.csr, x, g_all, D, src_scale, dvec, _targs_or_c(_noise_spec(ctx.noise, in_norm=0)),
                                   ctx.S, ctx.stride, reduce_k=True, seg_len=ctx.seg_len)
        for s_i in range(ctx.S if (need_x or not fused) else 0):
            nz = copy.copy(ctx.noise)
            nz.offset = (ctx.noise.offset + s_i * ctx.stride) & _MASK64
            spec = _targs_or_c(_noise_spec(nz, in_norm=0))
            g = g_all[s_i]
            dxs = e0 = e1 = None
            if need_p and not fused and D <= 256:
                dxs, e0, e1 = _agg_bwd_edge_raw(graph.csr_t, g, x, D, spec, dvec, src_scale, ctx.seg_len, want_dx=need_x)
            else:
                if need_x:
                    dxs, _, _ = _agg_bwd_raw(graph.csr_t, g, D, spec, dvec, src_scale, ctx.seg_len, False)
                if need_p and not fused:
                    gg = (g if dvec is None else g * dvec.unsqueeze(1)).contiguous()
                    e0, e1 = _bwd_w_raw(graph.csr, x, gg, D, src_scale, spec=spec, reduce_k=True, both=True,
                                        seg_len=ctx.seg_len)
            if need_x:
                dx = dxs if dx is None else dx + dxs
            if need_p and not fused:
                d0 = e0 if d0 is None else d0 + e0
                d1 = e1 if d1 is None else d1 + e1
        dp = [None, None]
        if need_p:
            for i, d in enumerate((d0, d1)):
                if ctx.needs_input_grad[1 + i]:
                    shape = ctx.pshapes[i]
                    dp[i] = d.sum_to_size(shape) if d.dim() >= len(shape) and shape != d.shape else d.reshape(shape)
        return dx, dp[0], dp[1], None, None, None, None, None, None, None, None


# ---- Monte-Carlo samples of amortised [E, D] edge noise (STAG_PARAM_PER_EDGE) from one pass ------------------------------
# stag_agg_fwd_mc_pedge: S samples of a layer whose q_a is an AmortizedDistribution(in, in) — both layers of
# `citation_rec/gcn`, evaluated and trained through model.forward / model.loss with n_samples > 1 (stag/models.py:45-55,
# 67-68) — from one walk of the plan: per edge the ids, the lane's values of both [E, D] parameter rows (the log-scale
# exponentiated once) and the row are read once, and only the Philox block is drawn per sample.  The switch ships True by
# the usual rule: the batched launch is not slower than the loop of S stag_agg_fwd launches, beyond the spread of two
# repeats, for EVERY case timed (profiles/r19/mc_pedge.txt; us per S samples, batched / loop, S = 2 | 4 | 8 | 16; two
# repeats of the loop differ by 0.2-7.9, of the batched launch by 0.4-34):
#   arxiv D = 128         Normal + log-scale 430 / 705 | 609 / 1386 | 1235 / 2750 | 2455 / 5481
#                         Uniform            392 / 705 | 516 / 1387 | 1023 / 2744 | 2030 / 5472
#   PPI batch D = 50      Normal + log-scale 199 / 289 | 252 / 566 | 500 / 1120 | 985 / 2219     Uniform 195 / 264 | 239 / 516 | 474 / 1021 | 940 / 2025
#   PPI batch D = 256     Normal + log-scale 510 / 826 | 737 / 1631 | 1465 / 3237 | 2910 / 6452  Uniform 453 / 824 | 608 / 1628 | 1211 / 3232 | 2403 / 6441
#   Cora-sized D = 1433   Normal + log-scale 134 / 181 | 167 / 352 | 342 / 733 | 668 / 1442      Uniform 127 / 170 | 154 / 331 | 313 / 685 | 617 / 1353
# The narrowest win is S = 2 on the Cora-sized graph (43 us, 50 times the spread); a pass of 4 samples costs 0.37-0.47 of
# four launches.  An inference StagModel.forward(n_samples = 16) of a citation_rec/gcn-shaped model (leading Dropout,
# 1433 -> 16 -> 7) on the Cora-sized graph: 6.0 ms against 20.8 — q_a.condition() runs once instead of 16 times.  With the
# switch off, PER_EDGE descriptors with n_samples > 1 take the loop.
MC_PEDGE_FUSED = True


def mc_pedge_why_not(x, noise, graph):
    """The first reason ops.aggregate_mc does not hand x [N, D] with this descriptor ([E, D] parameters, n_samples > 1)
    to stag_agg_fwd_mc_pedge, or None.  One clause per refusal of the entry point (include/stag_hip.h) and per path
    without a form there; whatever gets a reason takes the stack of single calls."""
    if not MC_PEDGE_FUSED:
        return "switch"
    if x.dim() != 2:
        return "shape"
    if x.stride(0) == 0:
        return "broadcast row"
    if x.dtype != torch.float32:
        return "dtype"
    if not isinstance(noise, EdgeNoise):
        return "no descriptor"
    if noise.param_mode != _lib.PARAM_PER_EDGE:
        return "noise parameters"
    if noise.dn != x.shape[1]:
        return "noise width"
    if noise.in_norm:
        return "in-norm"
    if noise.kind not in (_lib.NOISE_NORMAL, _lib.NOISE_UNIFORM):
        return "kind"
    if noise.deriv:
        return "derivative selector"
    if noise.chunk_base:
        return "channel shard"
    if (noise.pos_base & 0xFFFFFFFF) + noise.graph.number_of_edges() > (1 << 32):
        return "position range"
    if getattr(graph, "is_shard", False) or getattr(noise.graph, "is_shard", False):
        return "shard"
    if torch.compiler.is_compiling():
        return "compiling"
    if not x.is_cuda:
        return "device"
    return None


def _agg_fwd_mc_pedge_raw(csrv, x, noise, n_samples, offset_stride, reduce, src_scale, dst_scale, seg_len):
    """One stag_agg_fwd_mc_pedge call: [n_samples, n_dst, D].  Bound through ctypes only; the plan is walked in plan order,
    or in the view's share order."""
    D = x.shape[1]
    dev = _lib.require_device(x, csrv.indptr, src_scale, dst_scale)
    out = torch.empty((n_samples, csrv.n_dst, D), dtype=torch.float32, device=dev)
    if csrv.n_dst == 0:
        return out
    plan_t = csrv.plan(seg_len)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], 4 * D, 0) if plan_t is not None else 0
    plan_c, _keep = _plan_struct(csrv, seg_len, (D + 255) // 256, nbytes, dev, plan_t=plan_t, width=None, share=D)
    cs, spec = csrv.struct(), noise.spec()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_fwd_mc_pedge(
            C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x), x.stride(0), D,
            C.byref(spec), n_samples, offset_stride, reduce, _lib.ptr(src_scale), _lib.ptr(dst_scale),
            _lib.ptr(out), D, csrv.n_dst * D, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_fwd_mc_pedge")
    return out


class _AggregateMCPEdge(torch.autograd.Function):
    """S Monte-Carlo samples of one aggregation with [E, D] noise parameters, with gradients: the forward is ONE batched
    pass (stag_agg_fwd_mc_pedge), the backward the per-sample passes of the sequential loop, on the kernels _AggregateVI
    chooses for [E, D] parameters — stag_agg_bwd on csr_t for dx, and both [E, D] parameter gradients from one
    stag_agg_bwd_w call.  dx and the parameter gradients are summed over the samples in place.  Sample s draws at
    offset + s * stride, so values and gradients are those of the loop.  Nothing beyond the gradients themselves is
    [E, D]-sized.  Where mc_bwd_why_not allows (MC_BWD_FUSED) both [E, D] gradients of all samples come from one
    stag_agg_bwd_w_mc call instead; dx stays the loop's."""

    @staticmethod
    def forward(ctx, x, p0, p1, graph, noise, n_samples, stride, reduce, src_scale, dst_scale, seg_len):
        x = _f32c(x)
        out = _agg_fwd_mc_pedge_raw(graph.csr, x, noise, n_samples, stride, reduce, src_scale, dst_scale, seg_len)
        ctx.graph, ctx.noise, ctx.S, ctx.stride, ctx.reduce, ctx.seg_len = _owner(graph), noise, n_samples, stride, reduce, seg_len
        ctx.pshapes = None if p0 is None else (p0.shape, p1.shape)
        ctx.save_for_backward(x, src_scale, dst_scale)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        import copy
        x, src_scale, dst_scale = ctx.saved_tensors
        graph, D = ctx.graph, x.shape[1]
        g_all = _f32c(grad_out)
        dvec = dst_scale
        if ctx.reduce == _lib.REDUCE_MEAN:
            inv = 1.0 / graph.csr.degrees.clamp(min=1).to(torch.float32)
            dvec = inv if dvec is None else dvec * inv
        need_x = ctx.needs_input_grad[0]
        need_p = ctx.pshapes is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx = d0 = d1 = None
        # both [E, D] gradients of all S samples from one pass (stag_agg_bwd_w_mc): dvec rides along as g_scale, so no
        # [N, D] product is formed and each gradient table is written once
        fused = need_p and mc_bwd_why_not(x, ctx.noise, graph, need_x) is None
        if fused:
            d0, d1 = _bwd_w_mc_raw(graph.csr, x, g_all, D, src_scale, dvec, _targs_or_c(_noise_spec(ctx.noise, in_norm=0)),
                                   ctx.S, ctx.stride, reduce_k=False, seg_len=ctx.seg_len)
        # a sample's dx and both of its [E, D] gradients from one transposed pass (stag_agg_bwd_pedge), where x needs a
        # gradient and the batched call above did not take the parameters
        one_pass = (PEDGE_BWD_MC_LOOP and need_x and need_p and not fused
                    and pedge_bwd_why_not(x, ctx.noise, graph, need_x) is None)
        for s_i in range(ctx.S if (need_x or not fused) else 0):
            nz = copy.copy(ctx.noise)
            nz.offset = (ctx.noise.offset + s_i * ctx.stride) & _MASK64
            spec = _noise_spec(nz, in_norm=0)
            g = g_all[s_i]
            if one_pass:
                dxs, e0, e1 = _agg_bwd_pedge_raw(graph.csr_t, g, x, D, _targs_or_c(spec), dvec, src_scale, ctx.seg_len)
                dx = dxs if dx is None else dx.add_(dxs)
                d0 = e0 if d0 is None else d0.add_(e0)
                d1 = e1 if d1 is None else d1.add_(e1)
                continue
            if need_x:
                dxs, _, _ = _agg_bwd_raw(graph.csr_t, g, D, spec, dvec, src_scale, ctx.seg_len, False)
                dx = dxs if dx is None else dx.add_(dxs)
            if need_p and not fused:
                gg = (g if dvec is None else g * dvec.unsqueeze(1)).contiguous()
                e0, e1 = _bwd_w_raw(graph.csr, x, gg, D, src_scale, spec=_targs_or_c(spec), both=True, seg_len=ctx.seg_len)
                d0 = e0 if d0 is None else d0.add_(e0)
                d1 = e1 if d1 is None else d1.add_(e1)
        dp = [None, None]
        if need_p:
            for i, d in enumerate((d0, d1)):
                if ctx.needs_input_grad[1 + i]:
                    shape = ctx.pshapes[i]
                    dp[i] = d.sum_to_size(shape) if d.dim() >= len(shape) and shape != d.shape else d.reshape(shape)
        return dx, dp[0], dp[1], None, None, None, None, None, None, None, None


# ---- dx and both [E, D] parameter gradients of one draw from ONE transposed pass --------------------------------------
# stag_agg_bwd_pedge: on the source-major CSR the row of x an edge's gradients need is the unit's own row and the row of g
# is the one the dx pass gathers anyway, so one walk (one gather, one read of each parameter table, one Philox block per
# edge and chunk) replaces stag_agg_bwd on csr_t + the [N, D] product g * dvec + stag_agg_bwd_w on csr, which gathers a row
# per edge again, reads both tables again and draws the same blocks again.  Taken by _AggregateVI.backward, and by the
# per-sample loop of _AggregateMCPEdge.backward (PEDGE_BWD_MC_LOOP), for [E, D] parameters without in-norm when x needs a
# gradient as well; without dx stag_agg_bwd_w alone is already one pass.
# Compiler's report (csrc/_obj/agg_bwd_pedge.remarks): 0 bytes of scratch in all 15 instantiations; the walk takes 129 VGPRs
# for Normal (3 waves per SIMD) and 122 for Uniform (4), the merge 92-96 (5).
# Measured (profiles/r25/pedge_bwd.txt; us per backward call, one pass / the three launches, Normal + log-scale | Uniform;
# two repeats of the three launches differ by 0.6-12.3, of the one pass by 0.0-6.2):
#   arxiv D = 128          676 /  943 | 535 /  925        PPI batch D = 50      350 / 489 | 373 / 521
#   PPI batch D = 256      852 / 1172 | 669 / 1138        Pubmed-sized D = 500  237 / 443 | 224 / 457
#   Cora-sized D = 1433    121 /  663 | 118 /  660        Cora-sized D = 16      19 / 102 |  19 / 102
# The training step of StagLayer(GCN(in, in), AmortizedDistribution(in, in), vi=True) on an input that needs a gradient, ms,
# switch on / off: 8.15 / 8.39, 4.12 / 4.23, 13.19 / 13.48, 5.41 / 5.64, 5.02 / 5.60, 1.93 / 1.93 (in that order).
# The switch ships True by the usual rule (True only if the one pass is not slower than the three launches, beyond the
# spread of two repeats, for EVERY case timed): all 18 cases meet it.
PEDGE_BWD_FUSED = True
# ... and whether the per-sample loop of _AggregateMCPEdge.backward takes it as well.  Ships False: that loop was not among
# the cases timed (the rule asks for a measurement of every case a switch turns on), and tests/test_gpu_mc_bwd.py holds the
# loop at the shipped defaults to one stag_agg_bwd_w call per sample.  tests/test_gpu_bwd_pedge.py runs it switched on.
PEDGE_BWD_MC_LOOP = False


def pedge_bwd_why_not(x, noise, graph, need_x):
    """The first reason the backward of an aggregation with [E, D] noise parameters (_AggregateVI, the per-sample loop of
    _AggregateMCPEdge) does not take dx and both gradient tables from one stag_agg_bwd_pedge call, or None.  One clause per
    refusal of the entry point (include/stag_hip.h) and per path without a form there; whatever gets a reason keeps
    stag_agg_bwd + stag_agg_bwd_w.  need_x: x needs a gradient — without it stag_agg_bwd_w alone is one pass already."""
    if not PEDGE_BWD_FUSED:
        return "switch"
    if x.dim() != 2:
        return "shape"
    if x.stride(0) == 0:
        return "broadcast row"
    if x.dtype != torch.float32:
        return "dtype"
    if not isinstance(noise, EdgeNoise):
        return "no descriptor"
    if noise.param_mode != _lib.PARAM_PER_EDGE:
        return "noise parameters"
    if noise.dn != x.shape[1]:
        return "noise width"
    if noise.in_norm:
        return "in-norm"
    if noise.kind not in (_lib.NOISE_NORMAL, _lib.NOISE_UNIFORM):
        return "kind"
    if noise.deriv:
        return "derivative selector"
    if noise.chunk_base:
        return "channel shard"
    if (noise.pos_base & 0xFFFFFFFF) + noise.graph.number_of_edges() > (1 << 32):
        return "position range"
    if getattr(graph, "is_shard", False) or getattr(noise.graph, "is_shard", False):
        return "shard"
    if not need_x:
        return "no dx"
    if torch.compiler.is_compiling():
        return "compiling"
    if not x.is_cuda:
        return "device"
    return None


# ---- The per-edge parameter gradients of a Monte-Carlo batch from one pass ---------------------------------------------
# stag_agg_bwd_w_mc: the parameter side of the backward of _AggregateMCEdge and _AggregateMCPEdge.  On the forward csr
# everything a sample does not own is shared — x[u], the edge's parameters (one exp of a log-scale), the ids — the S
# gradient rows are the unit's own rows, only the Philox block is drawn per sample, and the sum over samples happens in
# registers: each gradient table is written once.  For [E, D] heads one call replaces S x (g * dvec pass + stag_agg_bwd_w +
# two add_ passes); for [E, 1] heads it replaces S stag_agg_bwd_edge passes over csr_t where x needs no gradient (the first
# layer of every model) and S stag_agg_bwd_w passes at D > 256.  dx keeps the loop's per-sample passes in every case.
# Compiler's report (csrc/_obj/agg_bwd_w_mc.remarks): 0 bytes of scratch in all 42 instantiations; a pass of 4 samples takes
# 235-238 VGPRs (2 waves per SIMD), of 2 samples 185-190 (2), of 1 sample 159-160 (3); teams of one lane 122-202.
# Measured (profiles/r21/mc_bwd.txt; us per backward of S samples, batched / loop, S = 2 | 4; both parameters live, x
# without a gradient; two repeats of the loop differ by 0.5-47, of the batched call by 0.1-60):
#   [E, D] heads   arxiv D = 128        Normal + log-scale 1189 / 1928 | 1431 / 4518     Uniform 1063 / 1941 | 1212 / 4458
#                  PPI batch D = 50     Normal + log-scale  532 /  920 |  596 / 2031     Uniform  513 /  921 |  577 / 2042
#                  PPI batch D = 256    Normal + log-scale 1456 / 2467 | 1654 / 5747     Uniform 1276 / 2538 | 1455 / 5914
#                  Cora-sized D = 1433  Normal + log-scale  965 / 1375 | 1202 / 2849     Uniform  954 / 1400 | 1154 / 2845
#   [E, 1] heads   arxiv D = 128        Normal + log-scale  792 /  433 |  998 /  861     Uniform  766 /  423 |  984 /  853
#                  PPI batch D = 50     Normal + log-scale  267 /  161 |  320 /  293     Uniform  256 /  144 |  312 /  258
#                  PPI batch D = 256    Normal + log-scale  951 /  505 | 1180 / 1011     Uniform  921 /  448 | 1169 /  907
#                  Cora-sized D = 1433  Normal + log-scale  399 /  537 |  565 / 1058     Uniform  410 /  535 |  617 / 1055
# The peak allocation of a backward halves for [E, D] heads at S = 2 and is a third at S = 4 (arxiv: 1140 MB against 2280 |
# 3420: the two gradient tables, without the loop's per-sample pair).
# The switch ships False by the usual rule (True only if the batched call is not slower than the loop, beyond the spread
# of two repeats, for EVERY case timed): every [E, D] case wins (0.69 of the loop at the narrowest, Cora-sized S = 2; 0.25-0.42
# at S = 4) and so do [E, 1] heads past one channel tile, but [E, 1] heads at D <= 256 whose input carries no gradient
# LOSE to the S stag_agg_bwd_edge passes in all 12 cases timed: arxiv D = 128, PPI batch D = 50 and D = 256, Normal with
# log-scale and Uniform, S = 2 and S = 4 (by 27-473 us; 1.09-2.06 of the loop).  There a pass costs a fixed ~590 us at the
# arxiv shape plus ~100 us per sample against the loop's ~215 us per sample: the walk of two edges at a time at 2 waves
# per SIMD is bound by its dependent loads (ids, then rows), not by traffic.  With the switch off both nodes run the loop.
MC_BWD_FUSED = False


def mc_bwd_why_not(x, noise, graph, need_x):
    """The first reason the backward of ops.aggregate_mc (_AggregateMCEdge, _AggregateMCPEdge) does not take the parameter
    gradients of its samples from one stag_agg_bwd_w_mc call, or None.  One clause per refusal of the entry point
    (include/stag_hip.h) and per path without a form there; whatever gets a reason keeps the per-sample loop.  need_x: x
    needs a gradient too — then [E, 1] heads at D <= 256 keep stag_agg_bwd_edge, which takes dx and both gradients from
    one gather per sample."""
    if not MC_BWD_FUSED:
        return "switch"
    if x.dim() != 2:
        return "shape"
    if x.stride(0) == 0:
        return "broadcast row"
    if x.dtype != torch.float32:
        return "dtype"
    if not isinstance(noise, EdgeNoise):
        return "no descriptor"
    if noise.param_mode not in (_lib.PARAM_PER_EDGE1, _lib.PARAM_PER_EDGE):
        return "noise parameters"
    if noise.dn != x.shape[1]:
        return "noise width"
    if noise.in_norm:
        return "in-norm"
    if noise.kind not in (_lib.NOISE_NORMAL, _lib.NOISE_UNIFORM):
        return "kind"
    if noise.deriv:
        return "derivative selector"
    if noise.chunk_base:
        return "channel shard"
    if (noise.pos_base & 0xFFFFFFFF) + noise.graph.number_of_edges() > (1 << 32):
        return "position range"
    if getattr(graph, "is_shard", False) or getattr(noise.graph, "is_shard", False):
        return "shard"
    if noise.param_mode == _lib.PARAM_PER_EDGE1 and need_x and x.shape[1] <= 256:
        return "one gather"
    if torch.compiler.is_compiling():
        return "compiling"
    if not x.is_cuda:
        return "device"
    return None


def _bwd_w_mc_raw(csrv, x, g_all, D, src_scale, g_scale, spec, n_samples, offset_stride, reduce_k=False,
                  seg_len=DEFAULT_SEG_LEN, both=True):
    """One stag_agg_bwd_w_mc call: (d/dp0, d/dp1) summed over the n_samples draws of spec, [E, D] or, with reduce_k,
    [E, 1].  g_all: [n_samples, n_dst, D], contiguous.  Bound through ctypes only."""
    dev = _lib.require_device(x, g_all, src_scale, g_scale)
    cols = 1 if reduce_k else D
    dw0 = torch.empty((csrv.n_edges, cols), dtype=torch.float32, device=dev)
    dw1 = torch.empty_like(dw0) if both else None
    if csrv.n_edges == 0 or csrv.n_dst == 0:
        return dw0, dw1
    plan_c, _keep = _plan_struct(csrv, seg_len, 1, 0, dev)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_agg_bwd_w_mc(C.byref(cs), C.byref(plan_c) if plan_c is not None else None,
                                          _lib.ptr(x), x.stride(0), _lib.ptr(g_all), g_all.stride(-2), g_all.stride(0), D,
                                          _lib.ptr(src_scale), _lib.ptr(g_scale), C.byref(spec), n_samples, offset_stride,
                                          int(reduce_k), _lib.ptr(dw0), _lib.ptr(dw1), cols, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd_w_mc")
    return dw0, dw1


def materialize_noise(graph, noise, seg_len=DEFAULT_SEG_LEN):
    """The [E, Dn] tensor the reference would have sampled (rows by edge id)."""
    csrv = graph.csr
    dev = _lib.require_device(csrv.indptr)
    dn = noise.dn
    w = torch.empty((csrv.n_edges, dn), dtype=torch.float32, device=dev)
    ns = torch.empty((csrv.n_dst, dn), dtype=torch.float32, device=dev) if noise.in_norm else None
    plan_t = csrv.plan(seg_len)
    nbytes = (_lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], dn, 1)
              if (plan_t is not None and noise.in_norm) else 0)
    plan_c, _keep = _plan_struct(csrv, seg_len, (dn + 255) // 256, nbytes, dev)
    spec, cs = noise.spec(), csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_noise_materialize(C.byref(cs), C.byref(plan_c) if plan_c is not None else None,
                                               C.byref(spec), dn, _lib.ptr(w), dn, _lib.ptr(ns),
                                               _lib.stream_of(dev))
    _lib.check(rc, "stag_noise_materialize")
    return w


def philox_raw(seed, offset, pos0, n_pos, n_chunk, device):
    out = torch.empty((n_pos, n_chunk, 4), dtype=torch.int32, device=device)
    dev = _lib.require_device(out)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_philox_raw(seed, offset, pos0, n_pos, n_chunk, _lib.ptr(out),
                                        _lib.stream_of(dev))
    _lib.check(rc, "stag_philox_raw")
    return out


def normal_tables(device):
    """(rad, cos, sin): the hardware functions of a Normal draw over all 2^23 mantissas, [3, 2^23] fp32
    (stag_normal_tables; test hook — a CPU checker can redraw the device's normals from them)."""
    t = torch.empty((3, 1 << 23), dtype=torch.float32, device=device)
    dev = _lib.require_device(t)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_normal_tables(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.stream_of(dev))
    _lib.check(rc, "stag_normal_tables")
    return t


def _segment_reduce_raw(x, offsets, reduce, dev):
    B, D = offsets.shape[0] - 1, x.shape[1]
    out = torch.empty((B, D), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_segment_reduce(_lib.ptr(x), x.stride(0), D, _lib.ptr(offsets), B,
                                            reduce, _lib.ptr(out), D, _lib.stream_of(dev))
    _lib.check(rc, "stag_segment_reduce")
    return out


_SEG_CHUNK = 256


class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offsets, reduce):
        x = _f32c(x)
        dev = _lib.require_device(x, offsets)
        B, n = offsets.shape[0] - 1, x.shape[0]
        if B > 0 and n > _SEG_CHUNK * B:
            # long segments (a team walks a segment's rows: 15.8 ms for one 169k-row graph): sum
            # chunks of <= 256 rows first — many teams —, then each segment's chunk sums (0.2 ms).
            # The chunk table is built on the device: no host read-back of the segment lengths.
            R = _SEG_CHUNK
            lens = (offsets[1:] - offsets[:-1]).long()
            cptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            cptr[1:] = torch.cumsum((lens + R - 1) // R, 0)
            n_max = (n + R - 1) // R + B                      # host-side bound on the chunk count
            c = torch.arange(n_max, dtype=torch.int64, device=dev)
            seg = torch.searchsorted(cptr[1:], c, right=True).clamp(max=B - 1)
            start = offsets[:-1].long()[seg] + (c - cptr[seg]) * R
            start = torch.where(c < cptr[-1], start, torch.full_like(start, n))     # padding chunks: empty
            off1 = torch.cat([start, torch.full((1,), n, dtype=torch.int64, device=dev)]).to(torch.int32)
            # a chunk ends where the next one starts, except the last chunk of a segment, which
            # ends with the segment; segments are contiguous, so "next start" is right in both cases
            part = _segment_reduce_raw(x, off1, _lib.REDUCE_SUM, dev)
            out = _segment_reduce_raw(part, cptr.to(torch.int32), _lib.REDUCE_SUM, dev)
            if reduce == _lib.REDUCE_MEAN:
                out = out / lens.clamp(min=1).to(out.dtype).unsqueeze(1)
        else:
            out = _segment_reduce_raw(x, offsets, reduce, dev)
        ctx.reduce, ctx.n = reduce, n
        ctx.save_for_backward(offsets)
        return out

    @staticmethod
    def backward(ctx, g):
        (offsets,) = ctx.saved_tensors
        sizes = (offsets[1:] - offsets[:-1]).long()
        if ctx.reduce == _lib.REDUCE_MEAN:
            g = g / sizes.clamp(min=1).to(g.dtype).unsqueeze(1)
        return torch.repeat_interleave(g, sizes, dim=0, output_size=ctx.n), None, None


def segment_reduce(x, offsets, reduce="sum"):
    """Per-graph readout over a batched graph (dgl.sum_nodes / mean_nodes)."""
    return _SegmentReduce.apply(x, offsets.to(torch.int32).contiguous(), _REDUCE[reduce])


def _gat_norm_scale(csrv, noise, H, seg_len, dev):
    """in-norm factor [N, H] of H-wide weights (stag/layers.py:8-36): row sums on the aggregation
    kernel (a broadcast row of ones, same noise, in-norm off), then indeg / sum."""
    ones = torch.ones(1, H, dtype=torch.float32, device=dev)
    sums, _ = _agg_raw(csrv, ones, H, _noise_spec(noise, in_norm=0), _lib.REDUCE_SUM, None, None, seg_len,
                       broadcast_x=True)
    deg = csrv.degrees.to(torch.float32).unsqueeze(1)
    return torch.where(sums != 0, deg / sums, torch.ones_like(sums)).contiguous()


def _gat_drop_struct(attn_drop):
    """(p, seed, offset[, epoch tensor]) -> stag_gat_drop, or None"""
    if attn_drop is None:
        return None
    d = _lib.GatDrop()
    d.keep_prob = 1.0 - float(attn_drop[0])
    d.seed, d.offset = int(attn_drop[1]) & ((1 << 64) - 1), int(attn_drop[2]) & ((1 << 64) - 1)
    d.epoch = _lib.ptr(attn_drop[3]) if len(attn_drop) > 3 else None
    return d


def gat_lanes_per_head(F):
    """Lanes a head takes in the cooperative GAT kernels: F / 4 rounded up to a power of two (their head sums are
    butterflies; lanes past a head's channels idle)."""
    l = 1
    while l * 4 < F:
        l *= 2
    return l


def gat_cooperative_shape(H, F, seg_len):
    """The workgroup-cooperative GAT kernels (forward, one-gather backward, in-kernel dropout) take this shape."""
    return (F % 4 == 0 and F >= 4 and H <= 16 and H * F <= 1024 and gat_lanes_per_head(F) <= 64
            and H * gat_lanes_per_head(F) <= 256 and seg_len is not None and 0 < seg_len <= _lib.BLOCK_EDGES)


def attn_drop_fusable(H, F, seg_len, want_attn=False):
    """Attention dropout rides in the workgroup-cooperative GAT kernels (forward and one-gather backward)."""
    return not want_attn and _GAT_BWD_FUSED and _GAT_BWD_ONE_GATHER and gat_cooperative_shape(H, F, seg_len)


# stag_gat_fwd_half on fp16 / bf16 ft rows | ft.float() + stag_gat_fwd.  The two routes give the same bits, so the switch
# is a speed decision only.  True because, at cfg5 (8 x 32, bf16 rows, us per call, profiles/r10/gat_half_rows.txt), the
# half launch is not slower than the cast route for any kind timed — none 147.8 against 264.6, Normal 149.5 / 266.2,
# Normal + attention dropout 153.6 / 268.9; two repeats of the cast route differ by 0.0-0.5.  
GAT_HALF_ROWS = True
# zoo.GAT under CUDA autocast with a half dtype: ft from a half GEMM (and el / er from the input through the folded
# attention weight, in fp32) | everything in fp32 as ops.node_linear pins it.  Off: a layer under autocast computes
# what it always did.
GAT_HALF_FT = False


def gat_half_rows_why_not(ft, seg_len=DEFAULT_SEG_LEN, graph=None, noise=None, attn_fn=None, ignore_switch=False):
    """The first reason ops.gat_aggregate keeps the cast route (ft.float(), stag_gat_fwd) for this call, or None: the
    forward launches stag_gat_fwd_half on ft as it is.  One clause per refusal of the entry point (include/stag_hip.h)
    and per path that has no half form (the composed path, Monte-Carlo batches, shards, a traced graph).
    ignore_switch: whatever GAT_HALF_ROWS says (zoo.GAT asks whether a half ft COULD be gathered as it is: the two
    routes give the same bits, so what the layer computes must not depend on the switch)."""
    if not GAT_HALF_ROWS and not ignore_switch:
        return "switch"
    if ft.dtype not in _HALF_DTYPES:
        return "dtype"
    if ft.dim() != 3 or not gat_cooperative_shape(ft.shape[1], ft.shape[2], seg_len):
        return "shape"
    if attn_fn is not None:
        return "attention function"
    if noise is not None and getattr(noise, "n_samples", 1) != 1:
        return "monte-carlo"
    if getattr(graph, "is_shard", False) or (noise is not None and getattr(getattr(noise, "graph", None), "is_shard", False)):
        return "shard"
    if torch.compiler.is_compiling():
        return "compiling"
    if not ft.is_contiguous():
        return "strides"
    if not ft.is_cuda:
        return "device"
    if ft.data_ptr() % 8 != 0:
        return "alignment"
    return None


def gat_half_rows_ok(ft, seg_len=DEFAULT_SEG_LEN, graph=None, noise=None, attn_fn=None):
    return gat_half_rows_why_not(ft, seg_len, graph, noise, attn_fn) is None


def _gat_fwd_half_raw(csrv, plan_t, el, er, ft, H, F, neg_slope, spec, nscale, drop, out, stats, seg_len, dev):
    """One stag_gat_fwd_half launch: ft [n_src, H, F] fp16 | bf16 as it is, out / stats fp32.  Bound through ctypes only;
    returns the plan struct (stag_gat_attn takes the same one)."""
    nbytes = _lib.lib().stag_gat_workspace_bytes(plan_t["n_seg"], H, F)
    plan_c, _keep = _plan_struct(csrv, seg_len, 1, nbytes, dev, plan_t=plan_t, gat_width=H * F)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_gat_fwd_half(C.byref(cs), C.byref(plan_c), _lib.ptr(el), _lib.ptr(er), _lib.ptr(ft),
                                          _HALF_DTYPES[ft.dtype], H, F, float(neg_slope), C.byref(spec), _lib.ptr(nscale),
                                          C.byref(drop) if drop is not None else None,
                                          _lib.ptr(out), _lib.ptr(stats), _lib.stream_of(dev))
    _lib.check(rc, "stag_gat_fwd_half")
    return plan_c, _keep


class _GatAggregate(torch.autograd.Function):
    """p0, p1 (optional): the live parameter tensors of a reparameterised `noise` (vi=True): the draw stays in the
    kernels, forward and backward, and the backward returns their finished gradients (stag_gat_bwd_dp)."""

    @staticmethod
    def forward(ctx, el, er, ft, w, graph, noise, neg_slope, want_attn, seg_len, attn_drop=None, p0=None, p1=None):
        # half rows (ops.GAT_HALF_ROWS): the forward gathers ft as it is, and the half ft is what is kept for the backward
        half = gat_half_rows_ok(ft, seg_len, graph, noise)
        el, er, ft = _f32c(el), _f32c(er), (ft if half else _f32c(ft))
        ctx.pshapes = None if p0 is None else (p0.shape, p1.shape)
        H, F = ft.shape[1], ft.shape[2]
        csrv = graph.csr
        dev = _lib.require_device(el, er, ft, csrv.indptr)
        if noise is not None:
            spec = noise.spec()
        elif w is not None:
            w = _f32c(w)
            spec = _targs_or_c(_explicit_spec(w))
        else:
            spec = _targs_or_c(_none_spec())
        if attn_drop is not None and noise is None:
            spec.pos_base = int(getattr(graph, "pos_base", 0))    # a shard's dropout mask is the whole graph's
        nscale = _gat_norm_scale(csrv, noise, H, seg_len, dev) if spec.in_norm else None
        need_grad = any(ctx.needs_input_grad[:4]) or any(ctx.needs_input_grad[10:12])
        out = torch.empty((csrv.n_dst, H, F), dtype=torch.float32, device=dev)
        # softmax statistics per row [N, 2H]: the backward and the attention values are computed
        # from them (storing a[E, H] from the forward kernel cost it 250 us at cfg5)
        stats = (torch.empty((csrv.n_dst, 2 * H), dtype=torch.float32, device=dev)
                 if (want_attn or need_grad) else None)
        plan_t = csrv.plan(seg_len, need=True)       # the cooperative kernels want the plan's unit batches
        if _torch_ext.available() and not want_attn and plan_t is not None and not half:
            # the dispatcher op (csrc/torch_ext.cpp: stag::gat_fwd): same library call, visible to a compiled graph
            targs = noise.torch_args() if noise is not None else (_explicit_spec(w) if w is not None else _NONE_ARGS)
            if attn_drop is not None and noise is None:
                targs = (targs[0], [targs[1][0], targs[1][1], int(getattr(graph, "pos_base", 0))]) + tuple(targs[2:])
            out, stats_t = torch.ops.stag.gat_fwd(*csrv.torch_args(), *_gat_plan_args(csrv, plan_t, dev, H * F), el, er, ft,
                                                  float(neg_slope), *targs, nscale, *_gat_drop_args(attn_drop), bool(need_grad))
            if need_grad:
                ctx.graph, ctx.noise, ctx.neg_slope, ctx.seg_len = _owner(graph), noise, float(neg_slope), seg_len
                ctx.attn_drop = attn_drop
                ctx.save_for_backward(el, er, ft, w, stats_t, out, nscale)
            return out
        cs = csrv.struct()
        attn = None
        drop = _gat_drop_struct(attn_drop)
        if half:
            plan_c, _keep = _gat_fwd_half_raw(csrv, plan_t, el, er, ft, H, F, neg_slope, spec, nscale, drop, out, stats,
                                              seg_len, dev)
        else:
            nbytes = _lib.lib().stag_gat_workspace_bytes(plan_t["n_seg"], H, F) if plan_t is not None else 0
            plan_c, _keep = _plan_struct(csrv, seg_len, 1, nbytes, dev, plan_t=plan_t, gat_width=H * F)
        with _lib.on_device(dev):
            if not half:
                rc = _lib.lib().stag_gat_fwd(C.byref(cs), C.byref(plan_c) if plan_c is not None else None,
                                             _lib.ptr(el), _lib.ptr(er), _lib.ptr(ft), H, F,
                                             float(neg_slope), C.byref(spec), _lib.ptr(nscale),
                                             C.byref(drop) if drop is not None else None,
                                             _lib.ptr(out), _lib.ptr(stats), _lib.stream_of(dev))
                _lib.check(rc, "stag_gat_fwd")
            if want_attn:
                attn = torch.empty((csrv.n_edges, H), dtype=torch.float32, device=dev)
                rc = _lib.lib().stag_gat_attn(C.byref(cs), C.byref(plan_c) if plan_c is not None else None,
                                              _lib.ptr(el), _lib.ptr(er), H, float(neg_slope), C.byref(spec),
                                              _lib.ptr(nscale), _lib.ptr(stats), _lib.ptr(attn),
                                              _lib.stream_of(dev))
                _lib.check(rc, "stag_gat_attn")
        if need_grad:
            ctx.graph, ctx.noise, ctx.neg_slope, ctx.seg_len = _owner(graph), noise, float(neg_slope), seg_len
            ctx.attn_drop = attn_drop
            ctx.save_for_backward(el, er, ft, w, stats, out, nscale)
        if want_attn:
            ctx.mark_non_differentiable(attn)
            return out, attn
        return out

    @staticmethod
    def backward(ctx, grad_out, *unused):
        el, er, ft, w, stats, out, nscale = ctx.saved_tensors
        graph, noise = ctx.graph, ctx.noise
        ft = _f32c(ft)      # (a half ft of the half-row forward: widened for the length of this call; d ft leaves as fp32)
        H, F = ft.shape[1], ft.shape[2]
        HF = H * F
        csrv, csrt = graph.csr, graph.csr_t
        dev = ft.device
        G = _f32c(grad_out)
        if noise is not None:
            spec = noise.spec()
        elif w is not None:
            spec = _targs_or_c(_explicit_spec(w))
        else:
            spec = _targs_or_c(_none_spec())
        want_dw = w is not None and ctx.needs_input_grad[3]
        if ctx.attn_drop is not None and noise is None:
            spec.pos_base = int(getattr(graph, "pos_base", 0))
        want_dp = ctx.pshapes is not None and any(ctx.needs_input_grad[10:12])
        if csrv.n_edges == 0:        # no edge, no gradient
            zp = lambda i: (torch.zeros(ctx.pshapes[i], dtype=torch.float32, device=dev)
                            if (want_dp and ctx.needs_input_grad[10 + i]) else None)
            return (torch.zeros_like(el) if ctx.needs_input_grad[0] else None,
                    torch.zeros_like(er) if ctx.needs_input_grad[1] else None,
                    torch.zeros_like(ft) if ctx.needs_input_grad[2] else None,
                    torch.zeros_like(w) if want_dw else None, None, None, None, None, None, None, zp(0), zp(1))
        spec_tensors = ((noise.p0, noise.p1, noise.epoch) if noise is not None else (w, None, None))
        fused = _gat_bwd_fused(csrv, csrt, el, er, ft, stats, G, out, H, F, ctx.neg_slope, spec, nscale,
                               want_dw, ctx.seg_len, dev, ctx.attn_drop, want_dp=want_dp, spec_tensors=spec_tensors)
        if fused is not None:
            d_el, d_er, d_ft, dw = fused[:4]
            dps = [None, None]
            if want_dp:
                for i in range(2):
                    if ctx.needs_input_grad[10 + i]:
                        d, shape = fused[4 + i], ctx.pshapes[i]
                        dps[i] = d.sum().reshape(shape) if len(shape) == 0 or d.numel() != int(torch.Size(shape).numel()) else d.reshape(shape)
            return (d_el if ctx.needs_input_grad[0] else None, d_er if ctx.needs_input_grad[1] else None,
                    d_ft if ctx.needs_input_grad[2] else None, dw, None, None, None, None, None, None, dps[0], dps[1])
        if want_dp:
            raise NotImplementedError("vi=True GAT parameter gradients need the one-gather backward (stag_gat_bwd_dp)")
        if ctx.attn_drop is not None:
            raise NotImplementedError("attention dropout needs the one-gather GAT backward (stag_gat_bwd)")
        de = torch.empty((csrv.n_edges, H), dtype=torch.float32, device=dev)
        dw = torch.empty((csrv.n_edges, H), dtype=torch.float32, device=dev) if want_dw else None
        # a[E, H], a by-product of the edge pass: the weights of the d ft aggregation
        attn = (torch.empty((csrv.n_edges, H), dtype=torch.float32, device=dev)
                if ctx.needs_input_grad[2] else None)
        plan_c, _keep = _plan_struct(csrv, ctx.seg_len, 1, 0, dev)
        cs = csrv.struct()
        with _lib.on_device(dev):
            rc = _lib.lib().stag_gat_bwd_edge(
                C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(el),
                _lib.ptr(er), _lib.ptr(ft), _lib.ptr(stats), _lib.ptr(G), _lib.ptr(out), H, F,
                ctx.neg_slope, C.byref(spec), _lib.ptr(nscale), _lib.ptr(de), _lib.ptr(dw),
                _lib.ptr(attn), _lib.stream_of(dev))
        if rc == -38:
            raise NotImplementedError("GAT backward needs out_feats % 4 == 0 and out_feats / 4 a power of two")
        _lib.check(rc, "stag_gat_bwd_edge")
        ones = torch.ones(1, H, dtype=torch.float32, device=dev)
        d_el = d_er = d_ft = None
        if ctx.needs_input_grad[1]:      # d er[v,h] = sum over in-edges of de
            d_er, _ = _agg_raw(csrv, ones, H, _explicit_spec(de), _lib.REDUCE_SUM, None, None,
                               ctx.seg_len, broadcast_x=True)
        if ctx.needs_input_grad[0]:      # d el[u,h] = sum over out-edges of de
            d_el, _ = _agg_raw(csrt, ones, H, _explicit_spec(de), _lib.REDUCE_SUM, None, None,
                               ctx.seg_len, broadcast_x=True)
        if ctx.needs_input_grad[2]:      # d ft[u,h,:] = sum over out-edges of a[e,h] * G[v,h,:]
            d_ft, _ = _agg_raw(csrt, G.reshape(-1, HF), HF, _explicit_spec(attn, group=F), _lib.REDUCE_SUM, None, None,
                               ctx.seg_len)
            d_ft = d_ft.reshape(-1, H, F)
        return d_el, d_er, d_ft, dw, None, None, None, None, None, None, None, None


def _gat_plan_args(csrv, plan_t, dev, gat_width, transposed=False):
    """The plan arguments of torch.ops.stag.gat_fwd / gat_bwd: (units, long_rows, long_seg_ptr, block_ptr, xcd, counters,
    plan_ints), the unit batches the XCD-aware ones when the plan has them (transposed: the second plan of gat_bwd has no
    xcd slot)."""
    _, counters = _plan_counters(plan_t, 1, dev)    # shared with the aggregation launches of one channel tile: the GAT
                                                    # kernels use the first n_long ints only
    units, block_ptr, n_blocks, n_heavy = plan_t["units"], plan_t["block_ptr"], plan_t["n_blocks"], plan_t["n_heavy"]
    local = None
    if plan_t.get("xcd_on"):
        blocks = csrv.gat_blocks(plan_t, gat_width)
        if blocks is not None:
            units, block_ptr, n_blocks, n_heavy = blocks[0], blocks[1], blocks[2], 0
            local = units       # (non-NULL xcd slot: "these batches are XCD-local", as in _plan_struct)
    ints = [plan_t["seg_len"], plan_t["n_units"], plan_t["n_long"], plan_t["n_seg"], n_heavy, n_blocks, 0, 0]
    if transposed:
        return (units, plan_t["long_rows"], plan_t["long_seg_ptr"], block_ptr, counters, ints)
    return (units, plan_t["long_rows"], plan_t["long_seg_ptr"], block_ptr, local, counters, ints)


def _gat_drop_args(attn_drop):
    """(drop_floats, drop_u64, drop_epoch) of torch.ops.stag.gat_*: what _gat_drop_struct puts into a stag_gat_drop."""
    if attn_drop is None:
        return [], [], None
    s64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    seed, off = int(attn_drop[1]) & ((1 << 64) - 1), int(attn_drop[2]) & ((1 << 64) - 1)
    return [1.0 - float(attn_drop[0])], [s64(seed), s64(off)], (attn_drop[3] if len(attn_drop) > 3 else None)


def _ctypes_to_targs(s, tensors):
    """A ctypes stag_noise_spec back as the argument tuple of torch.ops.stag.* (tensors: (p0, p1, epoch) it points into)."""
    s64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    p0, p1, epoch = tensors
    return ([s.kind, s.param_mode, s.relu, s.in_norm, s.deriv, s.group, s.chunk_base, s.p1_log],
            [s64(s.seed), s64(s.offset), s.pos_base], [s.p0_scalar, s.p1_scalar], p0, p1, epoch)


def _gat_bwd_fused(csrv, csrt, el, er, ft, stats, G, out, H, F, neg_slope, spec, nscale, want_dw, seg_len, dev,
                   attn_drop=None, want_dp=False, spec_tensors=(None, None, None)):
    """stag_gat_bwd: the whole backward on the workgroup-cooperative kernels (one gather of the [H*F] rows; the
    two-gather form stag_gat_bwd_two_pass stays for A/B); None when the shape or the plans are outside what it
    covers (the caller then composes the older kernels)."""
    lph = F // 4
    E = csrv.n_edges
    one = _GAT_BWD_ONE_GATHER or attn_drop is not None or want_dp
    if not (_GAT_BWD_FUSED and E > 0 and gat_cooperative_shape(H, F, seg_len)
            and (one or (lph & (lph - 1)) == 0)):      # the two-pass form wants F / 4 a power of two
        return None
    if csrv.original_rows is not None:
        return _gat_bwd_reordered(csrv, csrt, el, er, ft, stats, G, out, H, F, neg_slope, _targs_or_c(spec), nscale, want_dw,
                                  seg_len, dev, attn_drop, want_dp)
    plan_f, plan_b = csrv.plan(seg_len, need=True), csrt.plan(seg_len, need=True)
    if _torch_ext.available() and not want_dp and (_GAT_BWD_ONE_GATHER or attn_drop is not None):
        # the dispatcher op (csrc/torch_ext.cpp: stag::gat_bwd): same library call, visible to a compiled graph
        if isinstance(spec, tuple):
            targs = spec
        else:       # (this function is handed the ctypes form: back to the argument tuple, the tensors from the caller's)
            targs = _ctypes_to_targs(spec, spec_tensors)
        try:
            d_el, d_er, d_ft, dw = torch.ops.stag.gat_bwd(
                *csrv.torch_args(), *_gat_plan_args(csrv, plan_f, dev, H * F),
                csrt.indptr, csrt.indices, csrt.eid, csrt.nidx, *_gat_plan_args(csrt, plan_b, dev, H * F, transposed=True),
                el, er, ft, stats, G, out, float(neg_slope), *targs, nscale, *_gat_drop_args(attn_drop), bool(want_dw))
        except RuntimeError as exc:
            if "rc=-38" in str(exc):        # STAG_ENOSYS: a shape / plan outside the cooperative kernels
                return None
            raise
        return d_el, d_er, d_ft, (dw if want_dw else None)
    nbytes = _lib.lib().stag_gat_bwd_workspace_bytes(plan_f["n_seg"], plan_b["n_seg"], H, F)
    pf, _k1 = _plan_struct(csrv, seg_len, 1, nbytes, dev, plan_t=plan_f, gat_width=H * F)
    pb, _k2 = _plan_struct(csrt, seg_len, 1, 0, dev, plan_t=plan_b, gat_width=H * F)
    d_el = torch.empty((csrt.n_dst, H), dtype=torch.float32, device=dev)
    d_er = torch.empty((csrv.n_dst, H), dtype=torch.float32, device=dev)
    d_ft = torch.empty((csrt.n_dst, H, F), dtype=torch.float32, device=dev)
    dw = torch.empty((E, H), dtype=torch.float32, device=dev) if want_dw else None
    scratch = torch.empty(_lib.lib().stag_gat_bwd_scratch_bytes(csrv.n_dst, E, H) // 4, dtype=torch.float32, device=dev)
    cs, ct = csrv.struct(), csrt.struct()
    drop = _gat_drop_struct(attn_drop)
    if want_dp:        # the one-gather backward that also finishes the gradients of scalar / per-head noise parameters
        dp0 = torch.empty(H, dtype=torch.float32, device=dev)
        dp1 = torch.empty(H, dtype=torch.float32, device=dev)
        wbytes = _lib.lib().stag_gat_bwd_dp_workspace_bytes(max(pb.n_blocks, pf.n_blocks), H)   # (the structs': XCD batches count more)
        ws = torch.empty(max(wbytes // 4, 1), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            rc = _lib.lib().stag_gat_bwd_dp(C.byref(cs), C.byref(pf), C.byref(ct), C.byref(pb), _lib.ptr(el), _lib.ptr(er),
                                            _lib.ptr(ft), _lib.ptr(stats), _lib.ptr(G), _lib.ptr(out), H, F, neg_slope,
                                            C.byref(spec), _lib.ptr(nscale), C.byref(drop) if drop is not None else None,
                                            _lib.ptr(d_el), _lib.ptr(d_er), _lib.ptr(d_ft), _lib.ptr(dp0), _lib.ptr(dp1),
                                            _lib.ptr(scratch), _lib.ptr(ws), wbytes, _lib.stream_of(dev))
        if rc == -38:
            return None
        _lib.check(rc, "stag_gat_bwd_dp")
        return d_el, d_er, d_ft, None, dp0, dp1
    fn = _lib.lib().stag_gat_bwd if (_GAT_BWD_ONE_GATHER or attn_drop is not None) else _lib.lib().stag_gat_bwd_two_pass
    with _lib.on_device(dev):
        rc = fn(C.byref(cs), C.byref(pf), C.byref(ct), C.byref(pb), _lib.ptr(el), _lib.ptr(er),
                _lib.ptr(ft), _lib.ptr(stats), _lib.ptr(G), _lib.ptr(out), H, F, neg_slope,
                C.byref(spec), _lib.ptr(nscale), C.byref(drop) if drop is not None else None,
                _lib.ptr(d_el), _lib.ptr(d_er), _lib.ptr(d_ft), _lib.ptr(dw), _lib.ptr(scratch), _lib.stream_of(dev))
    if rc == -38:
        return None
    _lib.check(rc, "stag_gat_bwd")
    return d_el, d_er, d_ft, dw


def _gat_fwd_into(csrv, plan_t, el, er, ft, H, F, neg_slope, spec, nscale, drop, out, stats, dev):
    """One stag_gat_fwd launch over the units of `plan_t` (the whole plan of csrv or a sub-plan of it: a shard's
    all-local rows, then the rest — partition._ShardGat) into existing out [n_dst, H, F] / stats [n_dst, 2H]."""
    nbytes = _lib.lib().stag_gat_workspace_bytes(plan_t["n_seg"], H, F)
    plan_c, _keep = _plan_struct(csrv, plan_t["seg_len"], 1, nbytes, dev, plan_t=plan_t, gat_width=H * F)
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_gat_fwd(C.byref(cs), C.byref(plan_c), _lib.ptr(el), _lib.ptr(er), _lib.ptr(ft), H, F,
                                     float(neg_slope), C.byref(spec), _lib.ptr(nscale),
                                     C.byref(drop) if drop is not None else None,
                                     _lib.ptr(out), _lib.ptr(stats), _lib.stream_of(dev))
    _lib.check(rc, "stag_gat_fwd")


class _GatBwdStages:
    """stag_gat_bwd one stage at a time (include/stag_hip.h, v19) with the arguments every stage shares held once:
    `rowdot()`, `source(sub-plan of csr_t)` as often as there are sub-plans, `der()`.  d_ft [csr_t.n_dst, H, F] and
    d_el [csr_t.n_dst, H] may be the head of larger allocations (the caller's)."""

    def __init__(self, csrv, csrt, el, er, ft, stats, G, out, H, F, neg_slope, spec, nscale, attn_drop, seg_len,
                 d_el, d_er, d_ft, dev):
        lib = _lib.lib()
        self.csrv, self.csrt, self.dev, self.H, self.F, self.seg_len = csrv, csrt, dev, H, F, seg_len
        self.plan_f, self.plan_b = csrv.plan(seg_len, need=True), csrt.plan(seg_len, need=True)
        nbytes = lib.stag_gat_bwd_workspace_bytes(self.plan_f["n_seg"], self.plan_b["n_seg"], H, F)
        # ONE forward-plan struct (and so one workspace) for every stage: the segment partials of step 2 and step 3
        self.pf, self._k1 = _plan_struct(csrv, seg_len, 1, nbytes, dev, plan_t=self.plan_f)
        self.scratch = torch.empty(lib.stag_gat_bwd_scratch_bytes(csrv.n_dst, csrv.n_edges, H) // 4, dtype=torch.float32,
                                   device=dev)
        self.drop = _gat_drop_struct(attn_drop)
        self.t = (el, er, ft, stats, G, out, nscale, d_el, d_er, d_ft)
        self.neg_slope, self.spec = float(neg_slope), spec
        self._keep = []

    def _call(self, plan_b, stages):
        pb, k = _plan_struct(self.csrt, self.seg_len, 1, 0, self.dev, plan_t=plan_b)
        self._keep.append(k)
        el, er, ft, stats, G, out, nscale, d_el, d_er, d_ft = self.t
        cs, ct = self.csrv.struct(), self.csrt.struct()
        with _lib.on_device(self.dev):
            rc = _lib.lib().stag_gat_bwd_stages(
                C.byref(cs), C.byref(self.pf), C.byref(ct), C.byref(pb), _lib.ptr(el), _lib.ptr(er), _lib.ptr(ft),
                _lib.ptr(stats), _lib.ptr(G), _lib.ptr(out), self.H, self.F, self.neg_slope, C.byref(self.spec),
                _lib.ptr(nscale), C.byref(self.drop) if self.drop is not None else None, _lib.ptr(d_el), _lib.ptr(d_er),
                _lib.ptr(d_ft), _lib.ptr(self.scratch), stages, _lib.stream_of(self.dev))
        _lib.check(rc, "stag_gat_bwd_stages")

    def rowdot(self):
        self._call(self.plan_b, _lib.GAT_BWD_ROWDOT)

    def source(self, plan_b=None):
        self._call(self.plan_b if plan_b is None else plan_b, _lib.GAT_BWD_SOURCE)

    def der(self):
        self._call(self.plan_b, _lib.GAT_BWD_DER)


def _gat_bwd_reordered(csrv, csrt, el, er, ft, stats, G, out, H, F, neg_slope, spec, nscale, want_dw, seg_len, dev,
                       attn_drop, want_dp):
    """The one-gather GAT backward on a graph of reorder_graph(noise="original").  stag_gat_bwd uses csr_t.nidx twice: as
    the noise index of an edge and as the slot its d s goes to, and step 3 (d er) expects a row's slots to be contiguous
    — on such a graph nidx names positions of the ORIGINAL graph, where they are contiguous in the original's rows.  So
    the stages run one at a time (stag_gat_bwd_stages): the row dots and the source pass on this graph, step 3 over the
    original graph's row pointers (no plan: a unit per row), and d er comes back through the permutation.  The stages
    return no [E, H] weight gradient and no parameter gradients."""
    if want_dw or want_dp:
        raise NotImplementedError("GAT weight / noise-parameter gradients on a graph reordered with noise='original': "
                                  "reorder with noise='own'")
    indptr0, perm = csrv.original_rows
    n = csrv.n_dst
    d_el = torch.empty((n, H), dtype=torch.float32, device=dev)
    d_er0 = torch.empty((n, H), dtype=torch.float32, device=dev)
    d_ft = torch.empty((n, H, F), dtype=torch.float32, device=dev)
    st = _GatBwdStages(csrv, csrt, el, er, ft, stats, G, out, H, F, neg_slope, spec, nscale, attn_drop, seg_len,
                       d_el, d_er0, d_ft, dev)
    st.rowdot()
    st.source()
    cs0 = _lib.Csr(n, n, csrv.n_edges, _lib.ptr(indptr0), _lib.ptr(csrv.indices), _lib.ptr(csrv.eid), None)
    p0 = _lib.Plan.from_buffer_copy(st.pf)
    p0.n_units = p0.n_long = p0.n_seg = 0          # step 3 then takes a row per thread from cs0.indptr
    pb, _k = _plan_struct(csrt, seg_len, 1, 0, dev, plan_t=st.plan_b)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_gat_bwd_stages(
            C.byref(cs0), C.byref(p0), C.byref(csrt.struct()), C.byref(pb), _lib.ptr(el), _lib.ptr(er), _lib.ptr(ft),
            _lib.ptr(stats), _lib.ptr(G), _lib.ptr(out), H, F, float(neg_slope), C.byref(spec), _lib.ptr(nscale),
            C.byref(st.drop) if st.drop is not None else None, _lib.ptr(d_el), _lib.ptr(d_er0), _lib.ptr(d_ft),
            _lib.ptr(st.scratch), _lib.GAT_BWD_DER, _lib.stream_of(dev))
    _lib.check(rc, "stag_gat_bwd_stages")
    return d_el, d_er0[perm], d_ft, None


_GAT_VI_FUSED = True       # vi=True parameter gradients inside the GAT kernels (stag_gat_bwd_dp) | materialised [E, H] weights
_GAT_BWD_FUSED = True      # tools/bench_configs.py --gat-old-bwd flips it for A/B runs
_GAT_BWD_ONE_GATHER = True  # stag_gat_bwd (one gather of [H*F] rows) | stag_gat_bwd_two_pass; --gat-two-pass for A/B


def gat_aggregate(graph, el, er, ft, neg_slope=0.2, weight=None, want_attn=False,
                  seg_len=DEFAULT_SEG_LEN, _gathered=False, attn_fn=None, attn_drop=None):
    """Fused noisy-logit edge softmax + aggregation (stag/zoo/gat.py:114-126).
    el: [N,H], er: [N,H], ft: [N,H,F]; weight: None | [E,H] tensor | EdgeNoise(dn=H).
    attn_drop: (p, seed, offset[, epoch]) — attention dropout (stag/zoo/gat.py:122) inside the kernels, its mask
    from its own Philox stream (attn_drop_fusable() says whether the shape has that form); attn_fn: any function of
    a[E, H] between the softmax and the sum, on the composed path.
    On a node-range shard the inputs are this rank's rows and the call includes the exchange.
    An EdgeNoise with n_samples > 1 (StagLayer.forward_mc) yields [n_samples, N, H, F]: gat_aggregate_mc."""
    if isinstance(weight, EdgeNoise) and weight.n_samples > 1:
        if want_attn or attn_fn is not None or attn_drop is not None:
            raise NotImplementedError("Monte-Carlo samples (n_samples > 1) without attention values or dropout only")
        import copy
        one = copy.copy(weight)
        one.n_samples = 1
        return gat_aggregate_mc(graph, el, er, ft, neg_slope, one, weight.n_samples, weight.offset_stride,
                                seg_len=seg_len, _gathered=_gathered)
    if getattr(graph, "is_shard", False) and not _gathered:
        if attn_fn is not None:
            raise NotImplementedError("a function of a[E, H] (attn_fn) is not partitioned: pass attn_drop")
        return graph.gat_aggregate(el, er, ft, neg_slope, weight, seg_len=seg_len, want_attn=want_attn,
                                   attn_drop=attn_drop)
    noise = weight if isinstance(weight, EdgeNoise) else None
    w = weight if torch.is_tensor(weight) else None
    if w is not None and w.shape[0] != graph.number_of_edges():
        raise AssertionError("edge_weight.shape[0] != number_of_edges")
    H, F = ft.shape[1], ft.shape[2]
    live = None
    if (noise is not None and noise.grad_params is not None and torch.is_grad_enabled()
            and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params)):
        # vi=True (stag/layers.py:123-124 through stag/zoo/gat.py:117-119).  Scalar / per-head parameters without
        # in-norm stay in the kernels: the forward draws from the descriptor, the one-gather backward redoes the draw
        # with its derivatives and returns the finished parameter gradients (stag_gat_bwd_dp) — no [E, H] tensor.
        # Otherwise the H-wide weights are formed from the kernel's standard draw and the live parameters ([E, H]:
        # 37 MB at cfg5), enter as explicit weights, the edge pass returns dw[E, H] and autograd does the affine map.
        # (the preconditions of stag_gat_bwd_dp mirrored here — channel shards' chunk_base, the plan's segment length
        # inside gat_cooperative_shape — so that a shape it refuses takes the materialised route below instead of
        # failing in the middle of a backward pass)
        if (_GAT_VI_FUSED and not noise.in_norm and noise.param_mode <= _lib.PARAM_PER_CHANNEL and ft.is_cuda
                and gat_cooperative_shape(H, F, seg_len) and _GAT_BWD_FUSED and not want_attn
                and int(getattr(noise, "chunk_base", 0) or 0) == 0):
            live = tuple(torch.as_tensor(p, dtype=torch.float32, device=ft.device) for p in noise.grad_params)
        else:
            w, noise = noise.materialize(), None
    lph = F // 4
    # the fused kernels: H*F <= 256 always; up to 1024 channels on the workgroup-cooperative forms (F % 4 == 0,
    # H <= 16, the default plan); the backward wants F/4 a power of two (<= 64)
    wide_ok = gat_cooperative_shape(H, F, seg_len)
    bwd_ok = wide_ok and _GAT_BWD_FUSED and (_GAT_BWD_ONE_GATHER or (lph & (lph - 1)) == 0)
    old_bwd_ok = F % 4 == 0 and lph <= 64 and (lph & (lph - 1)) == 0 and H * F <= 256     # stag_gat_bwd_edge + aggregations
    if (attn_fn is not None or H > 64 or H * F > (1024 if wide_ok else 256)
            or torch.is_grad_enabled() and not (bwd_ok or old_bwd_ok)):
        if getattr(graph, "is_shard", False):
            raise NotImplementedError("the composed GAT path (attention dropout, H > 64 or H*F > 256) is not partitioned")
        if attn_drop is not None:
            raise NotImplementedError("attn_drop rides in the fused kernels only: check attn_drop_fusable()")
        return _gat_composed(graph, el, er, ft, neg_slope, noise, w, want_attn, seg_len, attn_fn)
    if attn_drop is not None and not attn_drop_fusable(H, F, seg_len, want_attn):
        raise NotImplementedError("attn_drop rides in the fused kernels only: check attn_drop_fusable()")
    if live is not None:
        return _GatAggregate.apply(el, er, ft, None, graph, noise, neg_slope, want_attn, seg_len, attn_drop, *live)
    return _GatAggregate.apply(el, er, ft, w, graph, noise, neg_slope, want_attn, seg_len, attn_drop)


def gat_aggregate_mc(graph, el, er, ft, neg_slope, noise, n_samples, offset_stride=1, seg_len=DEFAULT_SEG_LEN,
                     _gathered=False):
    """[n_samples, N, H, F]: sample s == gat_aggregate(graph, el, er, ft, neg_slope, noise at offset + s *
    offset_stride), bit for bit.  The reference's Monte-Carlo loops (stag/models.py:45-55, :67-68) on a first GAT
    layer: el, er and ft are the same for every sample, so the fused form (stag_gat_fwd_mc) gathers each ft row once
    per pass of up to 4 samples and only the H-wide draws, the softmax and the weighted sums repeat.  Under autograd
    (el / er / ft carry a gradient) the forward is still batched and the backward is the loop's per-sample one-gather
    backward (_GatAggregateMC).  Shards, in-norm, explicit / per-edge parameters, live `vi=True` parameters under
    autograd, shapes outside the cooperative kernels, CPU tensors and n_samples == 1 take the stack of n_samples
    ordinary gat_aggregate calls."""
    import copy

    def one(s):
        nz = copy.copy(noise)
        nz.offset = (noise.offset + s * offset_stride) & _MASK64
        nz.n_samples = 1
        return gat_aggregate(graph, el, er, ft, neg_slope, nz, seg_len=seg_len, _gathered=_gathered)

    if not isinstance(noise, EdgeNoise):
        raise TypeError("gat_aggregate_mc draws its samples from an EdgeNoise")
    H, F = ft.shape[1], ft.shape[2]
    live = (noise.grad_params is not None and torch.is_grad_enabled()
            and any(torch.is_tensor(p) and p.requires_grad for p in noise.grad_params))
    fused = (n_samples > 1 and not (getattr(graph, "is_shard", False) and not _gathered) and ft.is_cuda
             and noise.kind >= _lib.NOISE_NORMAL and noise.param_mode <= _lib.PARAM_PER_CHANNEL and not noise.in_norm
             and not live and int(getattr(noise, "chunk_base", 0) or 0) == 0 and gat_cooperative_shape(H, F, seg_len)
             and graph.csr.n_dst > 0)
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (el, er, ft))
    if fused and needs_grad:
        fused = _GAT_BWD_FUSED and _GAT_BWD_ONE_GATHER     # the backward is the one-gather kernels' (per sample)
    if not fused:
        if n_samples == 1:
            return one(0).unsqueeze(0)
        if ft.dtype in _HALF_DTYPES:
            ft = ft.float()        # a Monte-Carlo batch keeps the cast route (gat_half_rows_why_not): widened once for the loop
        return torch.stack([one(s) for s in range(n_samples)], 0)
    if needs_grad:
        return _GatAggregateMC.apply(el, er, ft, graph, noise, int(n_samples), int(offset_stride), float(neg_slope),
                                     seg_len)
    out, _ = _gat_fwd_mc_raw(graph.csr, _f32c(el), _f32c(er), _f32c(ft), noise, int(n_samples), int(offset_stride),
                             float(neg_slope), seg_len, want_stats=False)
    return out


def _gat_fwd_mc_raw(csrv, el, er, ft, noise, n_samples, offset_stride, neg_slope, seg_len, want_stats):
    """One stag_gat_fwd_mc call: (out [S, n_dst, H, F], stats [S, n_dst, 2H] or None)."""
    H, F = ft.shape[1], ft.shape[2]
    dev = _lib.require_device(el, er, ft, csrv.indptr)
    plan_t = csrv.plan(seg_len, need=True)       # the cooperative kernels want the plan's unit batches
    if _torch_ext.available():      # the dispatcher op (csrc/torch_ext.cpp: stag::gat_fwd_mc), same library call
        out, stats = torch.ops.stag.gat_fwd_mc(*csrv.torch_args(), *_gat_plan_args(csrv, plan_t, dev, H * F), el, er, ft,
                                               float(neg_slope), *noise.torch_args(), int(n_samples), int(offset_stride),
                                               bool(want_stats))
        return out, (stats if want_stats else None)
    out = torch.empty((n_samples, csrv.n_dst, H, F), dtype=torch.float32, device=dev)
    stats = torch.empty((n_samples, csrv.n_dst, 2 * H), dtype=torch.float32, device=dev) if want_stats else None
    nbytes = _lib.lib().stag_gat_fwd_mc_workspace_bytes(plan_t["n_seg"], H, F, n_samples)
    plan_c, _keep = _plan_struct(csrv, seg_len, 1, nbytes, dev, plan_t=plan_t, gat_width=H * F)
    cs, spec = csrv.struct(), noise.spec()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_gat_fwd_mc(C.byref(cs), C.byref(plan_c), _lib.ptr(el), _lib.ptr(er), _lib.ptr(ft), H, F,
                                        float(neg_slope), C.byref(spec), n_samples, offset_stride, _lib.ptr(out),
                                        csrv.n_dst * H * F, _lib.ptr(stats), csrv.n_dst * 2 * H, _lib.stream_of(dev))
    _lib.check(rc, "stag_gat_fwd_mc")
    return out, stats


class _GatAggregateMC(torch.autograd.Function):
    """S Monte-Carlo samples of one GAT aggregation with gradients w.r.t. el, er and ft (a first GAT layer without
    dropout trained with n_samples_training > 1, stag/models.py:67-68): the forward is the batched stag_gat_fwd_mc
    (one gather of the ft rows per pass), the backward the loop's per-sample one-gather backward (stag_gat_bwd with
    sample s's statistics, output and offset), d el / d er / d ft summed over the samples."""

    @staticmethod
    def forward(ctx, el, er, ft, graph, noise, n_samples, stride, neg_slope, seg_len):
        el, er, ft = _f32c(el), _f32c(er), _f32c(ft)
        out, stats = _gat_fwd_mc_raw(graph.csr, el, er, ft, noise, n_samples, stride, neg_slope, seg_len, want_stats=True)
        ctx.graph, ctx.noise, ctx.S, ctx.stride, ctx.neg_slope, ctx.seg_len = (_owner(graph), noise, n_samples, stride,
                                                                                neg_slope, seg_len)
        ctx.save_for_backward(el, er, ft, out, stats)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        import copy
        el, er, ft, out, stats = ctx.saved_tensors
        graph = ctx.graph
        H, F = ft.shape[1], ft.shape[2]
        G = _f32c(grad_out)
        d_el = d_er = d_ft = None
        for s in range(ctx.S):
            nz = copy.copy(ctx.noise)
            nz.offset = (ctx.noise.offset + s * ctx.stride) & _MASK64
            nz.n_samples = 1
            r = _gat_bwd_fused(graph.csr, graph.csr_t, el, er, ft, stats[s], G[s], out[s], H, F, ctx.neg_slope,
                               nz.spec(), None, False, ctx.seg_len, ft.device, spec_tensors=(nz.p0, nz.p1, nz.epoch))
            if r is None:
                raise NotImplementedError("the batched GAT samples need the one-gather backward (stag_gat_bwd)")
            d_el = r[0] if d_el is None else d_el + r[0]
            d_er = r[1] if d_er is None else d_er + r[1]
            d_ft = r[2] if d_ft is None else d_ft + r[2]
        return (d_el if ctx.needs_input_grad[0] else None, d_er if ctx.needs_input_grad[1] else None,
                d_ft if ctx.needs_input_grad[2] else None, None, None, None, None, None, None)


def _gat_composed(graph, el, er, ft, neg_slope, noise, w, want_attn, seg_len, attn_fn=None):
    """The same layer outside the fused kernel's shape limits (one wave spans the H*F row: H <= 64,
    H*F <= 256; its backward wants F/4 a power of two): logits and the edge softmax as torch ops over
    [E, H] (segment max by scatter-reduce), the sums and the weighted aggregation on the aggregation
    kernel, which tiles any width.  Device-only like everything else; several passes instead of one."""
    N, H, F = ft.shape
    _, dst = graph.edges()
    dst = dst.long()
    e = torch.nn.functional.leaky_relu(gather_rows(graph, el, "src") + gather_rows(graph, er, "dst"), neg_slope)
    if noise is not None:
        w = noise.materialize()              # [E, H], relu / in-norm applied (stag/zoo/gat.py:117-119)
    if w is not None:
        e = e * (w if w.dim() == 2 else w.reshape(w.shape[0], -1))
    m = torch.full((N, H), float("-inf"), dtype=e.dtype, device=e.device)
    m = m.scatter_reduce(0, dst.unsqueeze(1).expand(-1, H), e.detach(), reduce="amax", include_self=True)
    p = torch.exp(e - m[dst])
    l = aggregate(graph, torch.ones(1, H, device=e.device), p, seg_len=seg_len, _broadcast_x=True)   # sum_in p
    a = p / gather_rows(graph, l, "dst")
    if attn_fn is not None:                  # e.g. attention dropout (stag/zoo/gat.py:122)
        a = attn_fn(a)
    out = aggregate(graph, ft.reshape(N, H * F), a.repeat_interleave(F, dim=1), seg_len=seg_len)
    out = out.reshape(N, H, F)
    return (out, a.detach()) if want_attn else out
