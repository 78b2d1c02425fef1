"""The per-edge gradient kernels, the max reducer's backward and count, and the small reductions across the float range.

tests/test_gpu_value_range.py takes the aggregation entry points through four groups (A power-of-two scaling, B
subnormals, C non-finite values, D parameter edges); this module takes the entry points it never reached through the same
groups, on the same fixture graph (tests/value_range_cases.py), at D = 6, 8 and 264 and seg_len 4 and 64:
  stag_agg_bwd_w (no spec, one derivative, both; [E, D] tables and, with reduce_k, [E, 1] tables), stag_agg_bwd_w_mc (seven
  samples: passes of 4, 2 and 1, the later ones reading back what the earlier ones stored), stag_agg_bwd_pedge (dx, dp0, dp1),
  stag_agg_max_fwd's cnt and stag_agg_max_bwd (dx, dw, dp0_rows, dp1_rows), stag_coldot, stag_segment_reduce, and
  stag_noise_materialize with in-norm.
Every comparison is against a float64 numpy statement of the header's formula (vc.grad_reference, vc.max_bwd_reference) on
the oracle's weights and derivatives, drawn under util.hw_normals: the device's, bit for bit.  The max backward takes out
and cnt from the kernel's own forward, which is itself compared with vc.max_fwd_reference.  tests/test_value_range_host.py
holds, without a GPU, what this module relies on: the scaling margins of group A, the r and f of group B's bars, the
affected sets of group C and their memory neighbours, the planted duplicates of group D.

The three gradient entry points share one layout on the view "t" (vc, "ONE LAYOUT"): x is the table an edge gathers,
g_all the rows the units own.  In stag_agg_bwd_pedge's own naming x is `g` and g_all[0] is `x`.

What is pinned for the max backward (group C): with x[U] poisoned, the elements that may change are dx[U, k], dx[u', k]
(and the dp rows) of every u' that shares a destination with U, and dw of every edge that enters such a destination (the
edges that leave U and their row-mates), k poisoned — that destination's out and cnt changed, so an edge that was
maximal there may no longer be; everything else keeps its bits.  With g[V0] poisoned and out / cnt clean, a source
whose edge into V0 is maximal receives the infinity, one whose edge is not stays finite and bit-identical: [m == out] is a
select, not a product.  stag_agg_bwd_pedge's dx follows the pinned Kahan rule of the forward kernels: plain sums report
the reference's signed infinity or NaN, Kahan units and long rows NaN."""
import time

import numpy as np
import pytest
import torch

import value_range_cases as vc
from test_gpu_value_range import _Errs, _Noise, _bits, _dev, _rig
from util import TOL, hw_normals

pytestmark = pytest.mark.gpu
_WORST = {}
_OG = {}


@pytest.fixture(autouse=True)
def _ctypes_front_end(monkeypatch, request):
    from stag_amd import _torch_ext
    monkeypatch.setattr(_torch_ext, "available", lambda: False)
    t0 = time.perf_counter()
    yield
    print(f"WALL {request.node.name}: {time.perf_counter() - t0:.2f} s")
    for k in sorted(_WORST):
        print(f"WORST {k}: {_WORST[k]:.3f} of the bar")
    _WORST.clear()


def _og_view(rig):
    """The transpose of the view "t" on the device: rows are the gathered table's rows (the sources of the max forward),
    nidx its own positions — the counters the forward on "t" drew at (ogt.nidx)."""
    if "v" not in _OG:
        from stag_amd.graph import CsrView
        og, dev = rig.st.og, rig.dev
        assert np.array_equal(np.sort(rig.st.ogt.nidx), np.arange(vc.N_EDGES))
        v = CsrView(vc.N, vc.N, _dev(og.indptr, dev), _dev(og.indices, dev), eid=_dev(og.eid, dev),
                    nidx=_dev(np.arange(vc.N_EDGES, dtype=np.int32), dev))
        for seg in vc.SEGS:
            plan = v.plan(seg, need=True)
            plan["xcd_decided"] = True
        assert v.plan(4)["n_long"] > 0, "some source rows are cut at seg_len 4"
        _OG["v"] = v
    return _OG["v"]


def _note(key, ratio):
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


def _match(errs, key, what, got, ref, scale=1.0, kind="rows", kahan=None, c=1.0):
    """got against the float64 reference: NaN where it is NaN, the same signed infinity where it is infinite (NaN in the
    elements of `kahan`), and the finite elements at util.TOL after both are divided by scale and by vc.out_scale.  c: the
    power of two the launch's input was scaled by and the reference's was not — got is divided by it first, in float64."""
    got, ref = np.asarray(got, np.float64) / c / scale, np.asarray(ref, np.float64) / scale
    nonfin = ~np.isfinite(ref)
    if kahan is not None and (nonfin & kahan).any():
        if not np.isnan(got[nonfin & kahan]).all():
            errs.append(f"{what}: Kahan sums over a non-finite term are pinned to NaN")
        nonfin_plain = nonfin & ~kahan
    else:
        nonfin_plain = nonfin
    if not np.array_equal(np.isnan(got[nonfin_plain]), np.isnan(ref[nonfin_plain])) or not np.array_equal(
            got[nonfin_plain][np.isinf(ref[nonfin_plain])], ref[nonfin_plain][np.isinf(ref[nonfin_plain])]):
        errs.append(f"{what}: not the reference's NaN / signed infinity where the reference is not finite")
    fin = ~nonfin
    if not np.isfinite(got[fin]).all():
        errs.append(f"{what}: {int((~np.isfinite(got[fin])).sum())} non-finite elements where the reference is finite")
        return
    sc = vc.out_scale(kind, ref)
    err = np.abs(got[fin] - ref[fin]) / sc / (1.0 + np.abs(ref[fin]) / sc)
    worst = float(err.max()) if err.size else 0.0
    _note(key, worst / TOL)
    if worst > TOL:
        errs.append(f"{what}: scaled error {worst:.3e} > {TOL:.1e}")


def _close_grad(errs, group, gc, got, refs, what, c=1.0):
    for (name, _), kind, g, r, norm in zip(gc.outputs(), gc.kinds(), got, refs, gc.norms()):
        _match(errs, f"{group} {gc.entry} {name}", f"{what} {name}", g, r, norm, kind, c=c)


def _launch(rig, gc, D, seg, x, g_all, spec=None):
    """One launch of a gradient case on the view "t": x [N, D] and g_all [S, N, D] device tensors."""
    from stag_amd import ops
    V, t, dev = rig.views["t"], rig.tables(D), rig.dev
    sp = spec if spec is not None else gc.spec
    ss, ds = (t["ss"] if gc.ss else None), t["ds"]
    if gc.entry == "bwd_w":
        if gc.mode == "plain":
            outs = [ops._bwd_w_raw(V, x, g_all[0], D, ss, spec=None, reduce_k=gc.reduce_k, seg_len=seg)]
        elif gc.mode == "both":
            outs = list(ops._bwd_w_raw(V, x, g_all[0], D, ss, spec=sp.c(dev), reduce_k=gc.reduce_k, both=True, seg_len=seg))
        else:
            outs = [ops._bwd_w_raw(V, x, g_all[0], D, ss, spec=sp.c(dev, deriv=gc.mode), reduce_k=gc.reduce_k, seg_len=seg)]
    elif gc.entry == "bwd_w_mc":
        outs = list(ops._bwd_w_mc_raw(V, x, g_all[:gc.S].contiguous(), D, ss, ds, sp.c(dev), gc.S, vc.GRAD_STRIDE,
                                      reduce_k=gc.reduce_k, seg_len=seg))
    else:
        outs = list(ops._agg_bwd_pedge_raw(V, x, g_all[0], D, sp.c(dev), ss, ds, seg))
    assert len(outs) == len(gc.outputs())
    return [o.cpu().numpy() for o in outs]


def _coldot(x, t0, t1):
    from stag_amd import ops
    o0, o1 = ops.coldot(x, t0, t1)
    return [o0.cpu().numpy(), o1.cpu().numpy()]


def _segred(x, offs, mean, dev):
    from stag_amd import _lib, ops
    return ops._segment_reduce_raw(x, offs, _lib.REDUCE_MEAN if mean else _lib.REDUCE_SUM, dev).cpu().numpy()


def _segred_ref(x, offs, mean):
    x = np.asarray(x, np.float64)
    out = np.zeros((len(offs) - 1, x.shape[1]))
    with np.errstate(all="ignore"):
        for b in range(len(offs) - 1):
            out[b] = x[offs[b]:offs[b + 1]].sum(0) / (max(offs[b + 1] - offs[b], 1) if mean else 1)
    return out


def _max_spec_weights(O, st, spec, D, deriv=0):
    return None if spec.kind == "none" else vc.weights(O, st, vc._wcase(spec), D, deriv=deriv)


def _max_fwd(rig, spec, D, seg, x):
    from stag_amd import ops
    out, cnt = ops._max_fwd_raw(rig.views["t"], x, D, spec.c(rig.dev), seg, True)
    return out, cnt


def _max_bwd(rig, spec, D, seg, x, out, cnt, g):
    """(dx, dw | None, dp0_rows | None, dp1_rows | None) as numpy arrays; dw for EXPLICIT, the dp rows for NORMAL | UNIFORM"""
    from stag_amd import ops
    outs = ops._max_bwd_raw(_og_view(rig), x, out, cnt, g, D, spec.c(rig.dev), seg, True, spec.kind == "explicit",
                            spec.kind in ("normal", "uniform"))
    return [None if o is None else o.cpu().numpy() for o in outs]


def _max_check_bwd(errs, group, rig, spec, D, seg, x_np, g_np, what, x=None, out=None, cnt=None):
    """forward (out, cnt against the restatement, bit for bit) and backward (against the loop over the header's lines on the
    kernel's own out and cnt, at TOL); returns the device out, cnt and the backward's outputs"""
    O, st, dev = rig.O, rig.st, rig.dev
    W = _max_spec_weights(O, st, spec, D)
    x = _dev(x_np, dev) if x is None else x
    if out is None:
        out, cnt = _max_fwd(rig, spec, D, seg, x)
        _, ro, rc = vc.max_fwd_reference(st, x_np, W)
        if not np.array_equal(_bits(out.cpu().numpy()), _bits(ro)):
            errs.append(f"{what}: out is not the restatement's, bit for bit")
        if not np.array_equal(cnt.cpu().numpy(), rc):
            errs.append(f"{what}: cnt is not the number of messages equal to out")
    d = [_max_spec_weights(O, st, spec, D, dv) for dv in (1, 2)] if spec.kind in ("normal", "uniform") else [None, None]
    refs = vc.max_bwd_reference(st, x_np, W, out.cpu().numpy(), cnt.cpu().numpy(), g_np, *d)
    got = _max_bwd(rig, spec, D, seg, x, out, cnt, _dev(g_np, dev))
    for name, gt, rf in zip(("dx", "dw", "dp0_rows", "dp1_rows"), got, refs):
        if gt is not None:
            _match(errs, f"{group} max_bwd {name}", f"{what} {name}", gt, rf)
    return out, cnt, got, refs


# ---- A. power-of-two scaling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", vc.WIDTHS)
def test_A_gradients_power_of_two_scaling(dev, oracle, D):
    """out(c x) == c out(x) and out(c g) == c out(g) bit for bit, c = 2^-100, 2^-60, 2^100, one input at a time, and the
    scaled launch over c within 1e-5 of the float64 reference: stag_agg_bwd_w (no spec, deriv 1, deriv 2, both; [E, D] and,
    with reduce_k, [E, 1] Normal-p1_log and Uniform tables), stag_agg_bwd_w_mc at 7 samples, stag_agg_bwd_pedge (dx scales
    with the gathered table and does not move with the owned one).  Also, at c = 1: dp0 / dp1 of stag_agg_bwd_pedge are
    stag_agg_bwd_w_mc's at one sample and dx is stag_agg_fwd_mc_pedge's, bit for bit."""
    from stag_amd import _lib, ops
    rig, GT, errs = _rig(oracle, dev), vc.grad_tables(D), _Errs()
    st, t, V = rig.st, rig.tables(D), rig.views["t"]
    xs = {c: _dev(GT.x * np.float32(c), dev) for c in (1.0,) + vc.SCALES}
    gs = {c: _dev(GT.g_all * np.float32(c), dev) for c in (1.0,) + vc.SCALES}
    ran = 0
    with hw_normals(oracle, dev):
        for gc in vc.cases_grad_A(D):
            refs = vc.grad_reference(oracle, st, gc, D, GT.x, GT.g_all, GT.ss, GT.ds)
            for seg in vc.SEGS:
                what = f"D={D} {gc.name} seg_len={seg}"
                base = _launch(rig, gc, D, seg, xs[1.0], gs[1.0])
                _close_grad(errs, "A", gc, base, refs, what)
                for c in vc.SCALES:
                    cf = np.float32(c)
                    got = _launch(rig, gc, D, seg, xs[c], gs[1.0])
                    errs.same_bits(got, [b * cf for b in base], f"{what} c={c:.1e}: out(c x) vs c out(x)")
                    _close_grad(errs, "A", gc, got, refs, f"{what} c={c:.1e} on x", c=c)
                    got = _launch(rig, gc, D, seg, xs[1.0], gs[c])
                    want = [b if d == 0 else b * cf for (_, d), b in zip(gc.outputs(), base)]
                    errs.same_bits(got, want, f"{what} c={c:.1e}: out(c g) vs c out(g)")
                    for (name, d), kind, g_, r_, norm in zip(gc.outputs(), gc.kinds(), got, refs, gc.norms()):
                        _match(errs, f"A {gc.entry} {name}", f"{what} c={c:.1e} on g {name}", g_, r_, norm, kind,
                               c=1.0 if d == 0 else c)
                    ran += 2
                if gc.entry == "bwd_pedge":
                    one = vc.GradCase("one sample", "bwd_w_mc", gc.spec, S=1)
                    errs.same_bits(base[1:], _launch(rig, one, D, seg, xs[1.0], gs[1.0]),
                                   f"{what}: dp0 / dp1 vs stag_agg_bwd_w_mc at one sample")
                    mc = ops._agg_fwd_mc_pedge_raw(V, xs[1.0], _Noise(gc.spec.c(dev)), 1, 1, _lib.REDUCE_SUM, t["ss"], t["ds"], seg)
                    errs.same_bits(base[:1], [mc[0].cpu().numpy()], f"{what}: dx vs stag_agg_fwd_mc_pedge at one sample")
    assert ran == len(vc.cases_grad_A(D)) * len(vc.SEGS) * len(vc.SCALES) * 2 and ran > 0
    errs.done()


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_A_max_backward_and_reductions_scaling(dev, oracle, D):
    """stag_agg_max_fwd on c x gives c out and the same cnt; with that out, stag_agg_max_bwd's dx scales with g, dw
    (EXPLICIT) with x and with g, dp0_rows / dp1_rows with g, bit for bit.  stag_coldot (n = 300 and a row count past the
    second grid-stride trip) and stag_segment_reduce (sum, mean): c on x, bit for bit; all against float64 at TOL."""
    rig, GT, T, errs = _rig(oracle, dev), vc.grad_tables(D), vc.tables(D), _Errs()
    g_np = GT.g_all[0]
    with hw_normals(oracle, dev):
        for name, spec in vc.max_specs_A(D).items():
            for seg in vc.SEGS:
                what = f"D={D} max {name} seg_len={seg}"
                out, cnt, base, _ = _max_check_bwd(errs, "A", rig, spec, D, seg, GT.x, g_np, what)
                for c in vc.SCALES:
                    cf = np.float32(c)
                    xc = GT.x * cf
                    oc, cc = _max_fwd(rig, spec, D, seg, _dev(xc, dev))
                    errs.same_bits([oc.cpu().numpy()], [out.cpu().numpy() * cf], f"{what} c={c:.1e}: out(c x) vs c out(x)")
                    if not torch.equal(cc, cnt):
                        errs.append(f"{what} c={c:.1e}: cnt moved with the scale of x")
                    # c on g, the clean x, out and cnt
                    got = _max_bwd(rig, spec, D, seg, _dev(GT.x, dev), out, cnt, _dev(g_np * cf, dev))
                    pairs = [(g_, b * cf) for g_, b in zip(got, base) if g_ is not None]
                    errs.same_bits([p[0] for p in pairs], [p[1] for p in pairs], f"{what} c={c:.1e}: bwd(c g) vs c bwd(g)")
                    # c on x with the matching out: dw scales, dx does not move
                    if spec.kind == "explicit":
                        got = _max_bwd(rig, spec, D, seg, _dev(xc, dev), oc, cc, _dev(g_np, dev))
                        errs.same_bits(got[:2], [base[0], base[1] * cf], f"{what} c={c:.1e}: dx, dw under c x")
        # stag_coldot, stag_segment_reduce
        for n in (vc.COLDOT_N, vc.coldot_big_n(D)):
            x, t0, t1 = (vc.away_table(70 + i + n % 7, (n, D)) for i in range(3))
            refs = [(x.astype(np.float64) * t.astype(np.float64)).sum(0) for t in (t0, t1)]
            t0d, t1d = _dev(t0, dev), _dev(t1, dev)
            base = _coldot(_dev(x, dev), t0d, t1d)
            scale = max(1.0, float(np.abs(refs[0]).max()), float(np.abs(refs[1]).max()))
            for c in (1.0,) + vc.SCALES:
                got = _coldot(_dev(x * np.float32(c), dev), t0d, t1d)
                errs.same_bits(got, [b * np.float32(c) for b in base], f"D={D} coldot n={n} c={c:.1e}: out(c x) vs c out(x)")
                for i in (0, 1):
                    _match(errs, "A coldot", f"D={D} coldot n={n} c={c:.1e} out{i}", got[i], refs[i], scale, c=c)
        offs = _dev(vc.SEGMENT_OFFSETS, dev)
        for mean in (False, True):
            ref = _segred_ref(GT.x, vc.SEGMENT_OFFSETS, mean)
            base = _segred(_dev(GT.x, dev), offs, mean, dev)
            for c in (1.0,) + vc.SCALES:
                got = _segred(_dev(GT.x * np.float32(c), dev), offs, mean, dev)
                errs.same_bits([got], [base * np.float32(c)], f"D={D} segment_reduce mean={mean} c={c:.1e}")
                _match(errs, "A segment_reduce", f"D={D} segment_reduce mean={mean} c={c:.1e}", got, ref, c=c)
    errs.done()


# ---- B. subnormals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", vc.WIDTHS)
def test_B_gradients_subnormals(dev, oracle, D):
    """Tables of 2^-149: stag_agg_bwd_w without a spec and without ss, g of small integers: dw == g 2^-149 exactly, and
    with reduce_k the sum over k exactly.  x = randn 2^-130 under Normal(1, 0.5): stag_agg_bwd_w (both), stag_agg_bwd_w_mc at
    3 samples, stag_agg_bwd_pedge at 1e-5 |ref| + r 2^-149 f (vc.grad_subnormal_bars: r roundings on the element's path, f
    the largest magnitude later multiplied into it; proved on an fp32 emulation by the host test)."""
    rig, GT, T, errs = _rig(oracle, dev), vc.grad_tables(D), vc.tables(D), _Errs()
    st = rig.st
    tiny = _dev(np.full((vc.N, D), vc.TINY, np.float32), dev)
    gint = _dev(GT.gint[None], dev)
    for rk in (False, True):
        gc = vc.GradCase("stag_agg_bwd_w no spec", "bwd_w", None, "plain", reduce_k=rk, ss=False)
        (want,) = vc.grad_reference(oracle, st, gc, D, np.full((vc.N, D), vc.TINY, np.float32), GT.gint[None], GT.ss, GT.ds)
        for seg in vc.SEGS:
            (got,) = _launch(rig, gc, D, seg, tiny, gint)
            if not np.array_equal(got.astype(np.float64), want):
                errs.append(f"D={D} reduce_k={rk} seg_len={seg}: not g 2^-149 (max |diff| "
                            f"{np.abs(got - want).max() / vc.TINY:.1f} x 2^-149, {int((got == 0).sum())} zeros against "
                            f"{int((want == 0).sum())})")
    xs_np = T.x * np.float32(2.0 ** -130)
    xs, gr = _dev(xs_np, dev), _dev(GT.grand, dev)
    ran = 0
    with hw_normals(oracle, dev):
        for gc in vc.cases_grad_B(D):
            refs = vc.grad_reference(oracle, st, gc, D, xs_np, GT.grand, GT.ss, GT.ds)
            bars = vc.grad_subnormal_bars(oracle, st, gc, D, GT.grand, GT.ds, refs)
            for seg in vc.SEGS:
                got = _launch(rig, gc, D, seg, xs, gr)
                for (name, _), g_, r_, bar in zip(gc.outputs(), got, refs, bars):
                    over = float((np.abs(g_.astype(np.float64) - r_) / bar).max())
                    _note(f"B {gc.entry} {name} (subnormal bar)", over)
                    if not over <= 1.0:
                        errs.append(f"D={D} {gc.name} seg_len={seg} {name}: {over:.2f} x the subnormal bar "
                                    f"({int((g_ == 0).sum())} zeros against {int((r_ == 0).sum())})")
                ran += 1
    assert ran == 5 * len(vc.SEGS)
    errs.done()


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_B_max_and_reductions_subnormals(dev, oracle, D):
    """x of 2^-149: stag_agg_max_fwd (NONE) gives out == 2^-149 and cnt == indeg; stag_agg_max_bwd with g = indeg 2^-149
    gives dx[u] == outdeg(u) 2^-149; stag_coldot and stag_segment_reduce give exact multiples.  x = randn 2^-130 under
    Normal(1, 0.5): the max backward against the restatement (its outputs are O(1): what is subnormal is the comparison
    m == out).  Ties: x of five values times 2^-149, NONE, g = cnt: every tied edge contributes exactly 1 to dx, so dx is
    the number of tied out-edges of a source, and the ties into a row number cnt."""
    rig, GT, T, errs = _rig(oracle, dev), vc.grad_tables(D), vc.tables(D), _Errs()
    st = rig.st
    none = vc.Spec("none")
    tiny_np = np.full((vc.N, D), vc.TINY, np.float32)
    outdeg = np.bincount(st.ogt.indices, minlength=vc.N)
    has = (st.indeg > 0)[:, None]
    xt_np = GT.xint * np.float32(vc.TINY)
    for seg in vc.SEGS:
        out, cnt = _max_fwd(rig, none, D, seg, _dev(tiny_np, dev))
        if not np.array_equal(out.cpu().numpy().astype(np.float64), np.where(has, np.float64(vc.TINY), 0.0) * np.ones((1, D))):
            errs.append(f"D={D} seg_len={seg}: out is not 2^-149")
        if not np.array_equal(cnt.cpu().numpy(), st.indeg[:, None] * np.ones((1, D), np.int64)):
            errs.append(f"D={D} seg_len={seg}: cnt is not indeg")
        g_np = (st.indeg[:, None] * np.float64(vc.TINY) * np.ones((1, D))).astype(np.float32)
        dx = _max_bwd(rig, none, D, seg, _dev(tiny_np, dev), out, cnt, _dev(g_np, dev))[0]
        if not np.array_equal(dx.astype(np.float64), outdeg[:, None] * np.float64(vc.TINY) * np.ones((1, D))):
            errs.append(f"D={D} seg_len={seg}: dx is not outdeg 2^-149 ({int((dx == 0).sum())} zeros)")
        # ties
        xt = _dev(xt_np, dev)
        out, cnt = _max_fwd(rig, none, D, seg, xt)
        _, ro, rc = vc.max_fwd_reference(st, xt_np, None)
        if not (np.array_equal(_bits(out.cpu().numpy()), _bits(ro)) and np.array_equal(cnt.cpu().numpy(), rc)):
            errs.append(f"D={D} seg_len={seg} ties: out / cnt are not the restatement's")
        dx = _max_bwd(rig, none, D, seg, xt, out, cnt, cnt.float())[0]
        tied = vc.max_bwd_reference(st, xt_np, None, out.cpu().numpy(), cnt.cpu().numpy(), cnt.cpu().numpy())[4]
        per_src, per_row = np.zeros((vc.N, D)), np.zeros((vc.N, D), np.int64)
        np.add.at(per_src, st.ogt.indices, tied)
        np.add.at(per_row, st.row_of_pos, tied)
        if not np.array_equal(dx.astype(np.float64), per_src):
            errs.append(f"D={D} seg_len={seg} ties: dx is not the number of tied out-edges "
                        f"({int((dx != per_src).sum())} elements differ)")
        if not np.array_equal(per_row, cnt.cpu().numpy()) or dx.sum() != cnt.sum().item():
            errs.append(f"D={D} seg_len={seg} ties: the ties do not number cnt per element")
    xs_np = T.x * np.float32(2.0 ** -130)
    with hw_normals(oracle, dev):
        for name, spec in (("scalar Normal(1, 0.5)", vc.Spec("normal", 1.0, 0.5)),
                           ("per-channel Normal(1, 0.5)", vc.Spec("normal", np.ones_like(T.c0), np.full_like(T.c0, 0.5)))):
            for seg in vc.SEGS:
                _max_check_bwd(errs, "B", rig, spec, D, seg, xs_np, GT.grand[0], f"D={D} max {name} seg_len={seg} x = randn 2^-130")
    ints = np.random.default_rng(5).integers(-3, 4, (vc.COLDOT_N, D)).astype(np.float32)
    got = _coldot(_dev(np.full((vc.COLDOT_N, D), vc.TINY, np.float32), dev), _dev(ints, dev), _dev(-ints, dev))
    want = ints.astype(np.float64).sum(0) * vc.TINY
    if not (np.array_equal(got[0].astype(np.float64), want) and np.array_equal(got[1].astype(np.float64), -want)):
        errs.append(f"D={D} coldot: not the exact multiple of 2^-149")
    got = _segred(_dev(xt_np, dev), _dev(vc.SEGMENT_OFFSETS, dev), False, dev)
    if not np.array_equal(got.astype(np.float64), _segred_ref(xt_np, vc.SEGMENT_OFFSETS, False)):
        errs.append(f"D={D} segment_reduce: not the exact multiple of 2^-149")
    errs.done()


# ---- C. non-finite values stay in place -------------------------------------------------------------------------------
def _contained(errs, key, what, clean, bad, ref, hit, kind="rows", kahan=None, scale=1.0):
    """outside `hit` the poisoned launch keeps the clean launch's bits; inside it is the reference's"""
    if not np.isfinite(clean).all():
        errs.append(f"{what}: the clean launch is not finite")
    leak = (_bits(bad) != _bits(clean)) & ~hit
    if leak.any():
        errs.append(f"{what}: {int(leak.sum())} elements outside the set differ from the clean launch (first at "
                    f"{tuple(np.argwhere(leak)[0])}: {bad[leak][0]!r} vs {clean[leak][0]!r})")
    ref = np.asarray(ref, np.float64)
    sc = vc.out_scale(kind, np.where(hit, 0.0, ref))       # the scale of the clean part
    g_in, r_in = np.where(hit, bad, 0.0), np.where(hit, ref, 0.0)
    _match(errs, key, what, g_in, r_in, scale * sc, "rows", kahan)


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_C_gradients_non_finite_values_stay_in_place(dev, oracle, D):
    """+inf, NaN, -inf in three channels of row U of x (exactly the edges that leave U), of row V0 of g (exactly the edges
    that enter it; stag_agg_bwd_w_mc: of sample 5 only, in the second pass), NaN in one edge's p0 row and +inf in its
    log-scale (exactly that edge; the next edge's row follows it in memory).  With reduce_k the set is those edges' single
    entry.  stag_agg_bwd_pedge's dx: H of the forward suite, Kahan sums pinned to NaN, and equal to stag_agg_fwd_mc_pedge at
    one sample bit for bit on the poisoned input as well."""
    import copy
    from stag_amd import _lib, ops
    rig, GT, T, errs = _rig(oracle, dev), vc.grad_tables(D), vc.tables(D), _Errs()
    st, t, V = rig.st, rig.tables(D), rig.views["t"]
    xp_np = vc.poisoned_row(T.x, vc.U, D)
    g0_np, g5_np = np.array(GT.grand), np.array(GT.grand)
    g0_np[0] = vc.poisoned_row(g0_np[0], vc.V0, D)
    g5_np[vc.GRAD_POISON_SAMPLE] = vc.poisoned_row(g5_np[vc.GRAD_POISON_SAMPLE], vc.V0, D)
    xc, xp, gcl, g0, g5 = (_dev(a, dev) for a in (T.x, xp_np, GT.grand, g0_np, g5_np))
    H = vc.hit_mask(st, D)
    Hp = np.zeros((vc.N, D), bool)
    Hp[vc.HUB, list(vc.POISON[D])] = True
    ran = 0
    with hw_normals(oracle, dev):
        for gc in vc.cases_grad_C(D):
            from_u, into_v0, at_ep = vc.poison_sets(st, D, gc.reduce_k)
            gp_np, gp = (g5_np, g5) if gc.S > 1 else (g0_np, g0)
            runs = [("x[U]", xp_np, xp, GT.grand, gcl, gc, from_u, H), ("g[V0]", T.x, xc, gp_np, gp, gc, into_v0, np.zeros_like(H))]
            for which in (("p0", "p1") if gc.spec is not None else ()):
                gcp = copy.copy(gc)
                gcp.spec = vc.poisoned_param(gc.spec, st, D, which)
                runs.append((which, T.x, xc, GT.grand, gcl, gcp, at_ep, Hp))
            all_refs = [vc.grad_reference(oracle, st, r[5], D, r[1], r[3], GT.ss, GT.ds) for r in runs]
            for seg in vc.SEGS:
                clean = _launch(rig, gc, D, seg, xc, gcl)
                kahan = np.broadcast_to((vc.row_class(st, seg) > 0)[:, None], H.shape)
                for (tag, x_np, x_d, g_np, g_d, case, hit, hit_dx), refs in zip(runs, all_refs):
                    what = f"D={D} {gc.name} seg_len={seg} poisoned {tag}"
                    bad = _launch(rig, case, D, seg, x_d, g_d)
                    for (name, d), kind, c_, b_, r_ in zip(gc.outputs(), gc.kinds(), clean, bad, refs):
                        if d == 0:
                            _contained(errs, f"C {gc.entry} {name}", f"{what} {name}", c_, b_, r_, hit_dx, kahan=kahan)
                            mc = ops._agg_fwd_mc_pedge_raw(V, x_d, _Noise(case.spec.c(dev)), 1, 1, _lib.REDUCE_SUM, t["ss"], t["ds"], seg)
                            errs.same_bits([b_], [mc[0].cpu().numpy()], f"{what}: dx vs stag_agg_fwd_mc_pedge at one sample")
                        else:
                            _contained(errs, f"C {gc.entry} {name}", f"{what} {name}", c_, b_, r_, hit, kind)
                    ran += 1
    assert ran == sum(2 + (2 if gc.spec is not None else 0) for gc in vc.cases_grad_C(D)) * len(vc.SEGS)
    errs.done()


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_C_max_and_reductions_non_finite_values(dev, oracle, D):
    """stag_agg_max_fwd on a poisoned x[U]: a NaN message gives cnt 0 and a NaN out, an infinite one the number of equal
    infinities, outside H nothing moves.  stag_agg_max_bwd with that out and cnt: see the module docstring for the set.
    With g[V0] poisoned and clean out and cnt: only sources with a maximal edge into V0 change.  stag_coldot: a NaN at
    x[r, k] reaches out0[k] and out1[k] only; stag_segment_reduce: that segment's channel only, and an empty segment under
    mean stays +0."""
    rig, GT, T, errs = _rig(oracle, dev), vc.grad_tables(D), vc.tables(D), _Errs()
    st = rig.st
    g = st.ogt
    ch = list(vc.POISON[D])
    xp_np, g_np = vc.poisoned_row(T.x, vc.U, D), GT.grand[0]
    gp_np = vc.poisoned_row(g_np, vc.V0, D)
    H = vc.hit_mask(st, D)
    share = np.unique(g.indices[np.isin(st.row_of_pos, st.fed)])          # U and every source that shares a destination
    assert vc.U in share and len(share) < vc.N
    Hdx = np.zeros((vc.N, D), bool)
    Hdx[np.ix_(share, ch)] = True
    Hdw = np.zeros((vc.N_EDGES, D), bool)
    Hdw[np.ix_(g.eid[np.isin(st.row_of_pos, st.fed)], ch)] = True         # U's out-edges and their row-mates (see above)
    specs = {"none": vc.Spec("none"), "explicit positive": vc.Spec("explicit", T.wpos),
             "per-channel Normal": vc.Spec("normal", T.c0, np.full_like(T.c0, np.float32(0.5)))}
    with hw_normals(oracle, dev):
        for name, spec in specs.items():
            for seg in vc.SEGS:
                what = f"D={D} max {name} seg_len={seg}"
                out, cnt, clean, _ = _max_check_bwd(errs, "C", rig, spec, D, seg, T.x, g_np, what + " clean")
                # poisoned x[U]: forward
                xp = _dev(xp_np, dev)
                obad, cbad = _max_fwd(rig, spec, D, seg, xp)
                _, ro, rc = vc.max_fwd_reference(st, xp_np, _max_spec_weights(oracle, st, spec, D))
                ob, oc = obad.cpu().numpy(), out.cpu().numpy()
                if not (np.array_equal(np.isnan(ob), np.isnan(ro)) and np.array_equal(_bits(ob)[~np.isnan(ro)], _bits(ro)[~np.isnan(ro)])):
                    errs.append(f"{what} poisoned x[U]: out is not the restatement's")
                if not np.array_equal(cbad.cpu().numpy(), rc):
                    errs.append(f"{what} poisoned x[U]: cnt is not the restatement's (NaN: 0, infinities: how many)")
                if not (np.array_equal(_bits(ob)[~H], _bits(oc)[~H]) and np.array_equal(cbad.cpu().numpy()[~H], cnt.cpu().numpy()[~H])):
                    errs.append(f"{what} poisoned x[U]: out / cnt moved outside H")
                # ... and backward with that out and cnt
                refs = vc.max_bwd_reference(st, xp_np, _max_spec_weights(oracle, st, spec, D), ob, cbad.cpu().numpy(), g_np,
                                            *([_max_spec_weights(oracle, st, spec, D, dv) for dv in (1, 2)]
                                              if spec.kind == "normal" else [None, None]))
                bad = _max_bwd(rig, spec, D, seg, xp, obad, cbad, _dev(g_np, dev))
                for nm, c_, b_, r_, hit in zip(("dx", "dw", "dp0_rows", "dp1_rows"), clean, bad, refs, (Hdx, Hdw, Hdx, Hdx)):
                    if b_ is not None:
                        _contained(errs, f"C max_bwd {nm}", f"{what} poisoned x[U] {nm}", c_, b_, r_, hit)
                # poisoned g[V0], clean out and cnt
                refs = vc.max_bwd_reference(st, T.x, _max_spec_weights(oracle, st, spec, D), oc, cnt.cpu().numpy(), gp_np,
                                            *([_max_spec_weights(oracle, st, spec, D, dv) for dv in (1, 2)]
                                              if spec.kind == "normal" else [None, None]))
                tied = refs[4]
                rows = np.arange(g.indptr[vc.V0], g.indptr[vc.V0 + 1])
                Gdx, Gdw = np.zeros((vc.N, D), bool), np.zeros((vc.N_EDGES, D), bool)
                for p in rows:
                    for k in ch:
                        if tied[p, k]:
                            Gdx[g.indices[p], k] = True
                            Gdw[g.eid[p], k] = True
                not_tied_only = [(int(g.indices[p]), k) for p in rows for k in ch if not Gdx[g.indices[p], k]]
                if not (Gdx.any() and not_tied_only):
                    errs.append(f"{what}: the fixture holds no tied / no not-tied edge into V0")
                bad = _max_bwd(rig, spec, D, seg, _dev(T.x, dev), out, cnt, _dev(gp_np, dev))
                for nm, c_, b_, r_, hit in zip(("dx", "dw", "dp0_rows", "dp1_rows"), clean, bad, refs, (Gdx, Gdw, Gdx, Gdx)):
                    if b_ is not None:
                        _contained(errs, f"C max_bwd {nm}", f"{what} poisoned g[V0] {nm}", c_, b_, r_, hit)
                        if nm == "dx" and np.isfinite(b_[Gdx]).any():
                            errs.append(f"{what} poisoned g[V0]: a maximal edge did not receive the poisoned gradient")
    # stag_coldot: a NaN at x[r, k]
    for n in (vc.COLDOT_N, vc.coldot_big_n(D)):
        x, t0, t1 = (vc.away_table(80 + i, (n, D)) for i in range(3))
        r, k = n - 3, ch[1]
        xb = np.array(x)
        xb[r, k] = np.nan
        clean = _coldot(_dev(x, dev), _dev(t0, dev), _dev(t1, dev))
        bad = _coldot(_dev(xb, dev), _dev(t0, dev), _dev(t1, dev))
        for i in (0, 1):
            hit = np.zeros(D, bool)
            hit[k] = True
            if not (np.array_equal(_bits(bad[i])[~hit], _bits(clean[i])[~hit]) and np.isnan(bad[i][k]) and np.isfinite(clean[i]).all()):
                errs.append(f"D={D} coldot n={n} out{i}: a NaN at x[{r}, {k}] is not in column {k} alone")
    offs = vc.SEGMENT_OFFSETS
    seg_hit = int(np.searchsorted(offs, 15, side="right")) - 1
    xb = np.array(T.x)
    xb[15, ch[1]] = np.nan
    for mean in (False, True):
        clean, bad = (_segred(_dev(a, dev), _dev(offs, dev), mean, dev) for a in (T.x, xb))
        hit = np.zeros_like(clean, bool)
        hit[seg_hit, ch[1]] = True
        if not (np.array_equal(_bits(bad)[~hit], _bits(clean)[~hit]) and np.isnan(bad[hit]).all() and np.isfinite(clean).all()):
            errs.append(f"D={D} segment_reduce mean={mean}: a NaN at x[15, {ch[1]}] is not in its segment's channel alone")
        empty = np.diff(offs) == 0
        if _bits(bad)[empty].any():
            errs.append(f"D={D} segment_reduce mean={mean}: an empty segment is not +0")
    errs.done()


# ---- D. parameter edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", vc.WIDTHS)
def test_D_gradients_parameter_edges(dev, oracle, D):
    """Normal with scale 0 (d0 = 1, d1 = z) and with a log-scale of -16 (d1 = z e^-16), Uniform with low == high (1 - u, u),
    Normal(-2, 1) under relu (masks on 1 % to 10 % of the entries), Normal(0, 0) under relu (every gradient exactly 0),
    log-scales of +-16 (outputs that carry the scale divided by e^{+-16}): stag_agg_bwd_w (both; [E, D] and [E, 1] with
    reduce_k), stag_agg_bwd_w_mc at 7 samples, stag_agg_bwd_pedge."""
    rig, GT, T, errs = _rig(oracle, dev), vc.grad_tables(D), vc.tables(D), _Errs()
    st = rig.st
    x, gr = _dev(T.x, dev), _dev(GT.grand, dev)
    shares, ran = [], 0
    with hw_normals(oracle, dev):
        for gc in vc.cases_grad_D(D):
            refs = vc.grad_reference(oracle, st, gc, D, T.x, GT.grand, GT.ss, GT.ds)
            for seg in vc.SEGS:
                what = f"D={D} {gc.name} seg_len={seg}"
                got = _launch(rig, gc, D, seg, x, gr)
                _close_grad(errs, "D", gc, got, refs, what)
                if not all(np.isfinite(o).all() for o in got):
                    errs.append(f"{what}: not finite")
                if gc.zero and any(o.any() for o in got):
                    errs.append(f"{what}: every weight is clamped, a gradient is not 0")
                if "Normal(-2, 1) relu" in gc.name and gc.entry == "bwd_w" and not gc.reduce_k:
                    shares.append(float((got[0] != 0).mean()))
                ran += 1
    assert ran == len(vc.cases_grad_D(D)) * len(vc.SEGS) and len(shares) == len(vc.SEGS)
    assert all(0.01 <= s <= 0.10 for s in shares), f"the share of edges a relu over Normal(-2, 1) keeps: {shares}"
    errs.done()


class _NoiseIn:
    """What ops.materialize_noise reads of a descriptor and of a graph."""

    def __init__(self, spec_c, dn, csr):
        self._spec, self.dn, self.in_norm, self.csr = spec_c, dn, True, csr

    def spec(self):
        return self._spec


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_D_max_parameter_edges_and_in_norm_weights(dev, oracle, D):
    """Bernoulli p = 0: every message is +-0 and all of them tie — cnt == indeg, out keeps the first message's bits, dx == 0;
    a relu that clamps every weight (Normal(0, 0)) behaves the same.  Bernoulli p = 1 equals the NONE launch bit for bit.
    EXPLICIT weights with four exact duplicates of the hub's maximum, across a segment boundary at seg_len 4: cnt == 4, and dw
    gives each an equal share.  stag_noise_materialize with in-norm on the Bernoulli tables whose rows keep no edge: the
    oracle's weights at TOL, the all-zero rows exactly 0, at both seg_lens and without a plan."""
    from stag_amd import ops
    rig, GT, T, errs = _rig(oracle, dev), vc.grad_tables(D), vc.tables(D), _Errs()
    st = rig.st
    g = st.ogt
    g_np = GT.grand[0]
    x = _dev(T.x, dev)
    with hw_normals(oracle, dev):
        for seg in vc.SEGS:
            on, cn, none_bwd, _ = _max_check_bwd(errs, "D", rig, vc.Spec("none"), D, seg, T.x, g_np, f"D={D} max none seg_len={seg}")
            o1, c1, one_bwd, _ = _max_check_bwd(errs, "D", rig, vc.Spec("bernoulli", 1.0), D, seg, T.x, g_np,
                                                f"D={D} max Bernoulli(1) seg_len={seg}")
            errs.same_bits([o1.cpu().numpy(), one_bwd[0]], [on.cpu().numpy(), none_bwd[0]], f"D={D} seg_len={seg}: Bernoulli(1) vs NONE")
            if not torch.equal(c1, cn):
                errs.append(f"D={D} seg_len={seg}: cnt of Bernoulli(1) is not NONE's")
            for name, spec in (("Bernoulli(0)", vc.Spec("bernoulli", 0.0)), ("Normal(0, 0) relu", vc.Spec("normal", 0.0, 0.0, relu=True))):
                what = f"D={D} max {name} seg_len={seg}"
                out, cnt, bwd, _ = _max_check_bwd(errs, "D", rig, spec, D, seg, T.x, g_np, what)
                if not np.array_equal(cnt.cpu().numpy(), st.indeg[:, None] * np.ones((1, D), np.int64)):
                    errs.append(f"{what}: every message is +-0, cnt is not indeg")
                if out.cpu().numpy().any() or any(o is not None and o.any() for o in bwd):
                    errs.append(f"{what}: every weight is 0, an output is not")
            # planted duplicates
            W, xd_np, pos = vc.planted_duplicates(st, D)
            what = f"D={D} max planted duplicates seg_len={seg}"
            out, cnt, bwd, _ = _max_check_bwd(errs, "D", rig, vc.Spec("explicit", W), D, seg, xd_np, g_np, what)
            if not ((cnt.cpu().numpy()[vc.HUB] == 4).all() and (out.cpu().numpy()[vc.HUB] == 64.0).all()):
                errs.append(f"{what}: cnt does not count the duplicates across the segments")
            want = np.zeros((vc.N_EDGES, D), np.float32)
            hub_e = g.eid[g.indptr[vc.HUB]:g.indptr[vc.HUB + 1]]
            want[g.eid[pos]] = np.float32(8.0) * (g_np[vc.HUB] / np.float32(4.0))
            if not np.array_equal(bwd[1][hub_e], want[hub_e]):
                errs.append(f"{what}: dw does not give each duplicate an equal share")
        # stag_noise_materialize with in-norm
        _, pe, pd, _ = vc.bernoulli_tables(oracle, st, D)
        zero_e = np.concatenate([g.eid[g.indptr[r]:g.indptr[r + 1]] for r in (vc.ROW1, vc.ROW3, vc.ROW20, vc.HUB)])
        for name, p in (("[E,1]", pe), ("[E,D]", pd)):
            spec = vc.Spec("bernoulli", p, in_norm=True)
            ref = oracle.noise_materialize(g, spec.o(oracle, D), D)
            assert not ref[zero_e].any() and ref.any() and ref.max() > 1.0, "the oracle's in-norm weights"
            for seg in vc.SEGS + (0,):
                got = ops.materialize_noise(_NoiseIn(None, D, rig.views["t"]), _NoiseIn(spec.c(dev), D, None), seg).cpu().numpy()
                _match(errs, "D noise_materialize in-norm", f"D={D} materialize {name} in-norm seg_len={seg}", got, ref)
                if got[zero_e].any():
                    errs.append(f"D={D} materialize {name} in-norm seg_len={seg}: a row whose every in-edge has p = 0 is not exactly 0")
    errs.done()
