"""Every row length 0..40 (and 63..65, 68, 69, 127..129, 132) through every kernel's edge loop.

Each kernel walks a unit's edges in blocks of its own size with its own tail: agg_kernel's light units take 16, 8, 4 or 2
edges per trip, its heavy units rounds of SLOTS * NB behind `pb < pend` and `pb + e < pend`, its prefetch loop fetches the
next trip's ids only if `p0 + NB < pend`; plain_walk has its own two-edge loop; agg_half walks 4 or 2 edges, agg_max 4,
agg_bwd_w_mc 2; the segment merges step by 16, 8 and 8 and take another path past 16 segments; the cooperative GAT kernels
walk 1, 2 or 4 rows per round inside batches of at most 256 edges and 32 units.  An edge dropped, taken twice or read with a
stale id in one of these tails shows at particular lengths only, so one graph (tests/row_ladder_cases.py) carries every
length once, at node ids unrelated to the lengths, and is walked without a plan, at seg_len 64 and at seg_len 4, at one width
per lane count and tail form, by every entry point.

Two comparisons, no new number.  EXACT: on small integers, power-of-two scales and Bernoulli(0.5) keeps every partial sum
is exact in fp32, so the device result equals the float64 reference bit for bit, element by element, in any order of
addition.  AT util.TOL: N(0, 1) rows under drawn weights, mean, in-norm and the GAT softmax, against the oracle drawing from
the device's tables (util.hw_normals).  No row is left out; a failure names the entry point, D, seg_len and the LENGTHS of
the rows that differ.  Launches documented as bit-identical are held to that on the ladder too: the plain kernel against
STAG_AGG_PLAIN=0, STAG_COMBINE_GROUPS=0 against the default, a Monte-Carlo sample against the single launch at its offset,
stag_agg_bwd_w_mc at S = 1 against stag_agg_bwd_w, stag_gat_fwd_half against stag_gat_fwd on the widened rows.
tests/test_row_ladder_host.py proves the fixture, the plans, the batches and the references without a GPU.  The wide edge
embedding (stag_edge_embed_bwd over the ladder in both orientations, stag_edge_embed_fwd over the tails of its edge grid) is
follows, with exact values of its own: SiLU and SiLU' are exact at the five pre-activations it uses.  Last,
stag_agg_bwd_pedge over the source-major view (the out-degrees 0..21; cut rows at seg_len 4): exact on integers and
Normal(integer loc, 0) tables, at util.TOL on Normal [E, D] tables with log-scales, and bit for bit against
stag_agg_bwd_w_mc and stag_agg_fwd_mc_pedge at one sample."""
import numpy as np
import pytest
import torch

import row_ladder_cases as rl
from util import TOL, assert_close, assert_gat_grads_vs_oracle, hw_normals

pytestmark = pytest.mark.gpu

HALF = [(D, dt) for D in rl.HALF_WIDTHS for dt in ("bfloat16", "float16")]
_RIG = {}


@pytest.fixture(autouse=True)
def _front_end(monkeypatch):
    """The raw helpers through ctypes, with the library's stag_noise_spec as it is built here; the batched Monte-Carlo
    backward switched on, as tests/test_gpu_mc_bwd.py does."""
    from stag_amd import _torch_ext, ops
    monkeypatch.setattr(_torch_ext, "available", lambda: False)
    monkeypatch.setattr(ops, "MC_BWD_FUSED", True)


class _Noise:
    """What the Monte-Carlo raw helpers read of a descriptor."""

    def __init__(self, spec):
        self._spec = spec

    def spec(self):
        return self._spec


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


class _Rig:
    """The ladder on the device: the views, planned at both segment lengths, and the launches."""

    def __init__(self, O, dev):
        from stag_amd.graph import CsrView
        self.O, self.dev, self.st = O, dev, rl.structure(O)
        st = self.st
        rl.check_structure(st)
        g, s = st.ogt, st.ogs
        indptr, indices, eid, nidx = (_dev(a, dev) for a in (g.indptr, g.indices, g.eid, g.nidx))
        self.views = {"t": CsrView(rl.N, rl.N, indptr, indices, eid=eid, nidx=nidx),
                      "f": CsrView(rl.N, rl.N, indptr, indices, eid=eid),
                      "s": CsrView(rl.N, rl.N, *(_dev(a, dev) for a in (s.indptr, s.indices)), eid=_dev(s.eid, dev),
                                   nidx=_dev(s.nidx, dev))}
        for name in ("t", "f"):
            for seg in rl.PLAN_SEGS:
                plan = self.views[name].plan(seg, need=True)
                plan["xcd_decided"] = True          # plan order, whatever the library's own policy would do after some launches
                nl = plan["n_long"]
                segs = dict(zip(plan["long_rows"][:nl].tolist(), np.diff(_np(plan["long_seg_ptr"][:nl + 1])).tolist()))
                units = _np(plan["units"])[:plan["n_units"]]
                rl.check_plan(st, seg, plan["n_units"], nl, plan["n_seg"], plan["n_heavy"], segs, units)
                assert np.array_equal(_np(plan["block_ptr"]), rl.host_blocks(units)), "the batches of the host test"
        for seg in rl.PLAN_SEGS:
            self.views["s"].plan(seg, need=True)["xcd_decided"] = True
        self._t = {}

    def tables(self, D, exact):
        if (D, exact) not in self._t:
            T = rl.tables(D, exact)
            self._t[D, exact] = {k: _dev(getattr(T, k), self.dev) for k in ("x", "own", "ss", "ds")}
        return self._t[D, exact]

    def launch(self, case, D, seg, x, exact, offset=None, n_samples=None):
        """The outputs of one launch of the case on the gathered table x (a device tensor), as numpy arrays."""
        from stag_amd import _lib, ops
        V, t = self.views[case.view], self.tables(D, exact)
        sp = case.spec.c(self.dev)
        if offset is not None:
            sp.offset = offset
        red = _lib.REDUCE_MEAN if case.reduce == "mean" else _lib.REDUCE_SUM
        ss, ds, own = (t["ss"] if case.ss else None), (t["ds"] if case.ds else None), t["own"]
        e = case.entry
        if e == "fwd":
            outs = [ops._agg_raw(V, x, D, sp, red, ss, ds, seg)[0]]
        elif e == "mc":
            outs = [ops._agg_fwd_mc_raw(V, x, _Noise(sp), rl.MC_S, rl.MC_STRIDE, red, ss, ds, seg)]
        elif e == "half":
            outs = [ops._agg_half_raw(V, x, D, sp, red, ss, ds, seg)]
        elif e == "w1":
            outs = [ops._agg_w1_raw(V, x, D, sp, red, ss, ds, seg)]
        elif e == "mc_edge":
            outs = [ops._agg_fwd_mc_edge_raw(V, x, _Noise(sp), n_samples or rl.MCE_S, rl.MCE_STRIDE, red, ss, ds, seg)]
        elif e == "mc_pedge":
            outs = [ops._agg_fwd_mc_pedge_raw(V, x, _Noise(sp), n_samples or rl.MCE_S, rl.MCE_STRIDE, red, ss, ds, seg)]
        elif e == "bwd":
            outs = [o for o in ops._agg_bwd_raw(V, x, D, sp, ss, ds, seg, case.want_dp) if o is not None]
        elif e == "bwd_dp":
            outs = list(ops._agg_bwd_dp_raw(V, x, own, D, sp, ss, ds, seg))
        elif e == "bwd_edge":
            outs = list(ops._agg_bwd_edge_raw(V, x, own, D, sp, ss, ds, seg))
        else:
            assert e == "max"
            outs = [ops._max_fwd_raw(V, x, D, sp, seg, False)[0]]
        assert len(outs) == len(case.kinds())
        return [_np(o) for o in outs]


def _rig(O, dev):
    if "rig" not in _RIG:
        _RIG["rig"] = _Rig(O, dev)
    return _RIG["rig"]


def _variants(case, monkeypatch):
    """A plain case twice: as dispatched and with the general kernel forced (the library reads the variable at each launch)."""
    for forced in ((False, True) if case.plain else (False,)):
        if forced:
            monkeypatch.setenv("STAG_AGG_PLAIN", "0")
        else:
            monkeypatch.delenv("STAG_AGG_PLAIN", raising=False)
        yield " [STAG_AGG_PLAIN=0]" if forced else ""
    monkeypatch.delenv("STAG_AGG_PLAIN", raising=False)


class _Errs(list):
    """Collects what differs, with the lengths of the rows it differs in, and asserts once.  kind: rows [N, ...] | mc
    [S, N, ...] | edge [E, ...] by edge id (the length of the destination row the edge lies in) | src [N, ...] over the
    sources (out-degrees) | chan [D] (every row adds into it)."""

    def __init__(self, st):
        super().__init__()
        self.st = st

    def where(self, kind, bad):
        st = self.st
        if kind == "chan":
            return f"channels {np.flatnonzero(bad)[:8].tolist()}"
        if kind == "mc":
            bad = bad.any(0)
        hit = bad.reshape(bad.shape[0], -1).any(1)
        if kind == "edge":
            return f"edges of rows of lengths {sorted(set(st.len_of_eid[hit].tolist()))}"
        if kind == "src":
            return f"out-degrees {sorted(set(st.outdeg[hit].tolist()))}"
        return f"lengths {sorted(set(st.indeg[hit].tolist()))}"

    def exact(self, got, ref, kind, what):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bad = ~(got == ref)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            self.append(f"{what}: {self.where(kind, bad)} wrong ({int(bad.sum())} of {bad.size} elements are not the "
                        f"float64 sum; first at {at}: {got[at]!r} vs {ref[at]!r})")

    def close(self, got, ref, kind, what, scaled=False):
        """element by element at util.TOL; scaled: both divided by max(1, max |ref|) first — the gradients of parameters
        ([D], [E, 1], [E, D]), as everywhere in the suite"""
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        sc = max(1.0, float(np.abs(ref).max()) if ref.size else 0.0) if scaled else 1.0
        try:
            assert got.shape == ref.shape, (got.shape, ref.shape)
            assert_close(got / sc, ref / sc, what=what)
        except AssertionError as e:
            bad = ~(np.abs(got - ref) / sc <= TOL * (1.0 + np.abs(ref) / sc))
            self.append(f"{e} — {self.where(kind, bad)} wrong")

    def same_bits(self, a, b, kind, what):
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        bad = a.view(np.int32) != b.view(np.int32)
        if bad.any():
            self.append(f"{what}: {self.where(kind, bad)} differ in their bits ({int(bad.sum())} of {bad.size} elements)")

    def done(self):
        assert not self, f"{len(self)} failures:\n" + "\n".join(self[:40])


def _ungrouped(rig, case, D, x, exact, monkeypatch, got, errs, what):
    """seg_len 4 again with STAG_COMBINE_GROUPS=0 (one team adds a row's partials in segment order): the same bits"""
    monkeypatch.setenv("STAG_COMBINE_GROUPS", "0")
    try:
        again = rig.launch(case, D, 4, x, exact)
    finally:
        monkeypatch.delenv("STAG_COMBINE_GROUPS", raising=False)
    for i, (kind, a, b) in enumerate(zip(case.kinds(), got, again)):
        errs.same_bits(b, a, kind, f"{what} [{i}]: STAG_COMBINE_GROUPS=0 vs the default")


def _run(rig, case, D, x, T, exact, monkeypatch, errs):
    """One case at every segment length (a plain case: twice), each output against the oracle."""
    refs = rl.reference(rig.O, rig.st, case, T)
    first = {}
    for tag in _variants(case, monkeypatch):
        for seg in rl.SEGS:
            what = f"D={D} {case.name}{tag} seg_len={seg}"
            got = rig.launch(case, D, seg, x, exact)
            for i, (kind, g, r) in enumerate(zip(case.kinds(), got, refs)):
                if exact:
                    errs.exact(g, r, kind, f"{what} [{i}]")
                else:
                    errs.close(g, r, kind, f"{what} [{i}]", scaled=kind in ("chan", "edge"))
            if case.plain:
                if tag:
                    for i, (kind, a, b) in enumerate(zip(case.kinds(), got, first[seg])):
                        errs.same_bits(a, b, kind, f"{what} [{i}]: the general kernel vs the dispatched launch")
                else:
                    first[seg] = got
            if seg == 4 and not tag:
                _ungrouped(rig, case, D, x, exact, monkeypatch, got, errs, what)


# ---- exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", rl.WIDTHS)
def test_exact_sums(dev, oracle, monkeypatch, D):
    """Integers: stag_agg_fwd (none, explicit [E, D], Bernoulli(0.5) in the general and the plain kernel), stag_agg_fwd_mc,
    stag_agg_fwd_w1, stag_agg_bwd, stag_agg_max_fwd / _bwd, stag_agg_bwd_w with explicit weights and stag_segment_reduce
    over the ladder's offsets equal the float64 reference bit for bit."""
    from stag_amd import _lib, ops
    rig, T = _rig(oracle, dev), rl.tables(D, True)
    st, errs = rig.st, _Errs(rig.st)
    t = rig.tables(D, True)
    for case in rl.cases_exact(D):
        _run(rig, case, D, t["x"], T, True, monkeypatch, errs)
    # stag_agg_max_fwd with its tie counts, then stag_agg_max_bwd over the source-major view (rows: the out-degrees)
    for kind in ("none", "explicit"):
        W, out, cnt, gout, dx, dw = rl.max_case(oracle, st, D, kind)
        holder = rl.Spec(kind, W)               # (owns the device copy of W for as long as sp is launched)
        sp = holder.c(dev)
        for seg in rl.SEGS:
            what = f"D={D} stag_agg_max {kind} seg_len={seg}"
            o, c = ops._max_fwd_raw(rig.views["f"], t["x"], D, sp, seg, True)
            errs.exact(_np(o), out, "rows", f"{what} out")
            errs.exact(_np(c), cnt, "rows", f"{what} cnt")
            gdx, gdw, _, _ = ops._max_bwd_raw(rig.views["s"], t["x"], _dev(out.astype(np.float32), dev), _dev(cnt, dev),
                                              _dev(gout, dev), D, sp, seg, True, kind == "explicit", False)
            errs.exact(_np(gdx), dx, "src", f"{what} dx")
            if kind == "explicit":
                errs.exact(_np(gdw), dw, "edge", f"{what} dw")
    # stag_agg_bwd_w without a spec: dw[eid] = ss[u] x[u] g[v]
    ref = rl.bwd_w_exact(st, T)
    for seg in rl.SEGS:
        got = ops._bwd_w_raw(rig.views["t"], t["x"], t["own"], D, t["ss"], seg_len=seg)
        errs.exact(_np(got), ref, "edge", f"D={D} stag_agg_bwd_w explicit seg_len={seg}")
    # stag_segment_reduce: the ladder's rows as segments of an [E, D] table
    xe = rl.segment_table(D)
    got = ops._segment_reduce_raw(_dev(xe, dev), rig.views["t"].indptr, _lib.REDUCE_SUM, dev)
    errs.exact(_np(got), rl.segment_sums(st, xe), "rows", f"D={D} stag_segment_reduce")
    errs.done()


@pytest.mark.parametrize("D,dtype", HALF)
def test_exact_sums_half_rows(dev, oracle, monkeypatch, D, dtype):
    """stag_agg_fwd_half: small integers are exact in bf16 and fp16."""
    rig, T = _rig(oracle, dev), rl.tables(D, True)
    errs = _Errs(rig.st)
    xh, xf = rl.half_table(T, dtype)
    for case in rl.cases_exact_half(D):
        _run(rig, case, D, xh.to(dev), T.with_x(xf), True, monkeypatch, errs)
    errs.done()


# ---- at util.TOL -----------------------------------------------------------------------------------------------------------
def _one_sample(rig, case, D, x, monkeypatch, errs):
    """The first and the last sample of a Monte-Carlo batch (its first and its last pass), bit for bit: stag_agg_fwd_mc's are
    stag_agg_fwd at offset + s * stride; stag_agg_fwd_mc_edge's and _pedge's (which add in blocks of four positions, not
    in stag_agg_fwd's order) do not depend on the samples that share their pass: the call with one sample at that offset."""
    S, stride = (rl.MC_S, rl.MC_STRIDE) if case.entry == "mc" else (rl.MCE_S, rl.MCE_STRIDE)
    single = rl.Case(case.name, "fwd", case.spec, reduce=case.reduce, ss=case.ss, ds=case.ds, view=case.view)
    for seg in rl.SEGS:
        (mc,) = rig.launch(case, D, seg, x, False)
        for s in (0, S - 1):
            off = rl.OFFSET + s * stride
            if case.entry == "mc":
                (one,) = rig.launch(single, D, seg, x, False, offset=off)
            else:
                one = rig.launch(case, D, seg, x, False, offset=off, n_samples=1)[0][0]
            errs.same_bits(mc[s], one, "rows", f"D={D} {case.name} seg_len={seg}: sample {s} vs the single launch at its offset")


@pytest.mark.parametrize("D", rl.WIDTHS)
def test_drawn_weights_means_and_in_norm(dev, oracle, monkeypatch, D):
    """N(0, 1) rows at util.TOL: stag_agg_fwd (scalar and per-channel Normal with relu, Uniform and Bernoulli with in-norm,
    [E, 1] Normal with a log-scale, [E, D] Normal, mean, two plain launches), stag_agg_fwd_mc (S = 5; in-norm: passes of 2,
    2, 1), stag_agg_fwd_w1, stag_agg_fwd_mc_edge / _pedge (S = 7), stag_agg_bwd with both derivative aggregates,
    stag_agg_bwd_dp, stag_agg_bwd_edge with its stores by edge id, stag_agg_max_fwd, stag_agg_bwd_w and stag_agg_bwd_w_mc
    (S = 3) on an [E, D] Normal spec."""
    from stag_amd import ops
    rig, T = _rig(oracle, dev), rl.tables(D, False)
    errs, t = _Errs(rig.st), rig.tables(D, False)
    V = rig.views["t"]
    with hw_normals(oracle, dev):
        for case in rl.cases_tol(D):
            _run(rig, case, D, t["x"], T, False, monkeypatch, errs)
            if case.entry in ("mc", "mc_edge", "mc_pedge") and not case.spec.in_norm:
                _one_sample(rig, case, D, t["x"], monkeypatch, errs)
        # the per-edge parameter gradients: one sample (stag_agg_bwd_w, both derivatives from one pass) and S = 3
        holder = rl.bwd_w_spec(D)               # (owns the device copies of the two tables)
        sp = holder.c(dev)
        gmc = _dev(T.gmc, dev)
        ref1 = rl.bwd_w_reference(oracle, rig.st, T, 1, rl.MCB_STRIDE, None)
        ref3 = rl.bwd_w_reference(oracle, rig.st, T, rl.MCB_S, rl.MCB_STRIDE, T.ds)
        for seg in rl.SEGS:
            what = f"D={D} [E,D] Normal seg_len={seg}"
            one = ops._bwd_w_raw(V, t["x"], gmc[0], D, t["ss"], spec=sp, both=True, seg_len=seg)
            mc1 = ops._bwd_w_mc_raw(V, t["x"], gmc[:1], D, t["ss"], None, sp, 1, rl.MCB_STRIDE, seg_len=seg)
            mc3 = ops._bwd_w_mc_raw(V, t["x"], gmc, D, t["ss"], t["ds"], sp, rl.MCB_S, rl.MCB_STRIDE, seg_len=seg)
            for i in range(2):
                errs.close(_np(one[i]), ref1[i], "edge", f"{what} stag_agg_bwd_w d p{i}", scaled=True)
                errs.close(_np(mc3[i]), ref3[i], "edge", f"{what} stag_agg_bwd_w_mc S=3 d p{i}", scaled=True)
                errs.same_bits(_np(mc1[i]), _np(one[i]), "edge", f"{what} d p{i}: stag_agg_bwd_w_mc at S=1 vs stag_agg_bwd_w")
    errs.done()


@pytest.mark.parametrize("D,dtype", HALF)
def test_drawn_weights_half_rows(dev, oracle, monkeypatch, D, dtype):
    """stag_agg_fwd_half under Normal(1, 0.5) noise, sum and mean, against the oracle on the widened rows."""
    rig, T = _rig(oracle, dev), rl.tables(D, False)
    errs = _Errs(rig.st)
    xh, xf = rl.half_table(T, dtype)
    with hw_normals(oracle, dev):
        for case in rl.cases_tol_half(D):
            _run(rig, case, D, xh.to(dev), T.with_x(xf), False, monkeypatch, errs)
    errs.done()


# ---- GAT -------------------------------------------------------------------------------------------------------------------
def _gat_graph(dev, O):
    """The ladder as a stag_amd.Graph: its forward CSR is the view `ogf`, its unit batches are the host test's."""
    if "gat" not in _RIG:
        import stag_amd
        st = rl.structure(O)
        g = stag_amd.Graph(torch.from_numpy(st.coo_src), torch.from_numpy(st.coo_dst), rl.N, device=dev)
        c, ct = g.csr, g.csr_t
        for a, b in ((c.indptr, st.ogf.indptr), (c.indices, st.ogf.indices), (c.eid, st.ogf.eid),
                     (ct.indptr, st.ogs.indptr), (ct.indices, st.ogs.indices), (ct.eid, st.ogs.eid), (ct.nidx, st.ogs.nidx)):
            assert np.array_equal(_np(a), b)
        facts = {}
        for seg in rl.PLAN_SEGS:
            plan = c.plan(seg, need=True)
            units = _np(plan["units"])[:plan["n_units"]]
            host = rl.host_plan(st.ogf.indptr, seg)["units"]
            assert np.array_equal(units, host) and np.array_equal(_np(plan["block_ptr"]), rl.host_blocks(host))
            facts[seg] = rl.batch_facts(units, _np(plan["block_ptr"]))
        rl.check_batches(facts)
        _RIG["gat"] = g
    return _RIG["gat"]


def _gat_weight(dev, O, g, name, H, p, offset=None):
    """(the weight argument of ops.gat_aggregate, the oracle's spec)"""
    import stag_amd
    from stag_amd import _lib
    spec = rl.gat_spec(O, name, H, p["w"], offset)
    if name == "none":
        return None, spec
    if name == "explicit":
        return _dev(p["w"], dev), spec
    kw = dict(rl.GAT_NOISE)
    if offset is not None:
        kw["offset"] = offset
    return stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.5, **kw), spec


def _gat_stats(st, p, W, stats, errs, what):
    """stats[:, :H] equals the row maximum of the fp32 logits (formed in numpy float32 as the kernels form them, the
    library is built with -ffp-contract=off), stats[:, H:] is sum exp(logit - m) within util.TOL, relative; rows with
    in-edges."""
    g, H = st.ogf, p["el"].shape[1]
    u, v = g.indices, st.row_of_pos
    s = p["el"][u] + p["er"][v]
    lr = np.where(s > 0, s, np.float32(rl.GAT_SLOPE) * s)
    logit = lr if W is None else W[g.eid].astype(np.float32) * lr
    assert logit.dtype == np.float32
    m = np.full((rl.N, H), -np.inf, np.float32)
    np.maximum.at(m, v, logit)
    l = np.zeros(m.shape, np.float64)
    np.add.at(l, v, np.exp(logit.astype(np.float64) - m[v].astype(np.float64)))
    has = st.indeg > 0
    got = _np(stats)
    bad = np.zeros(rl.N, bool)
    bad[has] = (got[has, :H] != m[has]).any(1)
    if bad.any():
        errs.append(f"{what} stats m: lengths {sorted(set(st.indeg[bad].tolist()))} are not the row maximum of the logits")
    got_l, ref_l = np.where(has[:, None], got[:, H:], 1.0), np.where(has[:, None], l, 1.0)
    errs.close(got_l / ref_l - 1.0, np.zeros_like(ref_l), "rows", f"{what} stats l (relative)")


@pytest.mark.parametrize("H,F", rl.GAT_SHAPES)
def test_gat_forward(dev, oracle, H, F):
    """stag_gat_fwd out and stats, stag_gat_attn, stag_gat_fwd_half on bf16 and fp16 rows and stag_gat_fwd_mc (S = 5) at
    seg_len 64 and 4, without weights, with explicit [E, H] weights and under Normal(1, 0.5) noise: (1, 4) and (3, 4) one
    lane per head (four rows in flight; an odd head count), (4, 16) 64 lanes at one chunk per lane, (8, 64) two chunks,
    (4, 256) four chunks — the cooperative kernels, asserted from ops.gat_cooperative_shape — and (4, 5), outside them:
    gat_fwd_kernel, one unit per team."""
    from stag_amd import ops
    g, st, p = _gat_graph(dev, oracle), rl.structure(oracle), rl.gat_inputs(H, F)
    errs = _Errs(st)
    coop = (H, F) in rl.GAT_COOPERATIVE
    eld, erd, ftd = (_dev(p[k], dev) for k in ("el", "er", "ft"))
    halves = {dt: ftd.to(getattr(torch, dt)) for dt in ("bfloat16", "float16")}
    for seg in rl.PLAN_SEGS:
        assert ops.gat_cooperative_shape(H, F, seg) == coop
        if coop:
            assert ops.gat_lanes_per_head(F) == rl.GAT_LANES[H, F]
        for name in rl.GAT_WEIGHTINGS:
            what = f"GAT ({H}, {F}) {name} seg_len={seg}"
            weight, spec = _gat_weight(dev, oracle, g, name, H, p)
            with hw_normals(oracle, dev):
                ref, ref_attn = oracle.gat_fwd(st.ogf, p["el"], p["er"], p["ft"], rl.GAT_SLOPE, spec, want_attn=True)
            with torch.no_grad():
                out, attn = ops.gat_aggregate(g, eld, erd, ftd, rl.GAT_SLOPE, weight, want_attn=True, seg_len=seg)
            errs.close(_np(out), ref, "rows", f"{what} stag_gat_fwd out")
            errs.close(_np(attn), ref_attn, "edge", f"{what} stag_gat_attn")
            # the raw launch: the same out, and the softmax statistics
            out2 = torch.full((rl.N, H, F), float("nan"), device=dev)
            stats = torch.full((rl.N, 2 * H), float("nan"), device=dev)
            raw = (weight.spec() if name == "normal" else ops._targs_or_c(ops._explicit_spec(weight)) if name == "explicit"
                   else ops._targs_or_c(ops._none_spec()))
            ops._gat_fwd_into(g.csr, g.csr.plan(seg, need=True), eld, erd, ftd, H, F, rl.GAT_SLOPE, raw, None, None, out2, stats, dev)
            errs.same_bits(_np(out2), _np(out), "rows", f"{what}: the raw launch vs ops.gat_aggregate")
            W = None if name == "none" else p["w"] if name == "explicit" else _np(weight.materialize())
            _gat_stats(st, p, W, stats, errs, what)
            if not coop:
                continue
            # half rows: the oracle on the widened rows, and the fp32 entry's bits on them
            for dt, fth in halves.items():
                assert ops.gat_half_rows_why_not(fth, seg, g, weight if name == "normal" else None) is None
                with hw_normals(oracle, dev):
                    refh = oracle.gat_fwd(st.ogf, p["el"], p["er"], _np(fth.float()), rl.GAT_SLOPE, spec)
                with torch.no_grad():
                    outh = ops.gat_aggregate(g, eld, erd, fth, rl.GAT_SLOPE, weight, seg_len=seg)
                    wide = ops.gat_aggregate(g, eld, erd, fth.float(), rl.GAT_SLOPE, weight, seg_len=seg)
                errs.close(_np(outh), refh, "rows", f"{what} stag_gat_fwd_half {dt}")
                errs.same_bits(_np(outh), _np(wide), "rows", f"{what} stag_gat_fwd_half {dt} vs stag_gat_fwd on the widened rows")
        # Monte-Carlo samples of the Normal noise: each against the oracle and the single launch at its offset
        noise, _ = _gat_weight(dev, oracle, g, "normal", H, p)
        with torch.no_grad():
            mc = ops.gat_aggregate_mc(g, eld, erd, ftd, rl.GAT_SLOPE, noise, rl.GAT_MC_S, rl.GAT_MC_STRIDE, seg_len=seg)
        assert mc.shape == (rl.GAT_MC_S, rl.N, H, F)
        for s in range(rl.GAT_MC_S):
            what = f"GAT ({H}, {F}) seg_len={seg} stag_gat_fwd_mc sample {s}"
            nz, spec = _gat_weight(dev, oracle, g, "normal", H, p, offset=rl.GAT_NOISE["offset"] + s * rl.GAT_MC_STRIDE)
            with hw_normals(oracle, dev):
                ref = oracle.gat_fwd(st.ogf, p["el"], p["er"], p["ft"], rl.GAT_SLOPE, spec)
            errs.close(_np(mc[s]), ref, "rows", what)
            with torch.no_grad():
                one = ops.gat_aggregate(g, eld, erd, ftd, rl.GAT_SLOPE, nz, seg_len=seg)
            errs.same_bits(_np(mc[s]), _np(one), "rows", f"{what} vs the single launch at its offset")
    errs.done()


GAT_BWD_FORMS = {"one_gather": (True, True), "two_pass": (False, True), "edge": (True, False)}


def _gat_grad_lengths(errs, oracle, st, dev, p, spec, got, got_dw):
    """which rows of the gradients miss util.assert_gat_grads_vs_oracle's bar: d el and d ft over the sources (out-degrees),
    d er over the destinations, d w by edge id"""
    with hw_normals(oracle, dev):
        refs = oracle.gat_bwd(st.ogf, p["el"], p["er"], p["ft"], p["G"], rl.GAT_SLOPE, spec, want_dw=got_dw is not None)
    out = []
    for g_, r_, kind in zip(list(got) + [got_dw], refs, ("src", "rows", "src", "edge")):
        if g_ is None:
            continue
        g_, r_ = np.asarray(_np(g_), np.float64), np.asarray(r_, np.float64)
        bad = np.abs(g_ - r_) > TOL * (np.abs(r_).max() + np.abs(r_))
        if bad.any():
            out.append(errs.where(kind, bad))
    return "; ".join(out) or "inside the bar relative to each gradient's own largest entry"


@pytest.mark.parametrize("H,F", rl.GAT_SHAPES)
def test_gat_backward(dev, oracle, monkeypatch, H, F):
    """d el, d er, d ft (and d w of the explicit weights) with util.assert_gat_grads_vs_oracle through the one-gather
    backward (stag_gat_bwd), the two-pass form (stag_gat_bwd_two_pass) and with the fused backward off (stag_gat_bwd_edge
    plus aggregations where the shape has that form, else the composed path's autograd), at seg_len 64 and 4: the source
    pass walks the transposed CSR, whose rows run over the out-degrees 0..21."""
    from stag_amd import ops
    g, st, p = _gat_graph(dev, oracle), rl.structure(oracle), rl.gat_inputs(H, F)
    errs = _Errs(st)
    Gd = _dev(p["G"], dev)
    for seg in rl.PLAN_SEGS:
        for name in rl.GAT_WEIGHTINGS:
            for form, (one_gather, fused) in GAT_BWD_FORMS.items():
                monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", one_gather)
                monkeypatch.setattr(ops, "_GAT_BWD_FUSED", fused)
                what = f"GAT ({H}, {F}) {name} seg_len={seg} backward {form}"
                t = [_dev(p[k], dev).requires_grad_(True) for k in ("el", "er", "ft")]
                weight, spec = _gat_weight(dev, oracle, g, name, H, p)
                if name == "explicit":
                    weight.requires_grad_(True)
                ops.gat_aggregate(g, *t, rl.GAT_SLOPE, weight, seg_len=seg).backward(Gd)
                got, got_dw = [a.grad for a in t], (weight.grad if name == "explicit" else None)
                try:
                    assert_gat_grads_vs_oracle(oracle, st.ogf, p["el"], p["er"], p["ft"], p["G"], spec, got, got_dw=got_dw,
                                               what=what, dev=dev)
                except AssertionError as e:
                    errs.append(f"{e} — {_gat_grad_lengths(errs, oracle, st, dev, p, spec, got, got_dw)}")
    errs.done()


@pytest.mark.parametrize("H,F", rl.GAT_COOPERATIVE)
def test_gat_backward_parameter_gradients(dev, oracle, monkeypatch, H, F):
    """stag_gat_bwd_dp: live per-head Normal parameters stay in the kernels (no [E, H] tensor); the finished gradients
    against the oracle's backward on the materialised draw, dp_i[h] = sum_e dL/dw dw/dp_i, as
    tests/test_gpu_gat_softmax_range.py compares them."""
    import stag_amd
    from stag_amd import _lib, ops
    g, st, p = _gat_graph(dev, oracle), rl.structure(oracle), rl.gat_inputs(H, F)
    p0h, p1h = np.linspace(0.8, 1.2, H).astype(np.float32), np.linspace(0.3, 0.6, H).astype(np.float32)
    kw = dict(seed=rl.GAT_NOISE["seed"], offset=rl.GAT_NOISE["offset"], Dn=H, n_edges=rl.N_EDGES)
    with hw_normals(oracle, dev):
        std = oracle.noise_materialize(st.ogf, oracle.make_spec("normal", 0.0, 1.0, **kw), H).astype(np.float64)
        wmat = oracle.noise_materialize(st.ogf, oracle.make_spec("normal", p0h, p1h, **kw), H)
    spec = oracle.make_spec("explicit", wmat)
    d_el, d_er, d_ft, dw = oracle.gat_bwd(st.ogf, p["el"], p["er"], p["ft"], p["G"], rl.GAT_SLOPE, spec, want_dw=True)
    dw = dw.astype(np.float64)
    for seg in rl.PLAN_SEGS:
        p0, p1 = _dev(p0h, dev).requires_grad_(True), _dev(p1h, dev).requires_grad_(True)
        noise = stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, p0, p1, differentiable=True, **rl.GAT_NOISE)
        t = [_dev(p[k], dev).requires_grad_(True) for k in ("el", "er", "ft")]
        with monkeypatch.context() as m:
            m.setattr(stag_amd.EdgeNoise, "materialize",
                      lambda self: (_ for _ in ()).throw(AssertionError("an [E, H] tensor was materialised")))
            ops.gat_aggregate(g, *t, rl.GAT_SLOPE, noise, seg_len=seg).backward(_dev(p["G"], dev))
        for got, ref, nm in ((p0.grad, dw.sum(0), "d p0"), (p1.grad, (dw * std).sum(0), "d p1")):
            sc = max(1.0, float(np.abs(ref).max()), float(np.abs(dw).max()))
            assert_close(_np(got) / sc, ref / sc, what=f"GAT ({H}, {F}) seg_len={seg} stag_gat_bwd_dp {nm}")
        assert_gat_grads_vs_oracle(oracle, st.ogf, p["el"], p["er"], p["ft"], p["G"], spec, [a.grad for a in t],
                                   what=f"GAT ({H}, {F}) seg_len={seg} stag_gat_bwd_dp", dev=dev)


# ---- the wide edge embedding ---------------------------------------------------------------------------------------------------
def _embed_bwd(rig, orient, own, other, g, seg):
    from stag_amd import ops
    V = rig.views[rl.EMBED_ORIENT[orient][0]]
    return _np(ops._edge_embed_bwd_raw(V, *(_dev(a, rig.dev) for a in (own, other, g)), seg_len=seg))


@pytest.mark.parametrize("hidden", rl.EMBED_WIDTHS)
def test_edge_embed_backward(dev, oracle, hidden):
    """stag_edge_embed_bwd in both orientations (d pd over the destination rows: every length of the ladder; d ps over the
    source rows: the out-degrees) without a plan, at seg_len 64 and at seg_len 4: a unit's edges go in rounds of LPE (4, 16,
    64) and blocks of 4 positions.  EXACT: own in {0, 64}, other in {0, 64, -256}, so SiLU' is 0.5, 1 or 0 exactly and every
    partial sum of g SiLU' (g: nonzero integers in [-8, 8]) is a multiple of 1/2 below 2^22: d_own equals the float64
    reference as fp32 values.  AT util.TOL: N(0, 1) tables under util.assert_close_cond — a row adds up to 132 terms
    g SiLU' of both signs, each rounded to fp32 once by the kernel and formed in double by the reference; the plain
    distance stays below the plain bar on this graph (tests/test_row_ladder_host.py prints it for the float32
    restatement: at most 3.7e-06), and the conditioned bar is kept because it is the one the entry point's own tests
    hold these sums to."""
    from util import assert_close_cond
    rig = _rig(oracle, dev)
    errs = _Errs(rig.st)
    for orient, (_, kind) in rl.EMBED_ORIENT.items():
        view = rl.embed_view(rig.st, orient)
        for exact in (True, False):
            own, other, g = rl.embed_tables(hidden, exact, orient)
            ref, ab = rl.embed_bwd_reference(view, own, other, g, exact=exact)
            for seg in rl.SEGS:
                what = f"stag_edge_embed_bwd {orient} hidden={hidden} seg_len={seg} {'exact' if exact else 'N(0, 1)'}"
                got = _embed_bwd(rig, orient, own, other, g, seg)
                if exact:
                    errs.exact(got, ref, kind, what)
                    continue
                try:
                    assert_close_cond(got, ref, ab, what=what)
                except AssertionError as e:
                    bad = ~(np.abs(got - ref) <= TOL * (1.0 + np.abs(ref)) + 2.0 ** -24 * ab)
                    errs.append(f"{e} — {errs.where(kind, bad)} wrong")
    errs.done()


@pytest.mark.parametrize("hidden", list(rl.EMBED_FWD_WIDTHS))
def test_edge_embed_forward_tails(dev, hidden):
    """stag_edge_embed_fwd at E = 1, T - 1, T, T + 1, 4 T - 1, 4 T, 4 T + 1 (T = 256 / LPE teams per block, four edges per
    team: one block exactly full, one edge short, one edge over) at 4 and at 64 lanes per edge, vectorised and not: h equals
    the exact SiLU (0, 64, 128, -0) as fp32 values, and nothing behind row E - 1 is written."""
    from stag_amd import ops
    guard = 8
    bad = []
    for E in rl.embed_fwd_sizes(rl.EMBED_FWD_WIDTHS[hidden]):
        src, dst, ps, pd = rl.embed_fwd_case(hidden, E)
        ref = np.vectorize(lambda v: rl.EMBED_CLASS[float(v)][0])(ps[src] + pd[dst]).astype(np.float64)
        buf = torch.full((E + guard, hidden), float("nan"), device=dev)
        ops._edge_embed_fwd_raw(_dev(src, dev), _dev(dst, dev), _dev(ps, dev), _dev(pd, dev), out=buf[:E])
        got = _np(buf).astype(np.float64)
        wrong = ~(got[:E] == ref).all(1)
        if wrong.any():
            bad.append(f"hidden={hidden} E={E}: edges {np.flatnonzero(wrong)[:8].tolist()} are not SiLU of their pre-activation "
                       f"(first: {got[:E][wrong][0][:4].tolist()} vs {ref[wrong][0][:4].tolist()})")
        if not np.isnan(got[E:]).all():
            bad.append(f"hidden={hidden} E={E}: rows behind the last edge were written")
    assert not bad, "\n".join(bad)


# ---- stag_agg_bwd_pedge over the source-major view: the out-degree ladder 0..20 and, at seg_len 4, its cut rows -----------
@pytest.mark.parametrize("D", rl.PEDGE_WIDTHS)
def test_bwd_pedge_over_the_out_degree_ladder(dev, oracle, D):
    """dx (a sum over a source's out-edges, in plan order) and the two [E, D] gradient tables (products stored where the edge
    is walked) for every out-degree, without a plan, at seg_len 64 (whole rows, Kahan past 16) and 4 (rows of more than 4
    edges cut).  EXACT: integers and Normal(integer loc, 0) — dx equals the integer sums and dp0 the integer products bit
    for bit.  AT util.TOL: Normal [E, D] tables with log-scales against the float64 restatement, and bit for bit against
    the entries whose arithmetic it restates: stag_agg_bwd_w_mc at one sample on the forward view (dp0, dp1) and
    stag_agg_fwd_mc_pedge at one sample on this view (dx).  Leaving dx or dp1 out changes no other output."""
    from stag_amd import _lib, ops
    rig = _rig(oracle, dev)
    st, errs = rig.st, _Errs(rig.st)
    V, F = rig.views["s"], rig.views["f"]
    ran = 0
    with hw_normals(oracle, dev):
        for exact, spec in zip((True, False), rl.pedge_specs(D)):
            T, t = rl.tables(D, exact), rig.tables(D, exact)
            rdx, rd0, rd1, _ = rl.pedge_reference(oracle, st, T, spec)
            sp = spec.c(dev)
            for seg in rl.SEGS:
                what = f"stag_agg_bwd_pedge D={D} {'exact' if exact else 'Normal p1_log'} seg_len={seg}"
                dx, d0, d1 = (_np(o) for o in ops._agg_bwd_pedge_raw(V, t["x"], t["own"], D, sp, t["ss"], t["ds"], seg))
                if exact:
                    errs.exact(dx, rdx, "src", f"{what} dx")
                    errs.exact(d0, rd0, "edge", f"{what} dp0")
                else:
                    errs.close(dx, rdx, "src", f"{what} dx")
                    errs.close(d0, rd0, "edge", f"{what} dp0", scaled=True)
                    errs.close(d1, rd1, "edge", f"{what} dp1", scaled=True)
                w0, w1 = ops._bwd_w_mc_raw(F, t["own"], t["x"][None].contiguous(), D, t["ds"], t["ss"], sp, 1, 1, seg_len=seg)
                errs.same_bits(d0, _np(w0), "edge", f"{what} dp0 vs stag_agg_bwd_w_mc at one sample")
                errs.same_bits(d1, _np(w1), "edge", f"{what} dp1 vs stag_agg_bwd_w_mc at one sample")
                mc = ops._agg_fwd_mc_pedge_raw(V, t["x"], _Noise(sp), 1, 1, _lib.REDUCE_SUM, t["ss"], t["ds"], seg)
                errs.same_bits(dx, _np(mc[0]), "src", f"{what} dx vs stag_agg_fwd_mc_pedge at one sample")
                n0, e0, e1 = ops._agg_bwd_pedge_raw(V, t["x"], t["own"], D, sp, t["ss"], t["ds"], seg, want_dx=False)
                assert n0 is None
                errs.same_bits(_np(e0), d0, "edge", f"{what} dp0 without dx")
                errs.same_bits(_np(e1), d1, "edge", f"{what} dp1 without dx")
                x2, e0, n1 = ops._agg_bwd_pedge_raw(V, t["x"], t["own"], D, sp, t["ss"], t["ds"], seg, want_p1=False)
                assert n1 is None
                errs.same_bits(_np(x2), dx, "src", f"{what} dx without dp1")
                errs.same_bits(_np(e0), d0, "edge", f"{what} dp0 without dp1")
                ran += 1
    assert ran == 2 * len(rl.SEGS)
    errs.done()
