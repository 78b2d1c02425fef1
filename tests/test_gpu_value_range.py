"""The aggregation kernels across the float range and at the edges of the distribution parameters.

Every other GPU test feeds these kernels randn rows, uniform(0.5, 1.5) scales and parameters from the middle of their
ranges, and compares at |got - ref| <= 1e-5 (1 + |ref|): with O(1) data that bar has an absolute floor of 1e-5, so
nothing is checked relative to the data's own scale, and no subnormal, infinite or NaN value ever reaches a kernel.
Here one small graph (tests/value_range_cases.py: a hub of 90 edges, rows of 40, 20, 3, 1 and 0 edges, 150 random ones)
is walked at seg_len 4 (the hub is added group by group, the 40- and 20-edge rows are cut) and 64 (the hub is two
segments, the 40- and 20-edge rows are Kahan units, the rest plain sums), at D = 6 (no vector path, a partial chunk), 8
(vectorised) and 264 (two channel tiles), by every entry point: stag_agg_fwd (the general kernel and the plain-launch
kernel, which exists at 32 and 64 lanes per row: D = 264, and D = 128 without a plan; every plain case is repeated with
STAG_AGG_PLAIN=0 and must give the same bits), _mc, _half, _w1, _mc_edge, _mc_pedge, stag_agg_bwd, _bwd_dp, _bwd_edge.
Normal weights are drawn under util.hw_normals, so they are the device's bit for bit.  tests/test_value_range_host.py
holds every fixture and every bar used here against the oracle and a float64 loop, without a GPU.

What a wrong kernel looks like in each group:
A  power-of-two scaling.  out(c x) must equal c out(x) BIT FOR BIT for c = 2^-100, 2^-60, 2^100 (every operation on the x
   path is a multiply, an add or an fma, and the weights do not depend on x), and out(c x) / c must meet the oracle at
   1e-5: the project's bar at the data's own scale.  An absolute constant anywhere on the x path (an epsilon added to an
   accumulator or to a denominator, a clamp, a threshold) passes every O(1) test and breaks the equality at 2^-100;
   an intermediate formed at the wrong scale (a product of two scaled factors) overflows at 2^100.
B  subnormals.  A table of 2^-149 must sum to indeg 2^-149 exactly, and randn 2^-130 under Normal(1, 0.5) weights and both
   scales must meet the oracle at 1e-5 |ref| + 2 (indeg + 2) 2^-149.  A kernel (or a build flag) that flushes denormal
   inputs or results returns zeros.
C  non-finite values.  +inf, NaN and -inf in three channels of one source row U must make exactly H = {(v, k): v has an
   in-edge from U, k poisoned} non-finite and leave every other element bit-identical to the clean launch: a tail lane,
   a second channel tile, a workspace row of a segment or a cross-lane fold that mixes channels or rows turns a tiny error
   into a NaN in a neighbour, or a finite value inside H.  In plain sums the element is the oracle's (the same signed
   infinity, or NaN); in Kahan sums (units of more than 16 edges, the partials of long rows) a +-inf term becomes NaN,
   which is pinned here ("Value range").
D  parameter edges.  Bernoulli p = 0 and 1 (u < p with u in [0, 1): never | always; p equal to the draw itself: 0, one
   float above: 1 — `<=` in place of `<` fails here), rows whose in-edges all have p = 0 under in-norm (the
   `cur == 0 -> scale 1` branch in a plain sum, a Kahan unit and the group-wise combine), Normal with scale 0 (w == loc),
   Uniform with low == high (w == low), a relu that clamps 98 % or all of the weights (the rows stag_agg_fwd_w1 does not
   read, the 1[w > 0] masks of the three backward kernels), log-scales of +-16 through __expf.  Weights are compared with
   the oracle's bit for bit (stag_noise_materialize), one aggregation per entry point at util.TOL."""
import ctypes as C

import numpy as np
import pytest
import torch

import value_range_cases as vc
from util import assert_close, hw_normals

pytestmark = pytest.mark.gpu

ALL_WIDTHS = tuple(sorted(set(vc.WIDTHS) | set(vc.PLAIN_WIDTHS)))
HALF = [(D, dt) for D in vc.HALF_WIDTHS for dt in ("bfloat16", "float16")]
_RIG = {}


@pytest.fixture(autouse=True)
def _ctypes_front_end(monkeypatch):
    """The raw helpers through ctypes, with the library's stag_noise_spec as it is built here."""
    from stag_amd import _torch_ext
    monkeypatch.setattr(_torch_ext, "available", lambda: False)


class _Noise:
    """What the Monte-Carlo raw helpers read of a descriptor."""

    def __init__(self, spec):
        self._spec = spec

    def spec(self):
        return self._spec


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class _Rig:
    """The fixture graph on the device: the two views, planned at both segment lengths, and the launches."""

    def __init__(self, O, dev):
        from stag_amd.graph import CsrView
        self.O, self.dev, self.st = O, dev, vc.structure(O)
        vc.check_structure(self.st)
        g = self.st.ogt
        indptr, indices, eid, nidx = (_dev(a, dev) for a in (g.indptr, g.indices, g.eid, g.nidx))
        self.views = {"t": CsrView(vc.N, vc.N, indptr, indices, eid=eid, nidx=nidx),
                      "f": CsrView(vc.N, vc.N, indptr, indices, eid=eid)}
        for v in self.views.values():
            for seg in vc.SEGS:
                plan = v.plan(seg)
                plan["xcd_decided"] = True          # plan order, whatever the library's own policy would do after some launches
                nl = plan["n_long"]
                segs = dict(zip(plan["long_rows"][:nl].tolist(), np.diff(plan["long_seg_ptr"][:nl + 1].cpu().numpy()).tolist()))
                vc.check_plan(self.st, seg, plan["n_units"], nl, plan["n_seg"], plan["n_heavy"], segs)
        self._t = {}

    def tables(self, D):
        if D not in self._t:
            T = vc.tables(D)
            self._t[D] = {k: _dev(getattr(T, k), self.dev) for k in ("own", "ss", "ds")}
        return self._t[D]

    def launch(self, case, D, seg, x):
        """The outputs of one launch of the case on the gathered table x (a device tensor), as numpy arrays."""
        from stag_amd import _lib, ops
        V, t = self.views[case.view], self.tables(D)
        sp = case.spec.c(self.dev)
        red = _lib.REDUCE_MEAN if case.reduce == "mean" else _lib.REDUCE_SUM
        ss, ds, own = (t["ss"] if case.ss else None), (t["ds"] if case.ds else None), t["own"]
        e = case.entry
        if e == "fwd":
            outs = [ops._agg_raw(V, x, D, sp, red, ss, ds, seg)[0]]
        elif e == "mc":
            outs = [ops._agg_fwd_mc_raw(V, x, _Noise(sp), vc.MC_S, vc.MC_STRIDE, red, ss, ds, seg)]
        elif e == "half":
            outs = [ops._agg_half_raw(V, x, D, sp, red, ss, ds, seg)]
        elif e == "w1":
            outs = [ops._agg_w1_raw(V, x, D, sp, red, ss, ds, seg)]
        elif e == "mc_edge":
            outs = [ops._agg_fwd_mc_edge_raw(V, x, _Noise(sp), vc.MCE_S, vc.MCE_STRIDE, red, ss, ds, seg)]
        elif e == "mc_pedge":
            outs = [ops._agg_fwd_mc_pedge_raw(V, x, _Noise(sp), vc.MCE_S, vc.MCE_STRIDE, red, ss, ds, seg)]
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
        return [o.cpu().numpy() for o in outs]

    def materialize(self, case, dn, deriv=0):
        """stag_noise_materialize of the case's description without in-norm: [E, dn] by edge id"""
        from stag_amd import _lib
        V = self.views[case.view]
        spec, cs = case.spec.c(self.dev, deriv=deriv, in_norm=False), V.struct()
        w = torch.empty(vc.N_EDGES, dn, device=self.dev)
        with _lib.on_device(self.dev):
            _lib.check(_lib.lib().stag_noise_materialize(C.byref(cs), None, C.byref(spec), dn, _lib.ptr(w), dn, None,
                                                         _lib.stream_of(self.dev)), "stag_noise_materialize")
        return w.cpu().numpy()


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
    def close(self, case, got, refs, what, scale=1.0):
        """every output against its reference at util.TOL, both divided by scale (and the case's own norm) in float64"""
        for i, (kind, g, r, norm) in enumerate(zip(case.kinds(), got, refs, case.norms())):
            g, r = np.asarray(g, np.float64) / (scale * norm), np.asarray(r, np.float64) / (scale * norm)
            sc = vc.out_scale(kind, r)
            try:
                assert_close(g / sc, r / sc, what=f"{what}[{i}]")
            except AssertionError as e:
                self.append(str(e))

    def same_bits(self, a, b, what):
        for i, (x, y) in enumerate(zip(a, b)):
            if not np.array_equal(_bits(x), _bits(y)):
                bad = _bits(x) != _bits(y)
                self.append(f"{what}[{i}]: {int(bad.sum())} of {bad.size} elements differ in their bits "
                            f"(first at {tuple(np.argwhere(bad)[0])}: {x[bad][0]!r} vs {y[bad][0]!r})")

    def done(self):
        assert not self, f"{len(self)} failures:\n" + "\n".join(self[:40])


def _half_table(T, dtype, scale=1.0):
    """(the rows in the half type on the CPU, the same numbers as float32) — scaled in the half type itself, exactly"""
    if dtype == "float16":
        xh = torch.from_numpy(T.x16) * scale
    else:
        xh = torch.from_numpy(T.x).to(torch.bfloat16) * scale
    assert xh.dtype == getattr(torch, dtype)
    return xh, xh.float().numpy()


# ---- A. power-of-two scaling ------------------------------------------------------------------------------------------
def _group_A(rig, case, D, monkeypatch, errs, inputs):
    """inputs: {c: (device table, the Tables the oracle sees)} with c = 1 first"""
    O, st = rig.O, rig.st
    refs = {c: vc.reference(O, st, case, Tc) for c, (_, Tc) in inputs.items()}
    first = {}
    for tag in _variants(case, monkeypatch):
        for seg in case.segs():
            base = None
            for c, (xd, _) in inputs.items():
                what = f"D={D} {case.name}{tag} seg_len={seg} c={c:.1e}"
                got = rig.launch(case, D, seg, xd)
                if base is None:
                    base = got
                else:
                    errs.same_bits(got, [b * np.float32(c) for b in base], f"{what}: out(c x) vs c out(x)")
                errs.close(case, got, refs[c], what, scale=c)
                if case.plain:
                    if tag:
                        errs.same_bits(got, first[seg, c], f"{what}: the general kernel vs the dispatched launch")
                    else:
                        first[seg, c] = got


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_A_power_of_two_scaling(dev, oracle, monkeypatch, D):
    """out(c x) == c out(x) bit for bit and out(c x) / c within 1e-5 of the oracle, c = 2^-100, 2^-60, 2^100: every fp32
    entry point with every noise kind it takes, mean, both scales, in-norm; stag_agg_max_fwd in this group only.  The
    gradients of parameters (dp0 / dp1 [D], dw0 / dw1 [E, 1]) add every edge of the graph and are compared relative to
    their largest entry, as everywhere in the suite."""
    rig, T, errs = _rig(oracle, dev), vc.tables(D), _Errs()
    inputs = {}
    for c in (1.0,) + vc.SCALES:
        Tc = T.with_x(T.x * np.float32(c))
        assert np.isfinite(Tc.x).all() and (np.abs(Tc.x[Tc.x != 0]) >= 2.0 ** -126).all()
        inputs[c] = (_dev(Tc.x, dev), Tc)
    with hw_normals(oracle, dev):
        for case in vc.only(vc.cases_A(D), D):
            _group_A(rig, case, D, monkeypatch, errs, inputs)
    errs.done()


@pytest.mark.parametrize("D,dtype", HALF)
def test_A_power_of_two_scaling_half_rows(dev, oracle, monkeypatch, D, dtype):
    """stag_agg_fwd_half: bf16 rows under the same three scales; fp16 rows of +-uniform[0.25, 4) under 2^-10 and 2^12,
    which keeps every element normal and finite, so the scaling is exact in fp16 too."""
    rig, T, errs = _rig(oracle, dev), vc.tables(D), _Errs()
    inputs = {}
    for c in (1.0,) + (vc.FP16_SCALES if dtype == "float16" else vc.SCALES):
        xh, xf = _half_table(T, dtype, c)
        assert np.array_equal(xf, _half_table(T, dtype)[1] * np.float32(c)), "the scaling is exact in the half type"
        inputs[c] = (xh.to(dev), T.with_x(xf))
    with hw_normals(oracle, dev):
        for case in vc.cases_A_half(D):
            _group_A(rig, case, D, monkeypatch, errs, inputs)
    errs.done()


# ---- B. subnormals are kept -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_B_subnormals(dev, oracle, monkeypatch, D):
    """Exact sums: every element 2^-149, every weight exactly 1 -> indeg(v) 2^-149.  Drawn weights: randn 2^-130 under
    Normal(1, 0.5) and both scales, at 1e-5 |ref| + 2 (indeg(v) + 2) 2^-149 (every term and every scaling is rounded once
    to the subnormal grid, at most 2^-150 each, twice over for margin; sums that small are exact)."""
    rig, T, errs = _rig(oracle, dev), vc.tables(D), _Errs()
    st = rig.st
    tiny = _dev(np.full((vc.N, D), vc.TINY, np.float32), dev)
    want = st.indeg[:, None] * np.float64(vc.TINY) * np.ones((1, D))
    small = T.with_x(T.x * np.float32(2.0 ** -130))
    xs = _dev(small.x, dev)
    with hw_normals(oracle, dev):
        for case in vc.only(vc.cases_B_exact(D), D):
            for tag in _variants(case, monkeypatch):
                for seg in case.segs():
                    (got,) = rig.launch(case, D, seg, tiny)
                    if not np.array_equal(got.astype(np.float64), want):
                        errs.append(f"D={D} {case.name}{tag} seg_len={seg}: not indeg 2^-149 (max |diff| "
                                    f"{np.abs(got - want).max() / vc.TINY:.1f} x 2^-149, {int((got == 0).sum())} zeros)")
        for case in vc.only(vc.cases_B_drawn(D), D):
            (ref,) = vc.reference(oracle, st, case, small)
            bar = vc.subnormal_bar(st, ref, case.kinds()[0])
            for tag in _variants(case, monkeypatch):
                for seg in case.segs():
                    (got,) = rig.launch(case, D, seg, xs)
                    over = np.abs(got.astype(np.float64) - ref) / bar
                    if not over.max() <= 1.0:
                        errs.append(f"D={D} {case.name}{tag} seg_len={seg}: {over.max():.2f} x the subnormal bar "
                                    f"({int((got == 0).sum())} zeros against {int((ref == 0).sum())})")
    errs.done()


@pytest.mark.parametrize("D,dtype", HALF)
def test_B_subnormals_half_rows(dev, oracle, D, dtype):
    """fp16 rows of 2^-24 (bf16: 2^-133), the smallest subnormal of the type, widened in registers: indeg(v) times it,
    exactly.  bf16 rows of randn 2^-130 (subnormal in fp32 once widened) under Normal(1, 0.5) and both scales."""
    rig, errs = _rig(oracle, dev), _Errs()
    st = rig.st
    least = 2.0 ** -24 if dtype == "float16" else 2.0 ** -133
    tiny = torch.full((vc.N, D), least, dtype=getattr(torch, dtype))
    assert float(tiny.float().min()) == least
    want = st.indeg[:, None] * np.float64(least) * np.ones((1, D))
    case = vc.Case("stag_agg_fwd_half none", "half", vc.Spec("none"), ss=False, ds=False)
    for seg in vc.SEGS:
        (got,) = rig.launch(case, D, seg, tiny.to(dev))
        if not np.array_equal(got.astype(np.float64), want):
            errs.append(f"D={D} {dtype} seg_len={seg}: not indeg x the smallest subnormal ({int((got == 0).sum())} zeros)")
    if dtype == "bfloat16":
        xh = (torch.from_numpy(vc.tables(D).x) * 2.0 ** -130).to(torch.bfloat16)
        small = vc.tables(D).with_x(xh.float().numpy())
        assert np.abs(small.x).max() < 2.0 ** -126 and (small.x != 0).mean() > 0.9     # (|randn| < 2^-4 rounds to 0 in bf16)
        case = vc.Case("stag_agg_fwd_half scalar Normal", "half", vc.Spec("normal", 1.0, 0.5))
        with hw_normals(oracle, dev):
            (ref,) = vc.reference(oracle, st, case, small)
            bar = vc.subnormal_bar(st, ref, "rows")
            for seg in vc.SEGS:
                (got,) = rig.launch(case, D, seg, xh.to(dev))
                over = np.abs(got.astype(np.float64) - ref) / bar
                if not over.max() <= 1.0:
                    errs.append(f"D={D} bf16 drawn seg_len={seg}: {over.max():.2f} x the subnormal bar")
    errs.done()


# ---- C. non-finite values stay where the reference puts them --------------------------------------------------------
def _group_C(rig, case, D, monkeypatch, errs, x_clean, x_bad, T_bad):
    st = rig.st
    refs = vc.reference(rig.O, st, case, T_bad)
    H = vc.hit_mask(st, D)
    for tag in _variants(case, monkeypatch):
        for seg in case.segs():
            clean, bad = rig.launch(case, D, seg, x_clean), rig.launch(case, D, seg, x_bad)
            kahan = np.broadcast_to((vc.row_class(st, seg) > 0)[:, None], H.shape)
            for i, (kind, c, b, r) in enumerate(zip(case.kinds(), clean, bad, refs)):
                what = f"D={D} {case.name}{tag} seg_len={seg} [{i}]"
                if kind in ("rows", "mc"):
                    hit, kah = np.broadcast_to(H, b.shape), np.broadcast_to(kahan, b.shape)
                elif kind == "chan":
                    hit = np.zeros(D, bool)
                    hit[list(vc.POISON[D])] = True
                    kah = None
                else:
                    hit = np.zeros((vc.N_EDGES, 1), bool)
                    hit[st.eid_from_u] = True
                    kah = None
                if not np.isfinite(c).all():
                    errs.append(f"{what}: the clean launch is not finite")
                if not np.array_equal(_bits(b)[~hit], _bits(c)[~hit]):
                    leak = (_bits(b) != _bits(c)) & ~hit
                    errs.append(f"{what}: {int(leak.sum())} elements outside H differ from the clean launch "
                                f"(first at {tuple(np.argwhere(leak)[0])}: {b[leak][0]!r} vs {c[leak][0]!r})")
                if np.isfinite(b[hit]).any():
                    errs.append(f"{what}: {int(np.isfinite(b[hit]).sum())} finite elements inside H")
                if kah is None:
                    continue
                r = np.asarray(r)
                plain = hit & ~kah
                same = np.array_equal(np.isnan(b[plain]), np.isnan(r[plain])) and np.array_equal(
                    b[plain][np.isinf(r[plain])], r[plain][np.isinf(r[plain])])
                if not same:
                    errs.append(f"{what}: plain sums inside H are not the oracle's (the same signed infinity, or NaN)")
                # Kahan sums: (n - acc) - y is NaN once a term is infinite, and the next fold takes it into the sum
                if not np.isnan(b[hit & kah]).all():
                    errs.append(f"{what}: Kahan sums inside H are pinned to NaN, got {np.unique(b[hit & kah])}")


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_C_non_finite_values_stay_in_place(dev, oracle, monkeypatch, D):
    """Row U of the gathered table (of g for the backward entry points) holds +inf, NaN, -inf in three channels.  Weights:
    none, explicit and positive, Normal(1, 0.5) without relu (zero weights are stag_agg_fwd_w1's own contract).  Outputs
    [N, D] and [S, N, D]: exactly H non-finite, the rest the clean launch's bits, plain sums equal to the oracle, Kahan sums
    NaN.  dp0 / dp1: non-finite exactly in the poisoned channels; dw0 / dw1: exactly on the edges that leave U."""
    rig, T, errs = _rig(oracle, dev), vc.tables(D), _Errs()
    Tp = T.with_x(vc.poisoned(T.x, D))
    xc, xb = _dev(T.x, dev), _dev(Tp.x, dev)
    with hw_normals(oracle, dev):
        for case in vc.only(vc.cases_C(D), D):
            _group_C(rig, case, D, monkeypatch, errs, xc, xb, Tp)
    errs.done()


@pytest.mark.parametrize("D,dtype", HALF)
def test_C_non_finite_values_half_rows(dev, oracle, monkeypatch, D, dtype):
    rig, T, errs = _rig(oracle, dev), vc.tables(D), _Errs()
    xh, xf = _half_table(T, dtype)
    xp = xh.clone()
    xp[vc.U, list(vc.POISON[D])] = torch.tensor(vc.POISON_VALUES, dtype=xh.dtype)
    Tp = T.with_x(xp.float().numpy())
    assert np.array_equal(np.isfinite(Tp.x), np.isfinite(vc.poisoned(xf, D)))
    with hw_normals(oracle, dev):
        for case in vc.cases_C_half(D):
            _group_C(rig, case, D, monkeypatch, errs, xh.to(dev), xp.to(dev), Tp)
    errs.done()


# ---- D. parameter edges ---------------------------------------------------------------------------------------------
def _group_D(rig, case, D, monkeypatch, errs, xd, T):
    O, st, sp = rig.O, rig.st, case.spec
    dn = sp.dn or D
    g = vc.graph_of(st, case)
    # the weights and their derivatives, against the oracle's
    for deriv in ((0, 1, 2) if sp.kind in ("normal", "uniform") else (0,)):
        what = f"D={D} {case.name}: stag_noise_materialize deriv={deriv}"
        got = rig.materialize(case, dn, deriv)
        ref = O.noise_materialize(g, sp.o(O, D, deriv=deriv, in_norm=False), dn)
        if sp.p1_log and deriv != 1:          # e^{+-16} through __expf against libm: 1e-5 of the scale, not bit for bit
            try:
                assert_close(got.astype(np.float64) / case.norm, ref.astype(np.float64) / case.norm, what=what)
            except AssertionError as e:
                errs.append(str(e))
        else:
            errs.same_bits([got], [ref], what)
    refs = vc.reference(O, st, case, T)
    for tag in _variants(case, monkeypatch):
        for seg in case.segs():
            what = f"D={D} {case.name}{tag} seg_len={seg}"
            got = rig.launch(case, D, seg, xd)
            errs.close(case, got, refs, what)
            if case.zero and any(o.any() for o in got):
                errs.append(f"{what}: every weight is 0, the output is not")
            if not all(np.isfinite(o).all() for o in got):
                errs.append(f"{what}: not finite")


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_D_parameter_edges(dev, oracle, monkeypatch, D):
    """Bernoulli 0 / 1 (scalar, per channel, [E, 1], [E, D], with in-norm over rows that keep no edge), Normal with scale
    0, Uniform with low == high, Normal(-2, 1) and Normal(0, 0) under relu, log-scales of +-16 (every output that carries
    the scale divided by e^{+-16} before the bar; below about -87 the scale is subnormal and v_exp_f32 may flush: not
    tested).  STAG_PRINT_ERR=1 prints how close each comparison runs."""
    rig, T, errs = _rig(oracle, dev), vc.tables(D), _Errs()
    xd = _dev(T.x, dev)
    with hw_normals(oracle, dev):
        for case in vc.only(vc.cases_D(oracle, rig.st, D), D):
            _group_D(rig, case, D, monkeypatch, errs, xd, T)
    errs.done()


@pytest.mark.parametrize("D,dtype", HALF)
def test_D_parameter_edges_half_rows(dev, oracle, monkeypatch, D, dtype):
    rig, T, errs = _rig(oracle, dev), vc.tables(D), _Errs()
    xh, xf = _half_table(T, dtype)
    with hw_normals(oracle, dev):
        for case in vc.cases_D_half(D):
            _group_D(rig, case, D, monkeypatch, errs, xh.to(dev), T.with_x(xf))
    errs.done()
