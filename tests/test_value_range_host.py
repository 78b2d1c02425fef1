"""The fixtures of tests/test_gpu_value_range.py without a GPU: every case of groups A-D (tests/value_range_cases.py) goes
through the oracle and through an independent float64 numpy loop over the edges, and the conditions the device test
relies on are asserted for the reference alone:
  - the graph has the rows it was built for, source row U feeds the rows it must, and the host planner cuts it at
    seg_len 4 and 64 the way the device test says;
  - A: the oracle is bit-exactly equivariant under the three power-of-two scales and within the 1e-5 bar of the loop;
  - B: the 2^-149 table sums exactly, and on x = randn 2^-130 the oracle stays inside 1e-5 |ref| + 2 (indeg + 2) 2^-149;
  - C: the oracle's non-finite elements are exactly the hit set H, everything else is bit-identical to the clean run;
  - D: Bernoulli 0 / 1 give all zeros / all ones, p equal to the draw gives 0 and the next float above it 1, scale 0 gives
    loc, low = high gives low, the derivatives are 1 | z and 1 - u | u, Normal(-2, 1) under relu keeps between 1 % and 10 %
    of the weights, Normal(0, 0) under relu keeps none, log-scales of +-16 stay finite.
If a fixture drifts, this module fails here, not on the device."""
import numpy as np
import pytest

import value_range_cases as vc
from util import assert_close

ALL_WIDTHS = tuple(sorted(set(vc.WIDTHS) | set(vc.PLAIN_WIDTHS)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _close(case, kinds, refs, nps, scale, what):
    scales = scale if isinstance(scale, list) else [scale] * len(kinds)
    for i, (kind, r, n, s) in enumerate(zip(kinds, refs, nps, scales)):
        r, n = np.asarray(r, np.float64) / s, np.asarray(n, np.float64) / s
        sc = vc.out_scale(kind, r)
        assert_close(r / sc, n / sc, what=f"{what}[{i}] oracle vs the float64 loop")


def test_fixture_graph_and_plans(oracle):
    st = vc.structure(oracle)
    vc.check_structure(st)
    for seg in vc.SEGS:
        p = vc.host_plan(st.ogt.indptr, seg)
        vc.check_plan(st, seg, p["n_units"], p["n_long"], p["n_seg"], p["n_heavy"], p["segs"])
        cls = vc.row_class(st, seg)
        assert cls[vc.HUB] == 2 and cls[vc.ROW3] == cls[vc.ROW1] == 0
        assert cls[vc.ROW40] == cls[vc.ROW20] == (2 if seg == 4 else 1)
        # every class holds a row that U feeds
        assert set(cls[st.fed]) == ({0, 2} if seg == 4 else {0, 1, 2})
    assert set(vc.row_class(st, 0)) == {0, 1}
    for D, ch in vc.POISON.items():
        assert len(ch) == 3 and max(ch) < D
    assert vc.POISON[264][1] // 4 >= 1 and vc.POISON[264][2] >= 256, "another lane, and the second channel tile"


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_group_A_scaling(oracle, D):
    st = vc.structure(oracle)
    T = vc.tables(D)
    cases = vc.only(vc.cases_A(D), D) + (vc.only(vc.cases_A_half(D), D))
    assert cases
    for case in cases:
        base = vc.reference(oracle, st, case, T)
        _close(case, case.kinds(), base, vc.numpy_reference(oracle, st, case, T), 1.0, f"D={D} {case.name}")
        for c in vc.SCALES:
            Tc = T.with_x(T.x * np.float32(c))
            refs = vc.reference(oracle, st, case, Tc)
            for kind, r, b in zip(case.kinds(), refs, base):
                if r.dtype == np.float32:
                    assert np.array_equal(_bits(r), _bits(b * np.float32(c))), f"D={D} {case.name} c={c}: the oracle is equivariant"
            _close(case, case.kinds(), refs, vc.numpy_reference(oracle, st, case, Tc), c, f"D={D} {case.name} c={c:.1e}")


def test_group_A_half_tables():
    """bf16 rows of randn scale exactly by the fp32 scales, the fp16 rows by theirs: every element stays normal"""
    import torch
    T = vc.tables(8)
    xb = torch.from_numpy(T.x).to(torch.bfloat16)
    for c in vc.SCALES:
        assert torch.equal((xb * c).float(), xb.float() * c) and bool(((xb * c).float().abs() >= 2.0 ** -126).all())
    x16 = torch.from_numpy(T.x16)
    assert float(x16.abs().min()) >= 0.25 and float(x16.abs().max()) < 4.0
    for c in vc.FP16_SCALES:
        y = x16 * c
        assert torch.equal(y.float(), x16.float() * c) and float(y.abs().min()) >= 2.0 ** -14 and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_group_B_subnormals(oracle, D):
    st = vc.structure(oracle)
    T = vc.tables(D)
    tiny = T.with_x(np.full((vc.N, D), vc.TINY, np.float32))
    assert tiny.x.min() > 0 and _bits(tiny.x).max() == 1
    want = (st.indeg[:, None] * np.float64(vc.TINY)) * np.ones((1, D))
    for case in vc.only(vc.cases_B_exact(D), D):
        (ref,) = vc.reference(oracle, st, case, tiny)
        assert np.array_equal(ref.astype(np.float64), want), f"D={D} {case.name}: indeg 2^-149, exactly"
        assert np.array_equal(vc.weights(oracle, st, case, D), np.ones((vc.N_EDGES, D), np.float32))
    small = T.with_x(T.x * np.float32(2.0 ** -130))
    assert np.abs(small.x).max() < 2.0 ** -126 and (small.x != 0).mean() > 0.99
    for case in vc.only(vc.cases_B_drawn(D), D):
        (ref,), (npr,) = vc.reference(oracle, st, case, small), vc.numpy_reference(oracle, st, case, small)
        bar = vc.subnormal_bar(st, npr, case.kinds()[0])
        assert (np.abs(ref.astype(np.float64) - npr) <= bar).all(), f"D={D} {case.name}: the oracle inside the subnormal bar"
        assert np.abs(ref).max() > 0


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_group_C_containment(oracle, D):
    st = vc.structure(oracle)
    T = vc.tables(D)
    Tp = T.with_x(vc.poisoned(T.x, D))
    assert (~np.isfinite(Tp.x)).sum() == 3 and np.isfinite(np.delete(Tp.x, vc.U, 0)).all()
    H = vc.hit_mask(st, D)
    assert H.sum() == 3 * len(st.fed)
    for case in vc.only(vc.cases_C(D), D) + vc.only(vc.cases_C_half(D), D):
        W = vc.weights(oracle, st, case, D)
        assert (W != 0).all(), "zero weights are another contract (stag_agg_fwd_w1)"
        if case.spec.kind == "explicit":
            assert (W > 0).all()
        clean, bad = vc.reference(oracle, st, case, T), vc.reference(oracle, st, case, Tp)
        npr = vc.numpy_reference(oracle, st, case, Tp)
        for kind, c, b, n in zip(case.kinds(), clean, bad, npr):
            what = f"D={D} {case.name} ({kind})"
            assert np.isfinite(c).all()
            if kind in ("rows", "mc"):
                hit = np.broadcast_to(H, b.shape)
                assert np.array_equal(~np.isfinite(b), hit), f"{what}: the non-finite elements are exactly H"
                assert np.array_equal(_bits(b)[~hit], _bits(c)[~hit]), f"{what}: bit-identical outside H"
                assert np.array_equal(np.isnan(b), np.isnan(n)) and np.array_equal(b[np.isinf(b)], n[np.isinf(b)]), what
            elif kind == "chan":
                hit = np.zeros(D, bool)
                hit[list(vc.POISON[D])] = True
                assert np.array_equal(~np.isfinite(b), hit), f"{what}: exactly the poisoned channels"
            else:
                hit = np.zeros((vc.N_EDGES, 1), bool)
                hit[st.eid_from_u] = True
                assert np.array_equal(~np.isfinite(b), hit), f"{what}: exactly the edges that leave row U"
                assert np.array_equal(b[~hit], c[~hit])


def _draws(O, st, view, D, kind):
    """z or u of every (edge, channel): Normal(0, 1) / Uniform(0, 1) at the same counters"""
    case = vc.Case("draws", "fwd", vc.Spec(kind, 0.0, 1.0), view=view)
    return vc.weights(O, st, case, D)


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_group_D_parameter_edges(oracle, D):
    st = vc.structure(oracle)
    T = vc.tables(D)
    cases = vc.only(vc.cases_D(oracle, st, D), D) + vc.only(vc.cases_D_half(D), D)
    kept = []
    for case in cases:
        sp, what = case.spec, f"D={D} {case.name}"
        dn = sp.dn or D
        W = vc.weights(oracle, st, case, D, in_norm=False)
        full = lambda p: np.broadcast_to(np.asarray(p, np.float32), W.shape)
        if sp.kind == "bernoulli":
            p = full(sp.p0)
            assert set(np.unique(W)) <= {0.0, 1.0}
            assert (W[p == 0.0] == 0.0).all() and (W[p == 1.0] == 1.0).all(), f"{what}: p = 0 never, p = 1 always"
        elif sp.kind == "normal" and not sp.p1_log and not sp.relu and np.all(np.asarray(sp.p1) == 0):
            assert np.array_equal(_bits(W), _bits(full(sp.p0))), f"{what}: scale 0 gives loc, bit for bit"
            z = _draws(oracle, st, case.view, dn, "normal")
            assert np.array_equal(vc.weights(oracle, st, case, D, deriv=2), np.repeat(z, D // dn, 1) if dn != D else z)
            assert (vc.weights(oracle, st, case, D, deriv=1) == 1.0).all()
        elif sp.kind == "uniform":
            assert np.array_equal(_bits(W), _bits(full(sp.p0))), f"{what}: low == high gives low, bit for bit"
            if not sp.in_norm:
                u = _draws(oracle, st, case.view, dn, "uniform")
                u = np.repeat(u, D // dn, 1) if dn != D else u
                assert np.array_equal(vc.weights(oracle, st, case, D, deriv=2), u)
                assert np.array_equal(vc.weights(oracle, st, case, D, deriv=1), np.float32(1.0) - u)
        elif sp.relu and case.zero:
            assert (W == 0).all() and (vc.weights(oracle, st, case, D, deriv=1) == 0).all()
            assert (vc.weights(oracle, st, case, D, deriv=2) == 0).all(), f"{what}: every weight and derivative is 0"
        elif sp.relu:
            kept.append((W > 0).mean() if dn == D else (W[:, 0] > 0).mean())
            if sp.has_derivs and case.entry in ("bwd", "bwd_dp", "bwd_edge"):
                assert np.array_equal(vc.weights(oracle, st, case, D, deriv=1), (W > 0).astype(np.float32)), "the 1[w > 0] mask"
        elif sp.p1_log:
            assert np.isfinite(W).all() and np.abs(W).max() > 0
            if case.norm > 1:
                assert np.abs(W).max() > 1e6
            else:
                assert 0 < np.abs(W).max() < 1e-5
        refs, nps = vc.reference(oracle, st, case, T), vc.numpy_reference(oracle, st, case, T)
        _close(case, case.kinds(), refs, nps, case.norms(), what)
        for r, norm in zip(refs, case.norms()):
            assert np.isfinite(r).all()
            if case.zero:
                assert not np.asarray(r).any(), f"{what}: 0 everywhere"
            elif case.norm != 1.0:
                assert np.abs(np.asarray(r, np.float64) / norm).max() > 0.1, "the normalised outputs are of order one"
    # Normal(-2, 1) under relu keeps P(z > 2) = 2.3 % of the weights: neither empty nor ordinary
    assert kept and all(0.01 <= k <= 0.10 for k in kept), kept


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_group_D_bernoulli_tables(oracle, D):
    """The [E, D] table holds the draw itself on the in-edges of the 40-edge row: u < p fails at p = u and holds one float
    above; the rows whose every in-edge has p = 0 get the in-norm factor 1 and sum to 0."""
    st = vc.structure(oracle)
    pc, pe, pd, e40 = vc.bernoulli_tables(oracle, st, D)
    assert set(pc[:3]) == {0.0, 1.0, pc[2]} and 0 < pc[2] < 1
    for tab in (pe, pd):
        assert (tab == 0).any() and (tab == 1).any() and ((tab > 0) & (tab < 1)).any()
    case = vc.Case("pd", "fwd", vc.Spec("bernoulli", pd, in_norm=True))
    W = vc.weights(oracle, st, case, D, in_norm=False)
    assert (W[e40][:, 0::2] == 0).all() and (W[e40][:, 1::2] == 1).all()
    out, ns = oracle.agg_fwd(st.ogt, vc.tables(D).x, case.spec.o(oracle, D), want_norm_scale=True)
    for r in (vc.ROW1, vc.ROW3, vc.ROW20, vc.HUB):
        assert (ns[r] == 1.0).all() and not out[r].any(), "cur == 0: scale 1, sum 0"
    assert (ns[vc.ROW40, 1::2] == 1.0).all() and not out[vc.ROW40, 0::2].any()
