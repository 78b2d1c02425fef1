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
For tests/test_gpu_value_range_grad.py (the per-edge gradient kernels, the max reducer's backward and count, stag_coldot,
stag_segment_reduce, in-norm weights) the second half of this module holds: the float64 statements against the oracle's
own entry points; A: no intermediate of any case within a factor 4 of 2^-126 under 2^-100 nor of the float maximum under
2^100; B: an fp32 emulation of the reference, rounded where the kernels round, inside 1e-5 |ref| + r 2^-149 f; C: the
affected sets on the float64 statement, the memory neighbours of the poisoned rows and of the poisoned edge, and the max
backward's dw set (wider than the edges that leave U); D: the derivative identities, the planted duplicates and their
segment boundary, the oracle's in-norm weights.
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


# ---- the per-edge gradient, max-backward and small reduction entry points (tests/test_gpu_value_range_grad.py) --------
def _oracle_grad(O, st, gc, D, x, g_all, ss, ds):
    """The oracle's own fp32 statement of a gradient case: stag_agg_bwd_w_cpu per derivative and sample on the scaled
    rows (as tests/test_gpu_bwd_pedge.py forms it), agg_fwd for dx."""
    outs = []
    xs = (x * ss[:, None]).astype(np.float32) if gc.ss else x
    for _, d in gc.outputs():
        if d == 0:
            outs.append(O.agg_fwd(st.ogt, x, gc.spec.o(O, D), src_scale=ss, dst_scale=ds))
            continue
        tot = 0.0
        for s in range(gc.S):
            gs = (g_all[s] * ds[:, None]).astype(np.float32) if gc.ds else g_all[s]
            spec = None if d is None else gc.spec.o(O, D, deriv=d, offset=vc.OFFSET + s * vc.GRAD_STRIDE)
            tot = tot + O.agg_bwd_w(st.ogt, xs, gs, spec=spec, reduce_k=gc.reduce_k).astype(np.float64)
        outs.append(tot)
    return outs


def _close_grad(gc, got, refs, what, scale=1.0):
    for (name, _), kind, a, b, norm in zip(gc.outputs(), gc.kinds(), got, refs, gc.norms()):
        a, b = np.asarray(a, np.float64) / (scale * norm), np.asarray(b, np.float64) / (scale * norm)
        sc = vc.out_scale(kind, b)
        assert_close(a / sc, b / sc, what=f"{what} {name}")


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_grad_group_A_margins_and_reference(oracle, D):
    """Every group-A gradient case: the float64 restatement agrees with the oracle's fp32 entry points, and no
    intermediate of the 2^-100 launch falls below MARGIN 2^-126 nor one of the 2^100 launch above FLT_MAX / MARGIN —
    what makes out(c x) == c out(x) a statement about the kernel and not about the tables."""
    st, GT = vc.structure(oracle), vc.grad_tables(D)
    assert np.abs(GT.x).min() >= 1.0 and np.abs(GT.g_all).min() >= 4.0 and np.abs(GT.g_all).max() < 16.0
    worst = [np.inf, 0.0]
    for gc in vc.cases_grad_A(D):
        track = {}
        refs = vc.grad_reference(oracle, st, gc, D, GT.x, GT.g_all, GT.ss, GT.ds, track=track)
        _close_grad(gc, _oracle_grad(oracle, st, gc, D, GT.x, GT.g_all, GT.ss, GT.ds), refs, f"D={D} {gc.name}: oracle vs float64")
        assert track["lo"] * min(vc.SCALES) >= vc.MARGIN * 2.0 ** -126, f"D={D} {gc.name}: smallest intermediate {track['lo']:.3e}"
        assert track["hi"] * max(vc.SCALES) <= vc.FLT_MAX / vc.MARGIN, f"D={D} {gc.name}: largest intermediate {track['hi']:.3e}"
        worst = [min(worst[0], track["lo"]), max(worst[1], track["hi"])]
        assert gc.S == 1 or gc.S == 7, "passes of 4, 2 and 1"
    print(f"D={D}: intermediates between 2^{np.log2(worst[0]):.1f} and 2^{np.log2(worst[1]):.1f}")


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_grad_group_B_bars(oracle, D):
    """r and f of every output (vc.grad_subnormal_bars): the fp32 emulation of the reference, rounded where the kernels
    round, stays inside 1e-5 |ref| + r 2^-149 f on x = randn 2^-130, and the outputs are not all zero."""
    st, GT, T = vc.structure(oracle), vc.grad_tables(D), vc.tables(D)
    xs = T.x * np.float32(2.0 ** -130)
    assert np.abs(xs).max() < 2.0 ** -126 and (xs != 0).mean() > 0.99
    for gc in vc.cases_grad_B(D):
        refs = vc.grad_reference(oracle, st, gc, D, xs, GT.grand, GT.ss, GT.ds)
        emul = vc.grad_reference(oracle, st, gc, D, xs, GT.grand, GT.ss, GT.ds, f32=True)
        bars = vc.grad_subnormal_bars(oracle, st, gc, D, GT.grand, GT.ds, refs)
        for (name, _), r, e, bar in zip(gc.outputs(), refs, emul, bars):
            assert e.dtype == np.float32 and np.abs(r).max() > 0
            over = np.abs(e.astype(np.float64) - r) / bar
            assert over.max() <= 1.0, f"D={D} {gc.name} {name}: the fp32 emulation is {over.max():.2f} x the bar"
            assert (np.abs(r) < 2.0 ** -120).all(), "the outputs are subnormal or next to it"
    # the exact group: integers times 2^-149
    assert np.abs(GT.gint).max() <= 3 and (GT.gint != 0).mean() > 0.5
    tiny = np.full((vc.N, D), vc.TINY, np.float32)
    for rk in (False, True):
        gc = vc.GradCase("exact", "bwd_w", None, "plain", reduce_k=rk, ss=False)
        (ref,) = vc.grad_reference(oracle, st, gc, D, tiny, GT.gint[None], GT.ss, GT.ds)
        (emu,) = vc.grad_reference(oracle, st, gc, D, tiny, GT.gint[None], GT.ss, GT.ds, f32=True)
        assert np.array_equal(emu.astype(np.float64), ref), "exact in fp32"
        want = np.zeros((vc.N_EDGES, D))
        want[st.ogt.eid] = GT.gint[st.row_of_pos] * np.float64(vc.TINY)
        assert np.array_equal(ref, want.sum(1, keepdims=True) if rk else want)


@pytest.mark.parametrize("D", (6, 264))
def test_grad_group_C_sets(oracle, D):
    """The affected sets of group C on the float64 restatement: exactly the edges that leave U / enter V0 / the edge EP are
    non-finite (or changed), and the memory neighbours the leak would reach are clean edges of other rows."""
    st, GT, T = vc.structure(oracle), vc.grad_tables(D), vc.tables(D)
    g = st.ogt
    ep = vc.poison_edge(st)
    assert ep + 1 < vc.N_EDGES, "a parameter row follows EP's in memory"
    row_of_eid = np.empty(vc.N_EDGES, np.int64)
    row_of_eid[g.eid] = st.row_of_pos
    col_of_eid = np.empty(vc.N_EDGES, np.int64)
    col_of_eid[g.eid] = g.indices
    assert row_of_eid[ep] == vc.HUB and row_of_eid[ep + 1] != vc.HUB, "and belongs to an edge of another row"
    assert col_of_eid[ep] != vc.U and col_of_eid[ep + 1] != vc.U and row_of_eid[ep + 1] != vc.V0
    assert vc.U + 1 < vc.N and vc.V0 + 1 < vc.N and st.indeg[vc.V0 + 1] > 0 and vc.V0 in st.fed
    # the gradient rows that follow a poisoned one in memory: edge e + 1 of an edge e that leaves U is not itself hit
    hit_e = np.zeros(vc.N_EDGES, bool)
    hit_e[st.eid_from_u] = True
    nxt = st.eid_from_u[st.eid_from_u + 1 < vc.N_EDGES] + 1
    assert (~hit_e[nxt]).any(), "a clean gradient row follows a poisoned one"
    xp = vc.poisoned_row(T.x, vc.U, D)
    gp = np.array(GT.grand)
    gp[0] = vc.poisoned_row(gp[0], vc.V0, D)
    gp5 = np.array(GT.grand)
    gp5[vc.GRAD_POISON_SAMPLE] = vc.poisoned_row(gp5[vc.GRAD_POISON_SAMPLE], vc.V0, D)
    for gc in vc.cases_grad_C(D):
        from_u, into_v0, at_ep = vc.poison_sets(st, D, gc.reduce_k)
        clean = vc.grad_reference(oracle, st, gc, D, T.x, GT.grand, GT.ss, GT.ds)
        runs = [("x[U]", vc.grad_reference(oracle, st, gc, D, xp, GT.grand, GT.ss, GT.ds), from_u),
                ("g[V0]", vc.grad_reference(oracle, st, gc, D, T.x, gp5 if gc.S > 1 else gp, GT.ss, GT.ds), into_v0)]
        for which in (("p0", "p1") if gc.spec is not None else ()):
            sp = vc.poisoned_param(gc.spec, st, D, which)
            import copy
            gcp = copy.copy(gc)
            gcp.spec = sp
            runs.append((which, vc.grad_reference(oracle, st, gcp, D, T.x, GT.grand, GT.ss, GT.ds), at_ep))
        for tag, bad, hit in runs:
            for (name, d), c, b in zip(gc.outputs(), clean, bad):
                what = f"D={D} {gc.name} {tag} {name}"
                assert np.isfinite(c).all(), what
                if d == 0:
                    H = vc.hit_mask(st, D) if tag == "x[U]" else np.zeros((vc.N, D), bool)
                    if tag in ("p0", "p1"):
                        H[vc.HUB, list(vc.POISON[D])] = True
                    assert np.array_equal(~np.isfinite(b), H), f"{what}: non-finite exactly in its set"
                    assert np.array_equal(b[~H], c[~H])
                    continue
                assert np.array_equal(b[~hit], c[~hit]), f"{what}: unchanged outside the set"
                if tag == "p1" and gc.spec.p1_log and d == 2:       # (d/dloc is 1 and d/dscale is z whatever the parameters)
                    assert not np.isfinite(b[hit]).any(), f"{what}: z e^inf is not finite"
                if tag in ("x[U]", "g[V0]"):
                    assert not np.isfinite(b[hit]).any(), f"{what}: every element of the set is non-finite"


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_grad_group_D_reference(oracle, D):
    st, GT, T = vc.structure(oracle), vc.grad_tables(D), vc.tables(D)
    kept = []
    for gc in vc.cases_grad_D(D):
        what = f"D={D} {gc.name}"
        refs = vc.grad_reference(oracle, st, gc, D, T.x, GT.grand, GT.ss, GT.ds)
        _close_grad(gc, _oracle_grad(oracle, st, gc, D, T.x, GT.grand, GT.ss, GT.ds), refs, f"{what}: oracle vs float64")
        for r in refs:
            assert np.isfinite(r).all()
            assert bool(np.any(r)) != gc.zero, f"{what}: zero exactly when every weight is clamped"
        d1 = vc.weights(oracle, st, vc._wcase(gc.spec), D, deriv=1)
        d2 = vc.weights(oracle, st, vc._wcase(gc.spec), D, deriv=2)
        if "Normal(loc, 0)" in gc.name:
            z = _draws(oracle, st, "t", D, "normal")
            assert (d1 == 1.0).all() and np.array_equal(d2, z), f"{what}: d0 = 1, d1 = z"
        elif "log-scale -16)" in gc.name:
            z = _draws(oracle, st, "t", D, "normal").astype(np.float64)
            assert (d1 == 1.0).all() and np.allclose(d2, z * np.exp(-16.0), rtol=1e-5, atol=0), f"{what}: d1 = z e^-16"
        elif "Uniform(low, low)" in gc.name:
            u = _draws(oracle, st, "t", D, "uniform")
            assert np.array_equal(d1, np.float32(1.0) - u) and np.array_equal(d2, u), f"{what}: 1 - u, u"
        elif "Normal(-2, 1) relu" in gc.name:
            kept.append((d1 > 0).mean())
            assert set(np.unique(d1)) == {0.0, 1.0} and (d2[d1 == 0] == 0).all(), "the 1[w > 0] mask on both derivatives"
    assert len(kept) == 5 and all(0.01 <= k <= 0.10 for k in kept), kept


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_max_fixtures(oracle, D):
    """The max reducer's restatement against vc.numpy_max; the planted duplicates and their segment boundary; the tie
    table; the poisoned forward's count; a tied and a not-tied in-edge of V0 in every poisoned channel."""
    st, GT, T = vc.structure(oracle), vc.grad_tables(D), vc.tables(D)
    g = st.ogt
    for W in (None, T.wpos, T.w):
        m, out, cnt = vc.max_fwd_reference(st, T.x, W)
        want = vc.numpy_max(g, T.x, np.ones((vc.N_EDGES, D), np.float32) if W is None else W)
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt[st.indeg > 0].min(), 1)
        assert (cnt[st.indeg == 0] == 0).all() and (cnt <= st.indeg[:, None]).all()
    # ties: x of five values
    m, out, cnt = vc.max_fwd_reference(st, GT.xint * np.float32(vc.TINY), None)
    assert cnt.max() > 3 and (cnt[vc.HUB] > 1).all(), "many ties"
    _, _, _, _, tied = vc.max_bwd_reference(st, GT.xint * np.float32(vc.TINY), None, out, cnt, cnt.astype(np.float32))
    per_row = np.zeros((vc.N, D), np.int64)
    np.add.at(per_row, st.row_of_pos, tied)
    assert np.array_equal(per_row, cnt), "the ties number cnt per element"
    # planted duplicates
    W, x, pos = vc.planted_duplicates(st, D)
    p = vc.host_plan(g.indptr, 4)
    hub_units = sorted(u[1] for u in p["units"].tolist() if u[3] >= 0 and g.indptr[vc.HUB] <= u[1] < g.indptr[vc.HUB + 1])
    seg_of = [int(np.searchsorted(hub_units, q, side="right")) - 1 for q in pos]
    assert seg_of[0] == seg_of[1] and len(set(seg_of)) == 3, f"two in one segment, two in others: {seg_of}"
    m, out, cnt = vc.max_fwd_reference(st, x, W)
    assert (out[vc.HUB] == 64.0).all() and (cnt[vc.HUB] == 4).all()
    # poisoned x[U]: NaN -> cnt 0 and NaN, +inf -> the number of equal infinities, -inf never wins
    xp = vc.poisoned_row(T.x, vc.U, D)
    m, out, cnt = vc.max_fwd_reference(st, xp, None)
    kinf, knan, kneg = vc.POISON[D]
    assert np.isnan(out[st.fed, knan]).all() and (cnt[st.fed, knan] == 0).all()
    assert (out[st.fed, kinf] == np.inf).all() and cnt[vc.HUB, kinf] == 2 and (cnt[st.fed, kinf] >= 1).all()
    assert np.isfinite(out[st.fed, kneg]).all()
    clean = vc.max_fwd_reference(st, T.x, None)
    H = vc.hit_mask(st, D)
    assert np.array_equal(_bits(out)[~H], _bits(clean[1])[~H]) and np.array_equal(cnt[~H], clean[2][~H])
    # ... and the backward on that out and cnt: dx moves only in the rows that share a destination with U, dw only on the
    # edges that enter a destination U feeds — and there on edges that do NOT leave U too (a row-mate that was maximal)
    Wp = T.wpos
    mc, oc, cc = vc.max_fwd_reference(st, T.x, Wp)
    mp, op, cp = vc.max_fwd_reference(st, xp, Wp)
    rc = vc.max_bwd_reference(st, T.x, Wp, oc, cc, GT.grand[0])
    rp = vc.max_bwd_reference(st, xp, Wp, op, cp, GT.grand[0])
    share = np.unique(g.indices[np.isin(st.row_of_pos, st.fed)])
    Hdx, Hdw = np.zeros((vc.N, D), bool), np.zeros((vc.N_EDGES, D), bool)
    Hdx[np.ix_(share, list(vc.POISON[D]))] = True
    Hdw[np.ix_(g.eid[np.isin(st.row_of_pos, st.fed)], list(vc.POISON[D]))] = True
    same = lambda a, b: (a == b) | (np.isnan(a) & np.isnan(b))
    assert same(rp[0], rc[0])[~Hdx].all() and same(rp[1], rc[1])[~Hdw].all()
    from_u = np.zeros(vc.N_EDGES, bool)
    from_u[st.eid_from_u] = True
    assert (~same(rp[1], rc[1]))[~from_u].any(), "dw of a row-mate of U's edge moves: the set is wider than U's out-edges"
    assert vc.U in share and len(share) < vc.N
    # g[V0] poisoned: in every poisoned channel V0 has a maximal in-edge and one that is not
    m, out, cnt = clean
    rows = slice(g.indptr[vc.V0], g.indptr[vc.V0 + 1])
    tie = m[rows] == out[vc.V0]
    for k in vc.POISON[D]:
        assert tie[:, k].any() and not tie[:, k].all()


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_max_group_A_margins(oracle, D):
    """Every intermediate of the max reducer's group A (messages w x, g / cnt, the terms w gq, x gq, d gq and the running
    sums) keeps MARGIN to 2^-126 under c = 2^-100 and to the float maximum under 2^100.  A running sum may cancel below
    that: its terms are multiples of lo 2^-23 >= 2^-49, so is the sum, and c times it (a multiple of 2^-149) is exact —
    the same argument covers stag_coldot (products of two numbers in [1, 4): multiples of 2^-46) and stag_segment_reduce."""
    st, GT = vc.structure(oracle), vc.grad_tables(D)
    for name, spec in vc.max_specs_A(D).items():
        W = None if spec.kind == "none" else vc.weights(oracle, st, vc._wcase(spec), D)
        d = [vc.weights(oracle, st, vc._wcase(spec), D, deriv=dv) for dv in (1, 2)] if spec.kind in ("normal", "uniform") else [None, None]
        _, out, cnt = vc.max_fwd_reference(st, GT.x, W)
        track = []
        vc.max_bwd_reference(st, GT.x, W, out, cnt, GT.g_all[0], *d, track=track)
        mags = np.concatenate([np.abs(np.asarray(a, np.float64)).ravel() for a in track])
        terms = mags[(mags > 0) & np.isfinite(mags)]
        sums = np.concatenate([np.abs(a).ravel() for a in track if isinstance(a, np.ndarray) and a.shape == (D,) and a.dtype == np.float64])
        lo_terms = min(np.abs(np.asarray(a, np.float64))[np.abs(np.asarray(a, np.float64)) > 0].min() for a in track[-2:])
        assert lo_terms * min(vc.SCALES) >= vc.MARGIN * 2.0 ** -126, f"D={D} {name}: messages and g / cnt, {lo_terms:.3e}"
        assert terms.max() * max(vc.SCALES) <= vc.FLT_MAX / vc.MARGIN
        # every non-zero term of a sum (w gq, d gq, x gq) is large enough for its last bit to survive the scaling
        per_edge = [np.abs(np.asarray(a, np.float64)) for i, a in enumerate(track[:-2])]
        lo = min(a[a > 0].min() for a in per_edge if (a > 0).any())
        assert lo >= 2.0 ** -26, f"D={D} {name}: smallest term or running sum {lo:.3e}"
        assert sums.size


@pytest.mark.parametrize("D", vc.WIDTHS)
def test_in_norm_weights_of_the_oracle(oracle, D):
    """stag_noise_materialize with in-norm: the oracle scales a row's weights by indeg / sum w and leaves a row whose every
    in-edge has p = 0 at exactly 0 — what the device launch is compared with."""
    st = vc.structure(oracle)
    g = st.ogt
    _, pe, pd, _ = vc.bernoulli_tables(oracle, st, D)
    zero_e = np.concatenate([g.eid[g.indptr[r]:g.indptr[r + 1]] for r in (vc.ROW1, vc.ROW3, vc.ROW20, vc.HUB)])
    for p in (pe, pd):
        spec = vc.Spec("bernoulli", p, in_norm=True)
        w0 = oracle.noise_materialize(g, spec.o(oracle, D, in_norm=False), D).astype(np.float64)
        w = oracle.noise_materialize(g, spec.o(oracle, D), D)
        assert not w[zero_e].any() and w.max() > 1.0
        tot = np.zeros((vc.N, D))
        np.add.at(tot, st.row_of_pos, w0[g.eid])
        factor = np.where(tot > 0, st.indeg[:, None] / np.where(tot > 0, tot, 1.0), 1.0)
        want = np.zeros_like(w0)
        want[g.eid] = w0[g.eid] * factor[st.row_of_pos]
        assert_close(w, want, what=f"D={D}: the oracle's in-norm weights")


def test_small_reduction_fixtures():
    """coldot's second size is past the second grid-stride trip (1024 blocks of R rows, R = 256 / lanes across a row)"""
    import value_range_cases as vc2
    for D, R in ((6, 32), (8, 128), (264, 2)):
        elems = D // 4 if D % 4 == 0 else D
        cw = 1
        while cw < elems and cw < 256:
            cw <<= 1
        assert 256 // cw == R and vc2.coldot_big_n(D) > 2 * 1024 * R
    offs = vc2.SEGMENT_OFFSETS
    lens = np.diff(offs)
    assert (lens == 0).any() and lens[0] == 0 and lens[-1] == 0 and {1, 3, 4, 5, 9} <= set(lens.tolist()), "empty, < 4, 4, > 4"
