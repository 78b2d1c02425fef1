"""Everything tests/test_gpu_row_ladder.py takes for granted, without a GPU: the ladder graph (tests/row_ladder_cases.py) has
the degrees, permutations and out-degrees it promises; the host planner cuts it into the units the lengths were chosen for
(the light | heavy boundary between 16 and 17 edges, a whole row of seg_len and a cut row of seg_len + 1, 16 | 17 | 18 | 33
segments); the unit batches of the cooperative GAT kernels close on the unit cap, on the edge cap, on a single unit and on
an empty unit; the exact cases are exact (every sum of |terms| is a multiple of 1/4 below 2^22) and the oracle agrees with
a float64 numpy loop on them bit for bit; and the float64 oracle and a float32 restatement of every TOL case lie within
util.TOL of each other (STAG_PRINT_ERR=1 prints each distance), so the plain bar is the right one for rows of at most 132
terms.  For the wide edge embedding: SiLU and SiLU' are exact at the five pre-activations of its exact case, its sums are
multiples of 1/2 below 2^22, and a float32 restatement of its N(0, 1) case meets util.assert_close_cond's bar."""
import numpy as np
import pytest

import row_ladder_cases as rl
from util import TOL, assert_close, scaled_err


@pytest.fixture(scope="module")
def st(oracle):
    return rl.structure(oracle)


def test_the_ladder(st):
    rl.check_structure(st)
    assert rl.N_EDGES == 1755
    assert set(range(34)) <= set(st.indeg.tolist()), "two full trips and one edge at 16 edges per trip"
    assert {17 + 8 * j + r for j in range(3) for r in range(8)} == set(range(17, 41)), "every residue of 8, three times"


@pytest.mark.parametrize("seg_len", rl.PLAN_SEGS)
def test_the_plans(st, seg_len):
    p = rl.host_plan(st.ogt.indptr, seg_len)
    rl.check_plan(st, seg_len, p["n_units"], p["n_long"], p["n_seg"], p["n_heavy"], p["segs"], p["units"])
    if seg_len == 64:
        assert (p["n_units"], p["n_seg"], p["n_heavy"]) == (105, 16, 42)
    else:
        assert (p["n_units"], p["n_seg"], p["n_heavy"]) == (481, 430, 430)
        # added group by group: 65 and 68 (one group and one partial), 69, 127 and 128 (two full groups), 129 and 132
        assert sorted(k for k in p["segs"].values() if k > rl.COMBINE_GROUP) == [17, 17, 18, 32, 32, 33, 33]
        assert sorted(k for k in p["segs"].values() if k <= rl.COMBINE_GROUP)[-2:] == [16, 16], "63 and 64: the last rows not grouped"
    # the transposed CSR (the GAT backward's source pass): its rows run over the out-degrees
    pt = rl.host_plan(st.og.indptr, seg_len)
    whole = pt["units"][pt["n_seg"]:, 2]
    assert whole[-1] == 0 and pt["n_long"] == (st.outdeg > seg_len).sum()


def test_the_batches(st):
    facts = {}
    for seg_len in rl.PLAN_SEGS:
        p = rl.host_plan(st.ogt.indptr, seg_len)
        ptr = rl.host_blocks(p["units"])
        assert ptr[0] == 0 and ptr[-1] == p["n_units"] and (np.diff(ptr) > 0).all()
        facts[seg_len] = rl.batch_facts(p["units"], ptr)
    rl.check_batches(facts)
    assert facts[64][-2][:3] == (32, 73, "units") and facts[64][-1][0] == 15 and facts[64][-1][3] == 0
    assert facts[64][1][:3] == (4, 235, "edges")
    assert facts[4][-1] == (1, 0, "end", 0) and facts[4][0][:3] == (32, 128, "units")


def _exact_cases(D, half):
    return rl.cases_exact_half(D) if half else rl.cases_exact(D)


EXACT = [(D, False) for D in rl.WIDTHS] + [(D, True) for D in rl.HALF_WIDTHS]


@pytest.mark.parametrize("D,half", EXACT)
def test_the_exact_cases_are_exact(oracle, st, D, half):
    """sum |w| |x| ss ds of every row stays below 2^22 and every term is a multiple of 1/4: exact in fp32 in any order.  The
    oracle and the float64 loop give the same numbers, bit for bit."""
    T = rl.tables(D, True)
    for a in (T.x, T.own, T.w, T.w1):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 8
    assert np.abs(T.w).max() <= 4 and set(np.unique(T.ss)) | set(np.unique(T.ds)) <= {0.5, 1.0, 2.0}
    for dt in ("bfloat16", "float16"):
        assert np.array_equal(rl.half_table(T, dt)[1], T.x)
    for case in _exact_cases(D, half):
        bound = rl.abs_terms(oracle, st, case, T)
        assert bound < 2.0 ** 22 and 132 * 8 * 4 * 4 < 2.0 ** 22, (case.name, bound)
        W = rl.weights(oracle, st, case, D)
        assert np.array_equal(W, np.round(W)), "integer weights (Bernoulli: 0 | 1)"
        if case.spec.kind == "bernoulli":
            assert 0.3 < W.mean() < 0.7 and set(np.unique(W)) == {0.0, 1.0}
        ref, loop = rl.reference(oracle, st, case, T), rl.numpy_reference(oracle, st, case, T)
        for r, l in zip(ref, loop):
            assert np.array_equal(np.asarray(r, np.float64), l), f"D={D} {case.name}: the oracle is not the float64 loop"
            assert np.array_equal(l * 4, np.round(l * 4))
    if half:
        return
    # stag_agg_max_bwd, stag_agg_bwd_w, stag_segment_reduce
    for kind in ("none", "explicit"):
        W, out, cnt, gout, dx, dw = rl.max_case(oracle, st, D, kind)
        Wm = np.ones((rl.N_EDGES, D), np.float32) if W is None else W
        assert np.array_equal(out, rl.numpy_max(st.ogt, T.x, Wm).astype(np.float64))
        assert (cnt[st.indeg > 0] >= 1).all() and (cnt[st.indeg == 0] == 0).all() and cnt.max() > 1, "ties are met"
        assert np.array_equal(gout / np.maximum(cnt, 1), np.round(gout / np.maximum(cnt, 1)))
        assert np.abs(dx).max() < 2.0 ** 22 and np.array_equal(dx, np.round(dx)) and np.abs(dx).max() > 0
    dw = rl.bwd_w_exact(st, T)
    assert np.array_equal(dw, oracle.agg_bwd_w(st.ogt, T.x, T.own, src_scale=T.ss).astype(np.float64))
    xe = rl.segment_table(D)
    assert np.array_equal(rl.segment_sums(st, xe), oracle.segment_reduce(xe, st.ogt.indptr).astype(np.float64))


@pytest.mark.parametrize("D,half", EXACT)
def test_the_oracle_against_a_float32_restatement(oracle, st, D, half):
    """Every TOL case: the float64 oracle and the same sums in float32, term by term in edge order without compensation,
    within util.TOL — the plain bar holds on rows of at most 132 terms, no conditioned bar is needed."""
    T = rl.tables(D, False)
    if half:
        T = T.with_x(rl.half_table(T, "bfloat16")[1])
    for case in (rl.cases_tol_half(D) if half else rl.cases_tol(D)):
        ref = rl.reference(oracle, st, case, T)[0]
        assert_close(rl.f32_reference(oracle, st, case, T), ref, what=f"float32 restatement D={D} {case.name}")
    if half:
        return
    refs = rl.bwd_w_reference(oracle, st, T, rl.MCB_S, rl.MCB_STRIDE, T.ds)
    one = rl.bwd_w_reference(oracle, st, T, 1, rl.MCB_STRIDE, None)
    for r in refs + one:
        assert r.shape == (rl.N_EDGES, D) and np.isfinite(r).all() and np.abs(r).max() > 0


def test_the_edge_embedding_s_classes_are_exact():
    """The five pre-activations of the exact edge-embedding case: float64 SiLU and SiLU' rounded to fp32 are the class table
    (so is the documented formula in numpy float32), and the table is what own + other can give."""
    import edge_embed_range_cases as ec
    f = np.float32
    sums = {float(f(a) + f(b)) for a in rl.EMBED_OWN for b in rl.EMBED_OTHER}
    assert sums == set(rl.EMBED_CLASS) and len(sums) == 5
    for pre, (h, dh) in rl.EMBED_CLASS.items():
        h64, d64 = ec.silu64(np.float64(pre))
        assert f(h64) == f(h) and f(d64) == f(dh), (pre, h64, d64)
        h32, d32 = ec.silu32(f(pre))
        assert h32 == f(h) and d32 == f(dh), (pre, h32, d32)
    assert sorted(v[1] for v in rl.EMBED_CLASS.values()) == [0.0, 0.0, 0.5, 1.0, 1.0]


@pytest.mark.parametrize("orient", list(rl.EMBED_ORIENT))
@pytest.mark.parametrize("hidden", rl.EMBED_WIDTHS)
def test_the_edge_embedding_s_exact_case_is_exact(st, hidden, orient):
    """Every term g SiLU' is a multiple of 1/2, sum |terms| of every row stays below 2^22: any order of fp32 additions,
    compensated or not, gives the float64 sum.  Every edge counts in some channel, so a dropped edge changes its row."""
    view = rl.embed_view(st, orient)
    own, other, g = rl.embed_tables(hidden, True, orient)
    assert set(np.unique(own)) <= set(rl.EMBED_OWN) and set(np.unique(other)) <= set(rl.EMBED_OTHER)
    assert np.array_equal(g, np.round(g)) and np.abs(g).max() <= 8 and np.abs(g).min() >= 1
    ref, ab = rl.embed_bwd_reference(view, own, other, g, exact=True)
    assert ab.max() < 2.0 ** 22 and 132 * 8 < 2.0 ** 22
    assert np.array_equal(ref * 2, np.round(ref * 2)) and np.array_equal(ref, ref.astype(np.float32).astype(np.float64))
    # the reference again from the class table
    pre = own[view.dst_of_pos] + other[view.indices]
    dh = np.vectorize(lambda v: rl.EMBED_CLASS[float(v)][1])(pre)
    again = np.zeros_like(ref)
    np.add.at(again, view.dst_of_pos, g[view.eid].astype(np.float64) * dh)
    assert np.array_equal(again, ref)
    counts = (dh != 0).sum(1)
    assert (counts > 0).mean() > (0.9 if hidden == 3 else 0.999), "an edge's term is nonzero in some channel"
    assert ref.shape == (rl.N, hidden) and (ref[np.diff(view.indptr) == 0] == 0).all()


@pytest.mark.parametrize("orient", list(rl.EMBED_ORIENT))
@pytest.mark.parametrize("hidden", rl.EMBED_WIDTHS)
def test_the_edge_embedding_s_tol_case_against_a_float32_restatement(st, hidden, orient):
    """N(0, 1) tables: the formula in float32, terms added in position order without compensation, within
    util.assert_close_cond's bar of the float64 reference (the plain distance is printed under STAG_PRINT_ERR=1)."""
    import edge_embed_range_cases as ec
    from util import assert_close_cond
    view = rl.embed_view(st, orient)
    own, other, g = rl.embed_tables(hidden, False, orient)
    ref, ab = rl.embed_bwd_reference(view, own, other, g)
    term = g[view.eid] * ec.silu32(own[view.dst_of_pos] + other[view.indices])[1]
    got = np.zeros((rl.N, hidden), np.float32)
    for p in range(view.n_edges):
        got[view.dst_of_pos[p]] += term[p]
    assert_close_cond(got, ref, ab, what=f"float32 restatement {orient} hidden={hidden}")


def test_the_edge_embedding_s_forward_tails():
    for hidden, lanes in rl.EMBED_FWD_WIDTHS.items():
        nchunk = (hidden + 3) // 4
        assert min(64, max(4, 1 << (nchunk - 1).bit_length())) == lanes, "lanes_for(nchunk, 4) of csrc/entry_args.hpp"
        T = 256 // lanes
        sizes = rl.embed_fwd_sizes(lanes)
        assert {T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1, 1} == set(sizes) and sizes[-1] == 4 * T + 1
        src, dst, ps, pd = rl.embed_fwd_case(hidden, sizes[-1])
        pre = ps[src] + pd[dst]
        assert set(np.unique(pre).tolist()) <= set(rl.EMBED_CLASS) and len(np.unique(pre)) == 5


@pytest.mark.parametrize("H,F", rl.GAT_SHAPES)
def test_the_gat_oracle_against_a_float32_restatement(oracle, st, H, F):
    from stag_amd import ops
    assert ops.gat_cooperative_shape(H, F, 64) == ((H, F) in rl.GAT_COOPERATIVE) == ops.gat_cooperative_shape(H, F, 4)
    if (H, F) in rl.GAT_LANES:
        assert ops.gat_lanes_per_head(F) == rl.GAT_LANES[H, F]
    p = rl.gat_inputs(H, F)
    for name in rl.GAT_WEIGHTINGS:
        spec = rl.gat_spec(oracle, name, H, p["w"])
        out, attn = oracle.gat_fwd(st.ogf, p["el"], p["er"], p["ft"], rl.GAT_SLOPE, spec, want_attn=True)
        W = None if name == "none" else oracle.noise_materialize(st.ogf, spec, H)
        out32, attn32 = rl.gat_f32(st.ogf, p["el"], p["er"], p["ft"], rl.GAT_SLOPE, W)
        assert_close(out32, out, what=f"float32 restatement GAT ({H}, {F}) {name} out")
        assert_close(attn32, attn, what=f"float32 restatement GAT ({H}, {F}) {name} attn")
        sums = np.zeros((rl.N, H))
        np.add.at(sums, st.row_of_pos, attn[st.ogf.eid].astype(np.float64))
        assert scaled_err(sums[st.indeg > 0], 1.0) <= TOL and (sums[st.indeg == 0] == 0).all()


# ---- stag_agg_bwd_pedge over the source-major view -------------------------------------------------------------------------
def test_bwd_pedge_source_rows(st):
    """The out-degrees carry 0..20 once each and more than 16 elsewhere: without a plan and at seg_len 64 no source row is
    cut, rows of up to 16 edges are plain sums and the longer ones Kahan units; at seg_len 4 every row of more than 4 edges
    is cut, up to 6 segments, and the rows of 0..4 stay whole."""
    s = st.ogs
    assert np.array_equal(np.diff(s.indptr), st.outdeg) and sorted(s.nidx) == list(range(rl.N_EDGES))
    assert np.array_equal(st.ogf.eid[s.nidx], s.eid), "nidx: the position of the same edge in the forward view"
    assert set(rl.OUT_LADDER) <= set(st.outdeg.tolist()) and st.outdeg.max() <= 64
    for seg, classes in ((0, {0, 1}), (64, {0, 1}), (4, {0, 2})):
        cls = rl.source_row_class(st, seg)
        assert set(cls.tolist()) == classes
        if seg:
            p = rl.host_plan(s.indptr, seg)
            assert p["n_long"] == (cls == 2).sum() and p["n_heavy"] - p["n_seg"] == (cls == 1).sum()
    p4 = rl.host_plan(s.indptr, 4)
    assert max(p4["segs"].values()) == -(-int(st.outdeg.max()) // 4) and min(p4["segs"].values()) == 2
    assert {int(d) for d in st.outdeg[rl.source_row_class(st, 4) == 0]} == {0, 1, 2, 3, 4}
    assert (rl.source_row_class(st, 64) == 1).sum() >= 10 and (st.outdeg == 17).any() and (st.outdeg == 16).any()


@pytest.mark.parametrize("D", rl.PEDGE_WIDTHS)
def test_bwd_pedge_references(oracle, st, D):
    """Exact group: w == loc and d/dloc == 1 bit for bit, every term and sum a multiple of 1/4 below 2^22, the fp32 restatement
    equals the float64 one.  TOL group: the float64 restatement against the oracle's own entry points (agg_fwd on the
    source-major view, agg_bwd_w per derivative on the forward view) and against its fp32 restatement at util.TOL."""
    exact_spec, tol_spec = rl.pedge_specs(D)
    T = rl.tables(D, True)
    case = rl.Case("weights", "fwd", exact_spec, view="f")
    assert np.array_equal(rl.weights(oracle, st, case, D), T.w) and (rl.weights(oracle, st, case, D, deriv=1) == 1.0).all()
    dx, dp0, dp1, ab = rl.pedge_reference(oracle, st, T, exact_spec)
    for a in (dx, dp0, ab):
        assert np.array_equal(a * 4, np.round(a * 4)) and np.abs(a).max() < 2.0 ** 22
    fx, f0, _, _ = rl.pedge_reference(oracle, st, T, exact_spec, f32=True)
    assert fx.dtype == np.float32 and np.array_equal(fx.astype(np.float64), dx) and np.array_equal(f0.astype(np.float64), dp0)
    assert np.abs(dx).max() > 0 and np.abs(dp0).max() > 0
    T = rl.tables(D, False)
    dx, dp0, dp1, _ = rl.pedge_reference(oracle, st, T, tol_spec)
    assert_close(oracle.agg_fwd(st.ogs, T.x, tol_spec.o(oracle, D), src_scale=T.ss, dst_scale=T.ds), dx, what=f"D={D} dx: the oracle")
    xs, gg = T.own * T.ds[:, None], T.x * T.ss[:, None]
    for dv, ref in ((1, dp0), (2, dp1)):
        got = oracle.agg_bwd_w(st.ogf, xs, gg, spec=tol_spec.o(oracle, D, deriv=dv)).astype(np.float64)
        sc = max(1.0, float(np.abs(ref).max()))
        assert_close(got / sc, ref / sc, what=f"D={D} dp{dv - 1}: the oracle")
    fx, f0, f1, _ = rl.pedge_reference(oracle, st, T, tol_spec, f32=True)
    assert_close(fx, dx, what=f"D={D} dx: the fp32 restatement")
