"""The ladder graph, its tables, the case lists and the references of the row-ladder tests (no tests in here):
tests/test_row_ladder_host.py proves all of it without a GPU, tests/test_gpu_row_ladder.py puts it through the kernels.  Both
import this module, so a row length cannot mean one thing on the host and another on the device.

THE GRAPH: 96 nodes, square.  The destination rows carry, at node ids drawn by a seeded permutation,
  0, 1, ..., 40 once each           without a plan every row is a light unit: two full trips and one edge at the widest block
                                    (16 edges); at seg_len 64 the rows 17..40 are heavy whole rows (Kahan sums): every residue
                                    of the widest round (8 edges) three times
  63, 64, 65, 127, 128, 129         at seg_len 64: a whole row of exactly seg_len, the first row cut in two (33 + 32), 2 | 3
                                    segments
  68, 69, 132                       at seg_len 4: 17, 18 and 33 segments (the 64 above: exactly 16, the last row whose partials
                                    are not added group by group)
  FILL                              the other 46 rows, 1-3 edges each: light blocks are filled
Sources: 21 nodes have out-degree 0, 1, ..., 20 (the backward's source pass walks the transposed CSR), the other 75 share
the remaining edges evenly; which edge takes which source is random, so rows gather a source more than once.  Edge ids are a
permutation that keeps the order inside a row.  One view serves every entry point, as in tests/value_range_cases.py: `ogt`
(rows = destinations, eid and nidx two permutations) and `ogf`, the same rows without nidx (what the plain forward launch
needs); `og` is the transpose (rows = sources).

EXACT CASES: x and g are integers in [-8, 8], explicit weights integers in [-4, 4], the two scales drawn from {0.5, 1, 2},
Bernoulli keeps with p = 0.5 and no in-norm: every term and every partial sum is a multiple of 1/4 below 2^22 in magnitude
(test_row_ladder_host.py holds the fixture to it), so every order of fp32 additions, compensated or not, gives the float64
sum bit for bit.  TOL CASES: N(0, 1) rows, parameters from the middle of their ranges, compared at util.TOL."""
import numpy as np

import value_range_cases as vc

N = 96
LADDER = tuple(range(41))
CUT64 = (63, 64, 65, 127, 128, 129)
CUT4 = (68, 69, 132)
FILL = (1, 2, 3) * 14 + (1, 1, 2, 2)                # the other 46 rows (test_row_ladder_host.py: the batch conditions)
DEGREES = LADDER + CUT64 + CUT4 + FILL
N_EDGES = sum(DEGREES)
OUT_LADDER = tuple(range(21))
SEGS = (0, 64, 4)
PLAN_SEGS = (64, 4)
WIDTHS = (3, 16, 30, 32, 64, 128, 256, 260)
HALF_WIDTHS = (8, 128, 264)
HEAVY_LEN = 16                                      # STAG_HEAVY_LEN, STAG_KAHAN_MIN_LEN
COMBINE_GROUP = 16                                  # kCombineGroup
BLOCK_EDGES, BLOCK_UNITS = 256, 32                  # STAG_BLOCK_EDGES, STAG_BLOCK_UNITS
SEED, OFFSET = vc.SEED, vc.OFFSET
MC_S, MC_STRIDE = vc.MC_S, vc.MC_STRIDE             # stag_agg_fwd_mc: S = 5, a pass of four and one of one (in-norm: 2, 2, 1)
MCE_S, MCE_STRIDE = vc.MCE_S, vc.MCE_STRIDE         # stag_agg_fwd_mc_edge / _pedge: S = 7
MCB_S, MCB_STRIDE = 3, 2                            # stag_agg_bwd_w_mc
GAT_SHAPES = ((1, 4), (3, 4), (4, 16), (8, 64), (4, 256), (4, 5))
GAT_COOPERATIVE = GAT_SHAPES[:5]                    # (4, 5): F % 4 != 0, one unit per team and the composed backward
GAT_LANES = {(1, 4): 1, (3, 4): 1, (4, 16): 4, (8, 64): 16, (4, 256): 64}
GAT_SLOPE = 0.2
GAT_NOISE = dict(seed=23, offset=5)
GAT_MC_S, GAT_MC_STRIDE = 5, 2

_CACHE = {}


class Structure:
    pass


def structure(O):
    """The ladder graph as the oracle's CsrGraph objects (built once)."""
    if "st" in _CACHE:
        return _CACHE["st"]
    rng = np.random.default_rng(2323)
    assert len(DEGREES) == N
    indeg = np.zeros(N, np.int64)
    indeg[rng.permutation(N)] = DEGREES                        # length and row id are unrelated
    dst = np.repeat(np.arange(N), indeg)
    # out-degrees: 21 nodes run 0..20, the others share the rest evenly
    order = rng.permutation(N)
    outdeg = np.zeros(N, np.int64)
    outdeg[order[:len(OUT_LADDER)]] = OUT_LADDER
    rest, others = N_EDGES - sum(OUT_LADDER), order[len(OUT_LADDER):]
    outdeg[others] = rest // len(others)
    outdeg[others[:rest % len(others)]] += 1
    src = rng.permutation(np.repeat(np.arange(N), outdeg))
    # edge ids: a permutation that keeps the order inside a row (csr_build orders a row by edge id)
    ids = rng.permutation(N_EDGES)
    for r in range(N):
        m = dst == r
        ids[m] = np.sort(ids[m])
    u, v = np.empty(N_EDGES, np.int64), np.empty(N_EDGES, np.int64)
    u[ids], v[ids] = dst, src
    indptr, indices, eid, _, _ = O.csr_build(u, v, N, N)       # rows = table rows (sources), columns = destinations
    st = Structure()
    st.og = O.CsrGraph(indptr, indices, eid=eid, n_src=N)
    st.ogt = st.og.transpose()
    st.ogf = O.CsrGraph(st.ogt.indptr, st.ogt.indices, eid=st.ogt.eid, n_src=N)
    st.ogs = st.ogf.transpose()            # og's rows with nidx = the positions of ogf: what the backward of a launch on ogf walks
    assert np.array_equal(st.ogs.indptr, st.og.indptr) and np.array_equal(st.ogs.eid, st.og.eid)
    st.indeg = np.diff(st.ogt.indptr)
    st.outdeg = np.diff(st.og.indptr)
    st.row_of_pos = st.ogt.dst_of_pos
    st.len_of_eid = np.empty(N_EDGES, np.int64)                # the length of the destination row an edge id lies in
    st.len_of_eid[st.ogt.eid] = st.indeg[st.row_of_pos]
    st.coo_src, st.coo_dst = v, u                              # by edge id: what stag_amd.Graph is built from
    _CACHE["st"] = st
    return st


def check_structure(st):
    g = st.ogt
    assert g.n_dst == g.n_src == N and g.n_edges == N_EDGES and 1600 <= N_EDGES <= 1800
    assert sorted(st.indeg) == sorted(DEGREES)
    for d in LADDER + CUT64 + CUT4:
        assert (st.indeg == d).sum() == 1 + FILL.count(d), d
    assert set(FILL) == {1, 2, 3} and len(FILL) == N - 50
    lad = np.array([int(np.flatnonzero(st.indeg == d)[0]) for d in range(4, 41)])
    assert not np.all(np.diff(lad) > 0), "length and row id are unrelated"
    assert sorted(g.eid) == sorted(g.nidx) == list(range(N_EDGES))
    assert list(g.eid) != list(range(N_EDGES)) and list(g.nidx) != list(range(N_EDGES)) and list(g.eid) != list(g.nidx)
    for r in range(N):
        assert np.all(np.diff(g.eid[g.indptr[r]:g.indptr[r + 1]]) > 0), "edge ids keep the order inside a row"
    assert np.array_equal(st.ogf.indptr, g.indptr) and np.array_equal(st.ogf.indices, g.indices) and st.ogf.nidx is None
    assert np.array_equal(st.ogf.eid, g.eid)
    # the out-degree ladder, and repeats inside a row
    assert set(OUT_LADDER) <= set(st.outdeg.tolist()) and st.outdeg.sum() == N_EDGES
    assert st.outdeg.max() > HEAVY_LEN, "the transposed CSR has heavy rows too"
    rep = sum(1 for r in range(N) if len(set(g.indices[g.indptr[r]:g.indptr[r + 1]])) < st.indeg[r])
    assert rep >= 10, "rows gather a source more than once"
    assert np.array_equal(np.bincount(st.coo_dst, minlength=N), st.indeg)
    assert np.array_equal(np.bincount(st.coo_src, minlength=N), st.outdeg)


# ---- plans and batches (the host planner: no GPU call) ----------------------------------------------------------------------
host_plan = vc.host_plan


def balanced(length, seg_len):
    """the segment lengths the planner cuts a row of `length` into: ceil(length / seg_len) segments, the longer ones first"""
    k = -(-length // seg_len)
    return [length // k + (1 if i < length % k else 0) for i in range(k)]


def check_plan(st, seg_len, n_units, n_long, n_seg, n_heavy, segs=None, units=None):
    """What the two segment lengths were chosen for (counts: of the host planner or of a view's plan)."""
    deg = st.indeg
    row = lambda d: int(np.flatnonzero(deg == d)[0])
    assert n_long == (deg > seg_len).sum() and n_seg == sum(len(balanced(int(d), seg_len)) for d in deg if d > seg_len)
    assert n_units == n_seg + (deg <= seg_len).sum(), "every row that is not cut is one unit, the empty row too"
    assert n_heavy == n_seg + ((deg <= seg_len) & (deg > HEAVY_LEN)).sum()
    if seg_len == 64:
        assert n_long == 7 and n_heavy - n_seg == 24 + 2, "17..40, 63 and 64 are heavy whole rows"
        want = {65: 2, 68: 2, 69: 2, 127: 2, 128: 2, 129: 3, 132: 3}
    else:
        assert seg_len == 4 and n_heavy == n_seg, "no whole-row unit is longer than 16"
        want = {64: COMBINE_GROUP, 68: 17, 69: 18, 132: 33, 5: 2, 16: 4, 17: 5}
    if segs is not None:
        for d, k in want.items():
            assert segs[row(d)] == k, (seg_len, d, segs[row(d)])
        assert row(seg_len) not in segs and segs[row(seg_len + 1)] == 2
    if units is not None:
        units = np.asarray(units).reshape(-1, 4)
        assert (units[:n_seg, 3] == np.arange(n_seg)).all() and (units[n_seg:, 3] < 0).all()
        whole = units[n_seg:]
        assert (np.diff(whole[:, 2]) <= 0).all() and whole[-1, 2] == 0, "whole rows longest first, the empty row last"
        assert sorted(whole[:, 2].tolist()) == sorted(int(d) for d in deg if d <= seg_len)
        # the light | heavy boundary lies between the rows of 17 and 16 edges
        h = n_heavy - n_seg
        if seg_len == 64:
            assert whole[h - 1, 2] == HEAVY_LEN + 1 and whole[h, 2] == HEAVY_LEN
            assert whole[h - 1, 0] == row(17) and whole[h, 0] == row(16)
        # the segments of a long row are balanced, in order, and tile it
        by_row = {}
        for r_, start, ln, slot in units[:n_seg]:
            by_row.setdefault(int(segs_row(st, segs, slot)), []).append((int(start), int(ln)))
        for r_, parts in by_row.items():
            assert [ln for _, ln in parts] == balanced(int(deg[r_]), seg_len), (seg_len, int(deg[r_]), parts)
            assert parts[0][0] == st.ogt.indptr[r_] and all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:]))
        if seg_len == 64:
            assert [ln for _, ln in by_row[row(65)]] == [33, 32]


def segs_row(st, segs, slot):
    """the destination row that owns segment `slot`: long rows in the order the planner lists them"""
    at = 0
    for r, k in segs.items():
        if slot < at + k:
            return r
        at += k
    raise AssertionError(slot)


def host_blocks(units):
    """block_ptr of stag_plan_blocks (256 edges / 32 units) over host unit records"""
    import ctypes as C
    from stag_amd import _lib
    lib = _lib.lib()
    units = np.ascontiguousarray(units, np.int32)
    nb = C.c_int32(0)
    args = (units.ctypes.data, len(units), BLOCK_EDGES, BLOCK_UNITS)
    _lib.check(lib.stag_plan_blocks(*args, None, C.byref(nb)), "stag_plan_blocks")
    ptr = np.zeros(nb.value + 1, np.int32)
    _lib.check(lib.stag_plan_blocks(*args, ptr.ctypes.data, C.byref(nb)), "stag_plan_blocks")
    return ptr


def batch_facts(units, ptr):
    """per batch: (units, edges, why it closed: "units" | "edges" | "end")"""
    lens = np.asarray(units).reshape(-1, 4)[:, 2]
    out = []
    for b in range(len(ptr) - 1):
        a, e = int(ptr[b]), int(ptr[b + 1])
        edges = int(lens[a:e].sum())
        why = "end" if e == len(lens) else "units" if e - a == BLOCK_UNITS else "edges"
        if why == "edges":
            assert edges + lens[e] > BLOCK_EDGES
        out.append((e - a, edges, why, int(lens[e - 1])))
    return out


def check_batches(facts_by_seg):
    """The four kinds of batch the cooperative GAT kernels must meet, over both segment lengths."""
    every = [f for facts in facts_by_seg.values() for f in facts]
    assert all(0 < n <= BLOCK_UNITS and e <= BLOCK_EDGES for n, e, _, _ in every)
    assert any(n == BLOCK_UNITS and why == "units" for n, _, why, _ in every), "a batch closed by the unit cap"
    assert any(n < BLOCK_UNITS and why == "edges" for n, _, why, _ in every), "a batch closed by the edge cap"
    assert any(n == 1 for n, _, _, _ in every), "a batch of a single unit"
    assert any(last == 0 for _, _, _, last in every), "a batch whose last unit has no edge"
    # (units come longest first and a batch closes only on a cap, so the single unit is a plan's last one: the empty row
    # alone at seg_len 4; at seg_len 64 the same row ends a batch behind other units)
    assert any(n > 1 and last == 0 for n, _, _, last in every), "... behind other units of the same batch"


# ---- tables ------------------------------------------------------------------------------------------------------------
class Tables:
    """The inputs of one width.  exact = True: small integers and power-of-two scales; else N(0, 1) rows and parameters from
    the middle of their ranges.  x: the gathered table (g for the backward entry points), own: the rows the units own."""

    def __init__(self, D, exact):
        rng = np.random.default_rng((5000 if exact else 1000) + D)
        f, E = np.float32, N_EDGES
        self.D, self.exact = D, exact
        if exact:
            self.x = rng.integers(-8, 9, (N, D)).astype(f)
            self.own = rng.integers(-8, 9, (N, D)).astype(f)
            self.ss = rng.choice([0.5, 1.0, 2.0], N).astype(f)
            self.ds = rng.choice([0.5, 1.0, 2.0], N).astype(f)
            self.w = rng.integers(-4, 5, (E, D)).astype(f)
            self.w1 = rng.integers(-4, 5, (E, 1)).astype(f)
            return
        self.x = rng.standard_normal((N, D)).astype(f)
        self.own = rng.standard_normal((N, D)).astype(f)
        self.ss = rng.uniform(0.5, 1.5, N).astype(f)
        self.ds = rng.uniform(0.5, 1.5, N).astype(f)
        self.w = rng.standard_normal((E, D)).astype(f)
        self.e0, self.e1log = rng.uniform(0.2, 1.2, (E, 1)).astype(f), rng.uniform(-1.0, 0.0, (E, 1)).astype(f)
        self.q0, self.q1 = rng.uniform(0.2, 1.2, (E, D)).astype(f), rng.uniform(0.3, 0.9, (E, D)).astype(f)
        self.c0, self.c1 = rng.uniform(0.2, 1.0, D).astype(f), rng.uniform(0.3, 0.9, D).astype(f)
        self.gmc = rng.standard_normal((MCB_S, N, D)).astype(f)           # the gradients of stag_agg_bwd_w_mc's samples

    def with_x(self, x):
        import copy
        t = copy.copy(self)
        t.x = np.ascontiguousarray(x, np.float32)
        return t


def tables(D, exact):
    if ("T", D, exact) not in _CACHE:
        _CACHE[("T", D, exact)] = Tables(D, exact)
    return _CACHE[("T", D, exact)]


class Spec(vc.Spec):
    """value_range_cases.Spec on this graph's edges"""

    def o(self, O, D, deriv=0, offset=OFFSET, in_norm=None):
        in_norm = self.in_norm if in_norm is None else in_norm
        if self.kind in ("none", "explicit"):
            return O.make_spec(self.kind, self.p0, relu=self.relu, in_norm=in_norm)
        return O.make_spec(self.kind, self.p0, self.p1, Dn=self.dn or D, n_edges=N_EDGES, deriv=deriv, offset=offset,
                           seed=SEED, relu=self.relu, in_norm=in_norm, p1_log=self.p1_log)


Case = vc.Case            # entry, spec, reduce, ss, ds, view, want_dp, plain: as in tests/value_range_cases.py


def _plain(name, spec, **kw):
    return Case(name + " (plain launch)", "fwd", spec, ss=False, view="f", plain=True, **kw)


def cases_exact(D):
    """Every case whose device result must equal the float64 reference bit for bit (reference(): the oracle)."""
    T, S = tables(D, True), Spec
    return [
        Case("stag_agg_fwd none", "fwd", S("none")),
        Case("stag_agg_fwd none, no nidx", "fwd", S("none"), view="f"),
        Case("stag_agg_fwd explicit [E,D]", "fwd", S("explicit", T.w)),
        Case("stag_agg_fwd Bernoulli(0.5)", "fwd", S("bernoulli", 0.5)),
        _plain("stag_agg_fwd Bernoulli(0.5)", S("bernoulli", 0.5)),
        Case("stag_agg_fwd_mc Bernoulli(0.5)", "mc", S("bernoulli", 0.5)),
        Case("stag_agg_fwd_w1 explicit [E,1]", "w1", S("explicit", T.w1, dn=1)),
        Case("stag_agg_fwd_w1 Bernoulli(0.5)", "w1", S("bernoulli", 0.5, dn=1)),
        Case("stag_agg_bwd none", "bwd", S("none")),
        Case("stag_agg_bwd explicit", "bwd", S("explicit", T.w)),
        Case("stag_agg_bwd Bernoulli(0.5)", "bwd", S("bernoulli", 0.5)),
        Case("stag_agg_max_fwd none", "max", S("none"), ss=False, ds=False),
        Case("stag_agg_max_fwd explicit", "max", S("explicit", T.w), ss=False, ds=False),
        Case("stag_agg_max_fwd Bernoulli(0.5)", "max", S("bernoulli", 0.5), ss=False, ds=False),
    ]


def cases_exact_half(D):
    S = Spec
    return [Case("stag_agg_fwd_half none", "half", S("none")),
            Case("stag_agg_fwd_half Bernoulli(0.5)", "half", S("bernoulli", 0.5))]


def cases_tol(D):
    """Everything that draws Normal or Uniform weights, divides or exponentiates: at util.TOL."""
    T, S = tables(D, False), Spec
    out = [
        Case("stag_agg_fwd scalar Normal relu", "fwd", S("normal", 1.0, 0.5, relu=True)),
        Case("stag_agg_fwd per-channel Normal relu", "fwd", S("normal", T.c0, T.c1, relu=True)),
        Case("stag_agg_fwd scalar Uniform in-norm", "fwd", S("uniform", 0.5, 1.5, in_norm=True)),
        Case("stag_agg_fwd scalar Bernoulli in-norm", "fwd", S("bernoulli", 0.6, in_norm=True)),
        Case("stag_agg_fwd [E,1] Normal p1_log", "fwd", S("normal", T.e0, T.e1log, p1_log=True)),
        Case("stag_agg_fwd [E,D] Normal", "fwd", S("normal", T.q0, T.q1)),
        Case("stag_agg_fwd none mean", "fwd", S("none"), reduce="mean"),
        Case("stag_agg_fwd explicit mean", "fwd", S("explicit", T.w), reduce="mean"),
        _plain("stag_agg_fwd scalar Normal relu", S("normal", 1.0, 0.5, relu=True)),
        _plain("stag_agg_fwd scalar Uniform mean", S("uniform", 0.2, 1.8), reduce="mean"),
        Case("stag_agg_fwd_mc scalar Normal", "mc", S("normal", 1.0, 0.5)),
        Case("stag_agg_fwd_mc per-channel Uniform in-norm", "mc", S("uniform", T.c0, T.c0 + T.c1, in_norm=True)),
        Case("stag_agg_fwd_w1 scalar Normal", "w1", S("normal", 1.0, 0.5, dn=1)),
        Case("stag_agg_fwd_mc_edge Normal p1_log", "mc_edge", S("normal", T.e0, T.e1log, p1_log=True)),
        Case("stag_agg_fwd_mc_pedge Normal", "mc_pedge", S("normal", T.q0, T.q1)),
        Case("stag_agg_bwd per-channel Normal relu, derivatives", "bwd", S("normal", T.c0, T.c1, relu=True), want_dp=True),
        Case("stag_agg_bwd scalar Uniform, derivatives", "bwd", S("uniform", 0.2, 1.8), want_dp=True),
        Case("stag_agg_bwd_dp per-channel Normal relu", "bwd_dp", S("normal", T.c0, T.c1, relu=True)),
        Case("stag_agg_max_fwd scalar Normal", "max", S("normal", 1.0, 0.5), ss=False, ds=False),
    ]
    if D <= 256:          # (one channel tile)
        out.append(Case("stag_agg_bwd_edge Normal p1_log", "bwd_edge", S("normal", T.e0, T.e1log, p1_log=True)))
    return out


def cases_tol_half(D):
    S = Spec
    return [Case("stag_agg_fwd_half scalar Normal", "half", S("normal", 1.0, 0.5)),
            Case("stag_agg_fwd_half scalar Normal mean", "half", S("normal", 1.0, 0.5), reduce="mean")]


def half_table(T, dtype):
    """(the rows in the half type on the CPU, the same numbers as float32); the exact tables are exact in both types"""
    import torch
    xh = torch.from_numpy(T.x).to(getattr(torch, dtype))
    xf = xh.float().numpy()
    if T.exact:
        assert np.array_equal(xf, T.x)
    return xh, xf


# ---- references --------------------------------------------------------------------------------------------------------
reference = vc.reference          # the oracle's outputs of a case, in the order the launch returns them
numpy_agg, numpy_max, graph_of, weights = vc.numpy_agg, vc.numpy_max, vc.graph_of, vc.weights


def numpy_reference(O, st, case, T):
    """reference() of an exact case again: a float64 loop over the edges on the oracle's materialised weights."""
    g, D = graph_of(st, case), T.D
    W = lambda offset=OFFSET: weights(O, st, case, D, 0, offset)
    if case.entry == "max":
        return [numpy_max(g, T.x, W()).astype(np.float64)]
    ss, ds = (T.ss if case.ss else None), (T.ds if case.ds else None)
    if case.entry == "mc":
        return [np.stack([numpy_agg(g, T.x, W(OFFSET + s * MC_STRIDE), ss, ds) for s in range(MC_S)], 0)]
    assert case.entry in ("fwd", "w1", "half", "bwd") and case.reduce == "sum" and not case.want_dp
    return [numpy_agg(g, T.x, W(), ss, ds)]


def abs_terms(O, st, case, T):
    """sum |terms| of every sum of an exact case (the exactness bound)"""
    g, D = graph_of(st, case), T.D
    offs = [OFFSET + s * MC_STRIDE for s in range(MC_S)] if case.entry == "mc" else [OFFSET]
    return max(float(numpy_agg(g, np.abs(T.x), np.abs(weights(O, st, case, D, 0, o)), T.ss if case.ss else None,
                               T.ds if case.ds else None).max()) for o in offs)


def f32_agg(g, x, W, ss=None, ds=None, mean=False):
    """numpy_agg in float32, every term rounded and added in edge order: what a kernel without compensation computes"""
    f = np.float32
    out = np.zeros((g.n_dst, x.shape[1]), f)
    for v in range(g.n_dst):
        acc = np.zeros(x.shape[1], f)
        for p in range(g.indptr[v], g.indptr[v + 1]):
            u = g.indices[p]
            acc = acc + W[g.eid[p]] * (x[u] * (f(1.0) if ss is None else ss[u]))
        sc = (f(1.0) if ds is None else ds[v]) / (f(max(g.indptr[v + 1] - g.indptr[v], 1)) if mean else f(1.0))
        out[v] = acc * sc
    return out


def f32_reference(O, st, case, T):
    """The first output of a TOL case restated in float32 (in-norm comes inside the oracle's materialised weights)."""
    g, D = graph_of(st, case), T.D
    ss, ds = (T.ss if case.ss else None), (T.ds if case.ds else None)
    offs = vc._offsets(case)
    W = lambda offset=OFFSET: weights(O, st, case, D, 0, offset)
    if case.entry == "max":
        return numpy_max(g, T.x, W())
    if offs:
        return np.stack([f32_agg(g, T.x, W(o), ss, ds, case.reduce == "mean") for o in offs], 0)
    return f32_agg(g, T.x, W(), ss, ds, case.reduce == "mean")


# ---- stag_agg_max_bwd, stag_agg_bwd_w, stag_segment_reduce on exact data -------------------------------------------------------
def max_case(O, st, D, kind):
    """stag_agg_max_fwd / _bwd on the exact tables: (W [E, D] by edge id or None, out, cnt, g, dx, dw).  g = cnt x (an integer in
    [-4, 4]), so the equal shares g / cnt are integers and dx, a sum over a source's out-edges, is exact.  The backward
    walks the transposed CSR: its rows run over the out-degrees."""
    T, g = tables(D, True), st.ogt
    rng = np.random.default_rng(77 + D)
    W = T.w if kind == "explicit" else None
    m = (T.x[g.indices] if W is None else W[g.eid] * T.x[g.indices]).astype(np.float64)         # [positions, D]
    rows = st.row_of_pos
    out = np.zeros((N, D), np.float64)
    cnt = np.zeros((N, D), np.int32)
    for v in range(N):
        sel = m[rows == v]
        if len(sel):
            out[v] = sel.max(0)
            cnt[v] = (sel == out[v]).sum(0)
    share = rng.integers(-4, 5, (N, D)).astype(np.float64)
    gout = share * cnt
    hit = (m == out[rows]) * share[rows]                                                         # what each edge sends back
    dx = np.zeros((N, D), np.float64)
    np.add.at(dx, g.indices, hit if W is None else hit * W[g.eid])
    dw = np.zeros((N_EDGES, D), np.float64)
    dw[g.eid] = hit * T.x[g.indices]
    return W, out, cnt, gout.astype(np.float32), dx, dw


def bwd_w_exact(st, T):
    """stag_agg_bwd_w without a spec on the exact tables: dw[eid, k] = ss[u] x[u, k] g[v, k], g = T.own"""
    g = st.ogt
    dw = np.zeros((N_EDGES, T.D), np.float64)
    dw[g.eid] = (T.ss[g.indices, None].astype(np.float64) * T.x[g.indices]) * T.own[st.row_of_pos]
    return dw


def segment_table(D):
    rng = np.random.default_rng(900 + D)
    return rng.integers(-8, 9, (N_EDGES, D)).astype(np.float32)


def segment_sums(st, xe):
    out = np.zeros((N, xe.shape[1]), np.float64)
    np.add.at(out, st.row_of_pos, xe.astype(np.float64))
    return out


# ---- stag_agg_bwd_w / stag_agg_bwd_w_mc on a Normal spec -------------------------------------------------------------------
def bwd_w_spec(D):
    T = tables(D, False)
    return Spec("normal", T.q0, T.q1)


def bwd_w_reference(O, st, T, n_samples, stride, gs):
    """(d p0, d p1) [E, D] in float64: oracle.agg_bwd_w per sample and derivative on the view every launch walks, summed over
    the samples.  g of sample s: T.gmc[s] (times g_scale)."""
    sp, D = bwd_w_spec(T.D), T.D
    refs = []
    for dv in (1, 2):
        tot = np.zeros((N_EDGES, D), np.float64)
        for s in range(n_samples):
            gg = T.gmc[s] if gs is None else T.gmc[s] * gs[:, None]
            tot += O.agg_bwd_w(st.ogt, T.x, gg, src_scale=T.ss, spec=sp.o(O, D, deriv=dv, offset=OFFSET + s * stride)).astype(np.float64)
        refs.append(tot)
    return refs


# ---- stag_agg_bwd_pedge over the source-major view (the out-degree ladder and, at seg_len 4, its cut rows) ---------------------
PEDGE_WIDTHS = (3, 16, 64, 260)


def pedge_specs(D):
    """(exact, tol): Normal(integer loc, 0) — w == loc and d/dloc == 1 exactly — on the exact tables; Normal [E, D] tables
    with log-scales on the N(0, 1) tables"""
    Te, Tt = tables(D, True), tables(D, False)
    return (Spec("normal", Te.w, np.zeros_like(Te.w)),
            Spec("normal", Tt.q0, np.log(Tt.q1).astype(np.float32), p1_log=True))


def pedge_reference(O, st, T, spec, f32=False):
    """(dx [N, D] over the sources, dp0, dp1 [E, D] by edge id, sum |terms| of dx) in float64.  On ogs rows are sources u, the
    columns destinations v, nidx the positions of ogf (the draw), eid the edge ids: T.own holds the rows the units own
    (row_scale = T.ds), T.x the gathered table (g_scale = T.ss):
        dx[u] = ds[u] sum_p w[p] (ss[v] x[v]),  dp_i[eid_p] = D_i[p] (ds[u] own[u]) (ss[v] x[v]).
    f32: dx again with every term rounded to fp32 and added in edge order."""
    s, D = st.ogs, T.D
    rows, cols, eid = s.dst_of_pos, s.indices, s.eid
    case = Case("weights", "fwd", spec, view="f")
    W, D1, D2 = (weights(O, st, case, D, deriv=d) for d in (0, 1, 2))
    ft = np.float32 if f32 else np.float64
    gg = (T.ss[cols, None].astype(ft) * T.x[cols].astype(ft)).astype(ft)
    xx = (T.ds[rows, None].astype(ft) * T.own[rows].astype(ft)).astype(ft)
    dx, ab = np.zeros((N, D), ft), np.zeros((N, D), np.float64)
    for p in range(N_EDGES):                                   # in edge order
        dx[rows[p]] = dx[rows[p]] + (W[eid[p]].astype(ft) * gg[p]).astype(ft)
        ab[rows[p]] += np.abs(W[eid[p]].astype(np.float64) * gg[p])
    dx = (dx * T.ds[:, None].astype(ft)).astype(ft)
    ab *= T.ds[:, None]
    val = (xx * gg).astype(ft)
    dp0, dp1 = np.zeros((N_EDGES, D), ft), np.zeros((N_EDGES, D), ft)
    dp0[eid], dp1[eid] = (D1[eid].astype(ft) * val).astype(ft), (D2[eid].astype(ft) * val).astype(ft)
    return dx, dp0, dp1, ab


def source_row_class(st, seg_len):
    """per source row of ogs: 2 = cut into segments (long), 1 = a whole-row unit of more than 16 edges (Kahan), 0 = plain"""
    deg = st.outdeg
    long_row = (deg > seg_len) if seg_len else np.zeros(N, bool)
    return np.where(long_row, 2, np.where(deg > HEAVY_LEN, 1, 0))


# ---- GAT ---------------------------------------------------------------------------------------------------------------------
def gat_inputs(H, F):
    """el, er [N, H], ft, G [N, H, F] N(0, 1), w [E, H] explicit weights by edge id"""
    if ("gat", H, F) not in _CACHE:
        rng = np.random.default_rng(100 * H + F)
        f = np.float32
        _CACHE[("gat", H, F)] = dict(el=rng.standard_normal((N, H)).astype(f), er=rng.standard_normal((N, H)).astype(f),
                                     ft=rng.standard_normal((N, H, F)).astype(f), G=rng.standard_normal((N, H, F)).astype(f),
                                     w=rng.uniform(0.5, 1.5, (N_EDGES, H)).astype(f))
    return _CACHE[("gat", H, F)]


GAT_WEIGHTINGS = ("none", "explicit", "normal")


def gat_spec(O, name, H, w=None, offset=None):
    if name == "none":
        return O.make_spec("none")
    if name == "explicit":
        return O.make_spec("explicit", w)
    return O.make_spec("normal", 1.0, 0.5, Dn=H, n_edges=N_EDGES, seed=GAT_NOISE["seed"],
                       offset=GAT_NOISE["offset"] if offset is None else offset)


def gat_f32(g, el, er, ft, slope, W=None):
    """oracle.gat_fwd restated in float32 numpy: (out, attn by edge id), the softmax shifted by the row maximum"""
    f = np.float32
    H, F = ft.shape[1], ft.shape[2]
    out, attn = np.zeros((g.n_dst, H, F), f), np.zeros((g.n_edges, H), f)
    for v in range(g.n_dst):
        p = np.arange(g.indptr[v], g.indptr[v + 1])
        if not len(p):
            continue
        u = g.indices[p]
        s = el[u] + er[v]
        lr = np.where(s > 0, s, f(slope) * s)
        logit = lr if W is None else W[g.eid[p]] * lr
        ex = np.exp(logit - logit.max(0))
        a = (ex / ex.sum(0, dtype=f)).astype(f)
        attn[g.eid[p]] = a
        out[v] = (a[:, :, None] * ft[u]).sum(0, dtype=f)
    return out, attn


# ---- the wide edge embedding: stag_edge_embed_bwd over the ladder, stag_edge_embed_fwd over its tails -----------------------
EMBED_WIDTHS = (3, 16, 64, 256, 260)
EMBED_OWN, EMBED_OTHER = (0.0, 64.0), (0.0, 64.0, -256.0)
EMBED_CLASS = {0.0: (0.0, 0.5), 64.0: (64.0, 1.0), 128.0: (128.0, 1.0), -256.0: (-0.0, 0.0), -192.0: (-0.0, 0.0)}   # pre: (SiLU, SiLU')
EMBED_ORIENT = {"d pd": ("f", "rows"), "d ps": ("s", "src")}      # the view each orientation walks, and what its rows are
EMBED_FWD_WIDTHS = {16: 4, 256: 64, 5: 4, 260: 64}                # hidden: lanes per edge (T = 256 / lanes teams per block)
EMBED_FWD_NODES = 37


def embed_view(st, orient):
    return st.ogf if EMBED_ORIENT[orient][0] == "f" else st.ogs


def embed_tables(hidden, exact, orient):
    """own [N, hidden] (the rows the units own: pd for d pd, ps for d ps), other [N, hidden] (the gathered table), g [E, hidden]
    by edge id.  exact: own in {0, 64}, other in {0, 64, -256} (one in five: most terms count), g nonzero integers in [-8, 8]."""
    key = ("embed", hidden, exact, orient)
    if key not in _CACHE:
        rng = np.random.default_rng((9000 if exact else 8000) + hidden + (500 if orient == "d ps" else 0))
        f = np.float32
        if exact:
            own = rng.choice(EMBED_OWN, (N, hidden)).astype(f)
            other = rng.choice(EMBED_OTHER, (N, hidden), p=(0.4, 0.4, 0.2)).astype(f)
            g = (rng.integers(1, 9, (N_EDGES, hidden)) * rng.choice([-1, 1], (N_EDGES, hidden))).astype(f)
        else:
            own, other = rng.standard_normal((N, hidden)).astype(f), rng.standard_normal((N, hidden)).astype(f)
            g = rng.standard_normal((N_EDGES, hidden)).astype(f)
        _CACHE[key] = (own, other, g)
    return _CACHE[key]


def embed_bwd_reference(view, own, other, g, exact=False):
    """(d_own [rows, hidden], sum |terms|) in float64: sum over a row's positions of g[eid] SiLU'(own[row] + other[column]),
    the pre-activation rounded to fp32 first.  exact: float64 SiLU' rounded to fp32 (the class table: SiLU'(-256) is -1e-109
    before that rounding), so that the sums are those of fp32 numbers."""
    import edge_embed_range_cases as ec
    rows = view.dst_of_pos
    pre = (own[rows] + other[view.indices]).astype(np.float32)
    dh = ec.silu64(pre.astype(np.float64))[1]
    term = g[view.eid].astype(np.float64) * (dh.astype(np.float32).astype(np.float64) if exact else dh)
    out, ab = np.zeros((view.n_dst, own.shape[1])), np.zeros((view.n_dst, own.shape[1]))
    np.add.at(out, rows, term)
    np.add.at(ab, rows, np.abs(term))
    return out, ab


def embed_fwd_sizes(lanes):
    T = 256 // lanes
    return sorted({1, T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1})


def embed_fwd_case(hidden, E):
    """src, dst [E] int32 over EMBED_FWD_NODES nodes, ps in {0, 64}, pd in {0, 64, -256}: SiLU is exact in fp32"""
    rng = np.random.default_rng(100 * hidden + E)
    f, n = np.float32, EMBED_FWD_NODES
    return (rng.integers(0, n, E).astype(np.int32), rng.integers(0, n, E).astype(np.int32),
            rng.choice(EMBED_OWN, (n, hidden)).astype(f), rng.choice(EMBED_OTHER, (n, hidden)).astype(f))
