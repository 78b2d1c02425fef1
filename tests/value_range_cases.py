"""The fixture graph, the tables and the case lists of the value-range tests (no tests in here):
tests/test_value_range_host.py puts all of it through the oracle and a float64 numpy loop, tests/test_gpu_value_range.py
through the kernels.  Both import this module, so a case cannot mean one thing on the host and another on the device.

THE GRAPH: 48 nodes, 304 edges.  Destination rows 0..4 have in-degree 90, 40, 20, 3 and 1, rows 5..46 share 150 random
edges, row 47 has none.  One view serves every entry point: `ogt` (rows = the 48 destinations, columns = the 48 rows of the
gathered table, eid a permutation, nidx = the positions of its transpose `og`, another permutation: what a backward launch
is handed) and `ogf`, the same rows without nidx (the CSR's own positions as noise indices: what the plain forward launch
needs).  Source row U feeds the hub, the 40-, 20- and 3-edge rows and some ordinary rows, never inside the last 8 edges of a
row of more than 16 (so that a Kahan unit never ends on it: see group C), and not the 1-edge row.

A CASE names an entry point, a noise description and the launch options; `reference` gives the oracle's outputs for it,
`numpy_reference` the same numbers from a float64 loop over the edges on the oracle's materialised weights.

The second half of the file ("The per-edge gradient entry points ...") holds the fixtures of
tests/test_gpu_value_range_grad.py: GradTables, GradCase and the float64 statements grad_reference, max_fwd_reference and
max_bwd_reference, the bars of its group B and the poison sets of its group C."""
import numpy as np

N = 48
DEG_HEAD = (90, 40, 20, 3, 1)              # rows 0..4: the hub, two rows longer than 16, a row of three, a row of one
HUB, ROW40, ROW20, ROW3, ROW1 = range(5)
N_RANDOM = 150                             # edges into rows 5..46; row 47 has none
N_EDGES = sum(DEG_HEAD) + N_RANDOM
U = 7                                      # the source row group C poisons
SEGS = (4, 64)
WIDTHS = (6, 8, 264)                       # no vector path and a partial chunk | vectorised | two channel tiles
HALF_WIDTHS = (8, 264)
# The plain forward kernel exists at 32 and 64 lanes per row: D = 264 takes it with any plan, D = 128 without a plan
# (with this small plan 32 lanes take the two-slot general instantiation); D = 8 stays on the general kernel either way.
PLAIN_WIDTHS = (8, 128, 264)
PLAIN_SEGS = (4, 64, 0)
KAHAN_MIN_LEN = 16                         # STAG_KAHAN_MIN_LEN (csrc/agg_kernel.hpp)
SEED, OFFSET = 11, 2
MC_S, MC_STRIDE = 5, 3                     # stag_agg_fwd_mc: a pass of four samples and one of one (in-norm: 2, 2, 1)
MCE_S, MCE_STRIDE = 7, 2                   # stag_agg_fwd_mc_edge / _pedge: passes of 4, 2 and 1
SCALES = (2.0 ** -100, 2.0 ** -60, 2.0 ** 100)
FP16_SCALES = (2.0 ** -10, 2.0 ** 12)
POISON = {6: (1, 3, 4), 8: (1, 3, 4), 128: (1, 66, 124), 264: (1, 130, 260)}     # channels of row U: +inf, NaN, -inf
POISON_VALUES = (np.inf, np.nan, -np.inf)
TINY = 2.0 ** -149
LOG_SCALES = (16.0, -16.0)

_CACHE = {}


class Structure:
    pass


def structure(O):
    """The fixture graph as the oracle's CsrGraph objects (built once)."""
    if "st" in _CACHE:
        return _CACHE["st"]
    rng = np.random.default_rng(20240)
    dst = np.concatenate([np.repeat(np.arange(5), DEG_HEAD), np.sort(rng.integers(5, N - 1, N_RANDOM))])
    src = rng.integers(0, N, N_EDGES)
    src[src == U] = U + 1                                     # U feeds exactly the rows chosen here
    first = np.concatenate([[0], np.cumsum(DEG_HEAD)])
    src[first[HUB] + 30] = src[first[HUB] + 61] = U           # one edge in each segment of the hub at seg_len 64
    src[first[ROW40] + 12] = src[first[ROW20] + 7] = src[first[ROW3] + 1] = U
    ordinary = [int(np.flatnonzero(dst == r)[0]) for r in np.unique(dst[dst >= 5])[[0, 3, 9]]]
    src[ordinary] = U
    # edge ids: a permutation that keeps the order inside a row (csr_build orders a row by edge id)
    ids = rng.permutation(N_EDGES)
    for r in range(N):
        m = dst == r
        ids[m] = np.sort(ids[m])
    u, v = np.empty(N_EDGES, np.int64), np.empty(N_EDGES, np.int64)
    u[ids], v[ids] = dst, src
    indptr, indices, eid, _, _ = O.csr_build(u, v, N, N)      # rows = table rows, columns = destinations
    st = Structure()
    st.og = O.CsrGraph(indptr, indices, eid=eid, n_src=N)
    st.ogt = st.og.transpose()
    st.ogf = O.CsrGraph(st.ogt.indptr, st.ogt.indices, eid=st.ogt.eid, n_src=N)
    st.indeg = np.diff(st.ogt.indptr)
    st.row_of_pos = st.ogt.dst_of_pos
    st.pos_from_u = np.flatnonzero(st.ogt.indices == U)
    st.fed = np.unique(st.row_of_pos[st.pos_from_u])          # the rows with an in-edge from U
    st.eid_from_u = np.sort(st.ogt.eid[st.pos_from_u])
    _CACHE["st"] = st
    return st


def check_structure(st):
    g = st.ogt
    assert g.n_dst == g.n_src == N and g.n_edges == N_EDGES
    assert tuple(st.indeg[:5]) == DEG_HEAD and st.indeg[5:N - 1].sum() == N_RANDOM and st.indeg[N - 1] == 0
    assert st.indeg[5:].max() <= KAHAN_MIN_LEN, "the ordinary rows are plain sums at seg_len 64"
    assert st.indeg[5:].max() > 4, "and some of them are cut at seg_len 4"
    assert sorted(g.eid) == sorted(g.nidx) == list(range(N_EDGES))
    assert list(g.eid) != list(range(N_EDGES)) and list(g.nidx) != list(range(N_EDGES))
    assert np.array_equal(st.ogf.indptr, g.indptr) and np.array_equal(st.ogf.indices, g.indices) and st.ogf.nidx is None
    # what U feeds
    assert {HUB, ROW40, ROW20, ROW3} <= set(st.fed) and ROW1 not in st.fed and (st.fed >= 5).sum() >= 3
    assert len(st.fed) < N // 2, "most rows stay clean"
    for p in st.pos_from_u:
        r = st.row_of_pos[p]
        if st.indeg[r] > KAHAN_MIN_LEN:
            assert g.indptr[r + 1] - p > 8, "a Kahan unit never ends on the poisoned edge"
    hub_pos = st.pos_from_u[st.row_of_pos[st.pos_from_u] == HUB] - g.indptr[HUB]
    assert (hub_pos < 45).any() and (hub_pos >= 45).any(), "both segments of the hub at seg_len 64 gather U"


def host_plan(indptr, seg_len):
    """(n_units, n_long, n_seg, n_heavy, segments of each long row) from the host planner"""
    import ctypes as C
    from stag_amd import _lib
    lib = _lib.lib()
    indptr = np.ascontiguousarray(indptr, np.int32)
    n = len(indptr) - 1
    nu, nl, ns, nh = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(lib.stag_plan_count(indptr.ctypes.data, n, seg_len, C.byref(nu), C.byref(nl), C.byref(ns), C.byref(nh)), "count")
    units = np.zeros((max(nu.value, 1), 4), np.int32)
    long_rows, long_seg_ptr = np.zeros(max(nl.value, 1), np.int32), np.zeros(nl.value + 1, np.int32)
    _lib.check(lib.stag_plan_fill(indptr.ctypes.data, n, seg_len, units.ctypes.data, long_rows.ctypes.data,
                                  long_seg_ptr.ctypes.data), "fill")
    segs = dict(zip(long_rows[:nl.value].tolist(), np.diff(long_seg_ptr).tolist()))
    return dict(n_units=nu.value, n_long=nl.value, n_seg=ns.value, n_heavy=nh.value, segs=segs, units=units[:nu.value])


def check_plan(st, seg_len, n_units, n_long, n_seg, n_heavy, segs=None):
    """What the two segment lengths were chosen for (counts: of the host planner or of a view's plan)."""
    deg = st.indeg
    if seg_len == 4:
        assert n_long == (deg > 4).sum() and n_long >= 5
        assert n_heavy == n_seg, "no whole-row unit is longer than 16"
        if segs is not None:
            assert segs[HUB] == 23 and segs[HUB] > 16, "the hub is added group by group"
            assert segs[ROW40] == 10 and segs[ROW20] == 5 and ROW3 not in segs and ROW1 not in segs
    else:
        assert seg_len == 64 and n_long == 1 and n_seg == 2, "the hub is two segments"
        assert n_heavy == n_seg + 2, "the 40- and 20-edge rows are whole-row units longer than 16 (Kahan, heavy)"
        assert n_units == n_seg + (N - 1)
        if segs is not None:
            assert segs == {HUB: 2}


def row_class(st, seg_len):
    """per destination row: 2 = a long row (its segments' partials are Kahan-summed), 1 = a whole-row unit longer than 16
    (a Kahan sum), 0 = a plain sum.  seg_len 0: no plan, every row is a whole-row unit."""
    deg = st.indeg
    long_row = (deg > seg_len) if seg_len else np.zeros(N, bool)
    return np.where(long_row, 2, np.where(deg > KAHAN_MIN_LEN, 1, 0))


# ---- tables ------------------------------------------------------------------------------------------------------------
class Tables:
    """The inputs of one width: x (the gathered table: g for the backward entry points), own (the rows the units own),
    the two scales, and the weight / parameter tables by edge id."""

    def __init__(self, D):
        rng = np.random.default_rng(1000 + D)
        f = np.float32
        E = N_EDGES
        self.D = D
        self.x = rng.standard_normal((N, D)).astype(f)
        self.own = rng.standard_normal((N, D)).astype(f)
        self.ss = rng.uniform(0.5, 1.5, N).astype(f)
        self.ds = rng.uniform(0.5, 1.5, N).astype(f)
        self.w = rng.standard_normal((E, D)).astype(f)
        self.wpos = rng.uniform(0.5, 1.5, (E, D)).astype(f)
        self.w1 = rng.standard_normal((E, 1)).astype(f)
        self.w1pos = rng.uniform(0.5, 1.5, (E, 1)).astype(f)
        self.e0, self.e1log = rng.uniform(0.2, 1.2, (E, 1)).astype(f), rng.uniform(-1.0, 0.0, (E, 1)).astype(f)
        self.e1 = rng.uniform(0.3, 0.9, (E, 1)).astype(f)
        self.q0, self.q1 = rng.uniform(0.2, 1.2, (E, D)).astype(f), rng.uniform(0.3, 0.9, (E, D)).astype(f)
        self.c0, self.c1 = rng.uniform(0.2, 1.0, D).astype(f), rng.uniform(0.3, 0.9, D).astype(f)
        self.cb = rng.uniform(0.25, 0.75, D).astype(f)
        self.eb = rng.uniform(0.25, 0.75, (E, 1)).astype(f)
        self.qb = rng.uniform(0.25, 0.75, (E, D)).astype(f)
        self.x16 = (rng.uniform(0.25, 4.0, (N, D)) * rng.choice([-1.0, 1.0], (N, D))).astype(np.float16)

    def with_x(self, x):
        import copy
        t = copy.copy(self)
        t.x = np.ascontiguousarray(x, np.float32)
        return t


def tables(D):
    if ("T", D) not in _CACHE:
        _CACHE[("T", D)] = Tables(D)
    return _CACHE[("T", D)]


def poisoned(x, D):
    xp = np.array(x, np.float32)
    xp[U, list(POISON[D])] = POISON_VALUES
    return xp


def hit_mask(st, D):
    """H of group C as a [N, D] mask: rows with an in-edge from U x poisoned channels"""
    H = np.zeros((N, D), bool)
    H[np.ix_(st.fed, POISON[D])] = True
    return H


# ---- noise descriptions ----------------------------------------------------------------------------------------------
class Spec:
    """One noise description: .o(O, D) the oracle's spec, .c(dev) the library's stag_noise_spec (parameters on the device).
    p0 / p1: python floats, [Dn], [E, 1] or [E, Dn] float32 arrays (by edge id); dn: the width of the noise where it is not
    the launch's (stag_agg_fwd_w1: 1)."""

    def __init__(self, kind, p0=None, p1=None, relu=False, in_norm=False, p1_log=False, dn=None):
        self.kind, self.p0, self.p1, self.relu, self.in_norm, self.p1_log, self.dn = kind, p0, p1, relu, in_norm, p1_log, dn
        self._keep = {}

    def o(self, O, D, deriv=0, offset=OFFSET, in_norm=None):
        in_norm = self.in_norm if in_norm is None else in_norm
        if self.kind in ("none", "explicit"):
            return O.make_spec(self.kind, self.p0, relu=self.relu, in_norm=in_norm)
        return O.make_spec(self.kind, self.p0, self.p1, Dn=self.dn or D, n_edges=N_EDGES, deriv=deriv, offset=offset,
                           seed=SEED, relu=self.relu, in_norm=in_norm, p1_log=self.p1_log)

    def c(self, dev, deriv=0, in_norm=None):
        import torch
        from stag_amd import _lib
        mode = lambda p: (_lib.PARAM_SCALAR if not isinstance(p, np.ndarray) else _lib.PARAM_PER_CHANNEL if p.ndim == 1
                          else _lib.PARAM_PER_EDGE1 if p.shape[1] == 1 else _lib.PARAM_PER_EDGE)
        s = _lib.NoiseSpec()
        s.kind = {"none": _lib.NOISE_NONE, "explicit": _lib.NOISE_EXPLICIT, "normal": _lib.NOISE_NORMAL,
                  "uniform": _lib.NOISE_UNIFORM, "bernoulli": _lib.NOISE_BERNOULLI}[self.kind]
        if dev not in self._keep:
            self._keep[dev] = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) if isinstance(p, np.ndarray) else None
                               for p in (self.p0, self.p1)]
        keep = self._keep[dev]
        s.p0, s.p1 = _lib.ptr(keep[0]), _lib.ptr(keep[1])
        if s.kind >= _lib.NOISE_NORMAL:
            s.param_mode = max(mode(self.p0), mode(self.p1))
            if s.param_mode == _lib.PARAM_SCALAR:
                s.p0_scalar, s.p1_scalar = float(self.p0), float(0.0 if self.p1 is None else self.p1)
        s.relu, s.in_norm, s.p1_log = int(self.relu), int(self.in_norm if in_norm is None else in_norm), int(self.p1_log)
        s.deriv, s.seed, s.offset = deriv, SEED, OFFSET
        return s

    @property
    def has_derivs(self):
        return self.kind in ("normal", "uniform") and not self.in_norm


class Case:
    """entry: fwd | mc | half | w1 | mc_edge | mc_pedge | bwd | bwd_dp | bwd_edge | max.  view: "t" (ogt: eid and nidx
    permutations) | "f" (ogf: no nidx).  plain: the launch meets plain_launch_ok (scalar parameters, no src_scale, no
    in-norm, no nidx) — it is repeated with STAG_AGG_PLAIN=0.  norm: what every output is divided by before it meets
    the bar (the log-scale cases: e^{+-16})."""

    def __init__(self, name, entry, spec, reduce="sum", ss=True, ds=True, view="t", want_dp=False, plain=False, norm=1.0,
                 zero=False):
        self.name, self.entry, self.spec, self.reduce, self.ss, self.ds, self.view = name, entry, spec, reduce, ss, ds, view
        self.want_dp, self.plain, self.norm, self.zero = want_dp, plain, norm, zero
        if plain:
            assert entry == "fwd" and view == "f" and not ss and not spec.in_norm
            assert spec.kind in ("normal", "uniform", "bernoulli") and not isinstance(spec.p0, np.ndarray)
        if entry in ("bwd", "bwd_dp", "bwd_edge", "max"):
            assert reduce == "sum"

    def widths(self):
        if self.plain:
            return PLAIN_WIDTHS
        if self.entry == "half":
            return HALF_WIDTHS
        return tuple(D for D in WIDTHS if D <= 256) if self.entry == "bwd_edge" else WIDTHS      # (one channel tile)

    def segs(self):
        return PLAIN_SEGS if self.plain else SEGS

    def norms(self):
        """per output: dx and d/dlog_scale carry the scale, d/dloc does not"""
        return [self.norm, 1.0, self.norm] if self.entry == "bwd_edge" else [self.norm] * len(self.kinds())

    def kinds(self):
        """the kind of every output: rows [N, D] | mc [S, N, D] | chan [D] | edge [E, 1]"""
        return {"mc": ["mc"], "mc_edge": ["mc"], "mc_pedge": ["mc"], "bwd": ["rows"] * (3 if self.want_dp else 1),
                "bwd_dp": ["rows", "chan", "chan"], "bwd_edge": ["rows", "edge", "edge"]}.get(self.entry, ["rows"])


def _plain(name, spec, **kw):
    return Case(name + " (plain launch)", "fwd", spec, ss=False, view="f", plain=True, **kw)


def cases_A(D):
    """Group A: every entry point with every noise kind it takes; mean, both scales, in-norm for Uniform and Bernoulli."""
    T, S = tables(D), Spec
    one = np.array([0.6], np.float32)
    return [
        Case("stag_agg_fwd none", "fwd", S("none")),
        Case("stag_agg_fwd none mean", "fwd", S("none"), reduce="mean", ss=False),
        Case("stag_agg_fwd explicit [E,D]", "fwd", S("explicit", T.w)),
        Case("stag_agg_fwd scalar Normal relu", "fwd", S("normal", 1.0, 0.5, relu=True)),
        Case("stag_agg_fwd per-channel Normal mean", "fwd", S("normal", T.c0, T.c1), reduce="mean"),
        Case("stag_agg_fwd scalar Uniform in-norm", "fwd", S("uniform", 0.5, 1.5, in_norm=True)),
        Case("stag_agg_fwd scalar Bernoulli in-norm", "fwd", S("bernoulli", 0.6, in_norm=True)),
        Case("stag_agg_fwd per-channel Bernoulli", "fwd", S("bernoulli", T.cb)),
        Case("stag_agg_fwd [E,1] Normal p1_log", "fwd", S("normal", T.e0, T.e1log, p1_log=True)),
        Case("stag_agg_fwd [E,D] Normal", "fwd", S("normal", T.q0, T.q1)),
        Case("stag_agg_fwd [E,D] Uniform in-norm mean", "fwd", S("uniform", T.q0, T.q0 + T.q1, in_norm=True), reduce="mean"),
        Case("stag_agg_fwd [E,1] Bernoulli", "fwd", S("bernoulli", T.eb)),
        _plain("stag_agg_fwd scalar Normal relu", S("normal", 1.0, 0.5, relu=True)),
        _plain("stag_agg_fwd scalar Uniform mean", S("uniform", 0.2, 1.8), reduce="mean"),
        _plain("stag_agg_fwd scalar Bernoulli", S("bernoulli", 0.6)),
        Case("stag_agg_fwd_mc scalar Normal", "mc", S("normal", 1.0, 0.5)),
        Case("stag_agg_fwd_mc per-channel Uniform in-norm", "mc", S("uniform", T.c0, T.c0 + T.c1, in_norm=True)),
        Case("stag_agg_fwd_mc scalar Bernoulli in-norm mean", "mc", S("bernoulli", 0.6, in_norm=True), reduce="mean"),
        Case("stag_agg_fwd_w1 explicit", "w1", S("explicit", T.w1, dn=1)),
        Case("stag_agg_fwd_w1 scalar Normal", "w1", S("normal", 1.0, 0.5, dn=1)),
        Case("stag_agg_fwd_w1 [E,1] Uniform relu mean", "w1", S("uniform", T.e0 - 0.6, T.e0 + 0.4, relu=True, dn=1), reduce="mean"),
        Case("stag_agg_fwd_w1 one-element Bernoulli", "w1", S("bernoulli", one, dn=1)),
        Case("stag_agg_fwd_mc_edge Normal p1_log", "mc_edge", S("normal", T.e0, T.e1log, p1_log=True)),
        Case("stag_agg_fwd_mc_edge Uniform relu mean", "mc_edge", S("uniform", T.e0 - 0.6, T.e0 + 0.4, relu=True), reduce="mean"),
        Case("stag_agg_fwd_mc_pedge Normal", "mc_pedge", S("normal", T.q0, T.q1)),
        Case("stag_agg_fwd_mc_pedge Uniform relu", "mc_pedge", S("uniform", T.q0 - 0.6, T.q0 + 0.4, relu=True)),
        Case("stag_agg_bwd none", "bwd", S("none")),
        Case("stag_agg_bwd explicit", "bwd", S("explicit", T.w)),
        Case("stag_agg_bwd Bernoulli", "bwd", S("bernoulli", 0.6)),
        Case("stag_agg_bwd per-channel Normal relu, derivatives", "bwd", S("normal", T.c0, T.c1, relu=True), want_dp=True),
        Case("stag_agg_bwd scalar Uniform, derivatives", "bwd", S("uniform", 0.2, 1.8), want_dp=True),
        Case("stag_agg_bwd_dp per-channel Normal relu", "bwd_dp", S("normal", T.c0, T.c1, relu=True)),
        Case("stag_agg_bwd_dp scalar Uniform", "bwd_dp", S("uniform", 0.2, 1.8)),
        Case("stag_agg_bwd_edge Normal p1_log", "bwd_edge", S("normal", T.e0, T.e1log, p1_log=True)),
        Case("stag_agg_bwd_edge Uniform relu", "bwd_edge", S("uniform", T.e0 - 0.6, T.e0 + 0.4, relu=True)),
        Case("stag_agg_max_fwd none", "max", S("none"), ss=False, ds=False),
        Case("stag_agg_max_fwd explicit", "max", S("explicit", T.w), ss=False, ds=False),
        Case("stag_agg_max_fwd scalar Normal", "max", S("normal", 1.0, 0.5), ss=False, ds=False),
        Case("stag_agg_max_fwd per-channel Bernoulli", "max", S("bernoulli", T.cb), ss=False, ds=False),
    ]


def cases_A_half(D):
    T, S = tables(D), Spec
    return [
        Case("stag_agg_fwd_half none", "half", S("none")),
        Case("stag_agg_fwd_half scalar Normal mean", "half", S("normal", 1.0, 0.5), reduce="mean"),
        Case("stag_agg_fwd_half per-channel Uniform relu", "half", S("uniform", T.c0 - 0.6, T.c0 + 0.4, relu=True)),
        Case("stag_agg_fwd_half scalar Bernoulli", "half", S("bernoulli", 0.6), ss=False),
    ]


def cases_B_exact(D):
    """Group B, exact sums: every weight is exactly 1 (no noise, explicit ones, Bernoulli(1), Normal(1, 0)), no scales."""
    S = Spec
    kw = dict(ss=False, ds=False)
    return [
        Case("stag_agg_fwd none", "fwd", S("none"), **kw),
        Case("stag_agg_fwd Normal(1, 0)", "fwd", S("normal", 1.0, 0.0), **kw),
        _plain("stag_agg_fwd Bernoulli(1)", S("bernoulli", 1.0), ds=False),
        _plain("stag_agg_fwd Normal(1, 0)", S("normal", 1.0, 0.0), ds=False),
        Case("stag_agg_bwd none", "bwd", S("none"), **kw),
        Case("stag_agg_fwd_w1 explicit ones", "w1", S("explicit", np.ones((N_EDGES, 1), np.float32), dn=1), **kw),
    ]


def cases_B_drawn(D):
    """Group B, drawn weights: Normal(1, 0.5) and both scales on x = randn 2^-130."""
    T, S = tables(D), Spec
    half = np.float32(0.5)
    return [
        Case("stag_agg_fwd scalar Normal", "fwd", S("normal", 1.0, 0.5)),
        _plain("stag_agg_fwd scalar Normal", S("normal", 1.0, 0.5)),
        Case("stag_agg_fwd_mc scalar Normal", "mc", S("normal", 1.0, 0.5)),
        Case("stag_agg_fwd_w1 scalar Normal", "w1", S("normal", 1.0, 0.5, dn=1)),
        Case("stag_agg_fwd_mc_edge Normal", "mc_edge", S("normal", np.ones_like(T.e0), np.full_like(T.e0, half))),
        Case("stag_agg_fwd_mc_pedge Normal", "mc_pedge", S("normal", np.ones_like(T.q0), np.full_like(T.q0, half))),
        Case("stag_agg_bwd scalar Normal", "bwd", S("normal", 1.0, 0.5)),
    ]


def cases_C(D):
    """Group C: no noise, explicit positive weights, Normal(1, 0.5) without relu; no in-norm."""
    T, S = tables(D), Spec
    half = np.float32(0.5)
    n = lambda: S("normal", 1.0, 0.5)
    return [
        Case("stag_agg_fwd none", "fwd", S("none")),
        Case("stag_agg_fwd explicit positive mean", "fwd", S("explicit", T.wpos), reduce="mean"),
        Case("stag_agg_fwd scalar Normal", "fwd", n()),
        _plain("stag_agg_fwd scalar Normal", n()),
        Case("stag_agg_fwd_mc scalar Normal", "mc", n()),
        Case("stag_agg_fwd_w1 explicit positive", "w1", S("explicit", T.w1pos, dn=1)),
        Case("stag_agg_fwd_w1 scalar Normal", "w1", S("normal", 1.0, 0.5, dn=1)),
        Case("stag_agg_fwd_mc_edge Normal", "mc_edge", S("normal", T.e0, np.full_like(T.e0, half))),
        Case("stag_agg_fwd_mc_pedge Normal", "mc_pedge", S("normal", T.q0, np.full_like(T.q0, half))),
        Case("stag_agg_bwd none", "bwd", S("none")),
        Case("stag_agg_bwd explicit positive", "bwd", S("explicit", T.wpos)),
        Case("stag_agg_bwd per-channel Normal, derivatives", "bwd", S("normal", T.c0, np.full_like(T.c0, half)), want_dp=True),
        Case("stag_agg_bwd_dp per-channel Normal", "bwd_dp", S("normal", T.c0, np.full_like(T.c0, half))),
        Case("stag_agg_bwd_edge Normal", "bwd_edge", S("normal", T.e0, np.full_like(T.e0, half))),
    ]


def cases_C_half(D):
    S = Spec
    return [Case("stag_agg_fwd_half none", "half", S("none")),
            Case("stag_agg_fwd_half scalar Normal", "half", S("normal", 1.0, 0.5))]


def bernoulli_tables(O, st, D):
    """Group D's Bernoulli tables: exact 0.0 and 1.0 mixed with ordinary values.
    pc [D]: channel k has p = 0, 1, ordinary for k % 3 = 0, 1, 2.
    pe [E, 1], pd [E, D]: p = 0 on every in-edge of the 1-edge row, the 3-edge row, the 20-edge row and the hub (with
    in-norm: the `cur == 0 -> scale 1` branch in a plain sum, a Kahan unit — segments at seg_len 4 — and the group-wise
    combine); elsewhere 1, ordinary, 0 in turn.  On the in-edges of the 40-edge row pd holds the draw itself: p = u on even
    channels (u < p fails: weight 0) and the next float above u on odd channels (weight 1)."""
    if ("bern", D) in _CACHE:
        return _CACHE[("bern", D)]
    T, g = tables(D), st.ogt
    pc = np.where(np.arange(D) % 3 == 0, 0.0, np.where(np.arange(D) % 3 == 1, 1.0, T.cb)).astype(np.float32)
    turn = np.arange(N_EDGES)[:, None] % 3
    pe = np.where(turn == 0, 1.0, np.where(turn == 1, T.eb, 0.0)).astype(np.float32)
    turn = (np.arange(N_EDGES)[:, None] + np.arange(D)[None, :]) % 3
    pd = np.where(turn == 0, 1.0, np.where(turn == 1, T.qb, 0.0)).astype(np.float32)
    u = O.noise_materialize(g, Spec("uniform", 0.0, 1.0).o(O, D), D)               # the draws themselves, by edge id
    assert u.min() >= 0.0 and u.max() < 1.0
    e40 = g.eid[g.indptr[ROW40]:g.indptr[ROW40 + 1]]
    pd[e40] = np.where(np.arange(D) % 2 == 0, u[e40], np.nextafter(u[e40], np.float32(2.0)))
    for r in (ROW1, ROW3, ROW20, HUB):
        e = g.eid[g.indptr[r]:g.indptr[r + 1]]
        pe[e], pd[e] = 0.0, 0.0
    _CACHE[("bern", D)] = (pc, pe, pd, e40)
    return _CACHE[("bern", D)]


def log_table(value, shape):
    """log-scales of one sign between |value| - 1 and |value| in magnitude: +-16, +-15.5, +-15 in turn"""
    i = np.arange(int(np.prod(shape))).reshape(shape)
    return (np.sign(value) * (abs(value) - 0.5 * (i % 3))).astype(np.float32)


def cases_D(O, st, D):
    """Group D: the parameter edges, one aggregation per entry point that takes the kind and the parameter mode."""
    T, S = tables(D), Spec
    f = np.float32
    pc, pe, pd, _ = bernoulli_tables(O, st, D)
    z1, zD, zc = np.zeros_like(T.e0), np.zeros_like(T.q0), np.zeros_like(T.c0)
    out = [
        # ---- Bernoulli p = 0 and p = 1 ----
        Case("stag_agg_fwd Bernoulli(0)", "fwd", S("bernoulli", 0.0), zero=True),
        Case("stag_agg_fwd Bernoulli(1) mean", "fwd", S("bernoulli", 1.0), reduce="mean"),
        Case("stag_agg_fwd Bernoulli(0) in-norm", "fwd", S("bernoulli", 0.0, in_norm=True), zero=True),
        Case("stag_agg_fwd Bernoulli(1) in-norm mean", "fwd", S("bernoulli", 1.0, in_norm=True), reduce="mean"),
        Case("stag_agg_fwd per-channel Bernoulli 0 | 1 | p in-norm", "fwd", S("bernoulli", pc, in_norm=True)),
        Case("stag_agg_fwd [E,1] Bernoulli 0 | 1 | p in-norm", "fwd", S("bernoulli", pe, in_norm=True)),
        Case("stag_agg_fwd [E,D] Bernoulli 0 | 1 | p | the draw in-norm", "fwd", S("bernoulli", pd, in_norm=True)),
        _plain("stag_agg_fwd Bernoulli(0)", S("bernoulli", 0.0), zero=True),
        _plain("stag_agg_fwd Bernoulli(1)", S("bernoulli", 1.0)),
        Case("stag_agg_fwd_mc Bernoulli(0) in-norm", "mc", S("bernoulli", 0.0, in_norm=True), zero=True),
        Case("stag_agg_fwd_mc Bernoulli(1)", "mc", S("bernoulli", 1.0)),
        Case("stag_agg_fwd_mc per-channel Bernoulli 0 | 1 | p in-norm", "mc", S("bernoulli", pc, in_norm=True)),
        Case("stag_agg_fwd_w1 Bernoulli(0)", "w1", S("bernoulli", 0.0, dn=1), zero=True),
        Case("stag_agg_fwd_w1 Bernoulli(1)", "w1", S("bernoulli", 1.0, dn=1)),
        Case("stag_agg_fwd_w1 [E,1] Bernoulli 0 | 1 | p", "w1", S("bernoulli", pe, dn=1)),
        Case("stag_agg_bwd per-channel Bernoulli 0 | 1 | p", "bwd", S("bernoulli", pc)),
        # ---- Normal with scale exactly 0: w == loc ----
        Case("stag_agg_fwd Normal(0.75, 0)", "fwd", S("normal", 0.75, 0.0)),
        _plain("stag_agg_fwd Normal(0.75, 0)", S("normal", 0.75, 0.0)),
        Case("stag_agg_fwd [E,1] Normal(loc, 0)", "fwd", S("normal", T.e0, z1)),
        Case("stag_agg_fwd [E,D] Normal(loc, 0)", "fwd", S("normal", T.q0, zD)),
        Case("stag_agg_fwd_mc Normal(0.75, 0)", "mc", S("normal", 0.75, 0.0)),
        Case("stag_agg_fwd_w1 Normal(0.75, 0)", "w1", S("normal", 0.75, 0.0, dn=1)),
        Case("stag_agg_fwd_w1 [E,1] Normal(loc, 0)", "w1", S("normal", T.e0, z1, dn=1)),
        Case("stag_agg_fwd_mc_edge Normal(loc, 0)", "mc_edge", S("normal", T.e0, z1)),
        Case("stag_agg_fwd_mc_pedge Normal(loc, 0)", "mc_pedge", S("normal", T.q0, zD)),
        Case("stag_agg_bwd Normal(0.75, 0), derivatives", "bwd", S("normal", 0.75, 0.0), want_dp=True),
        Case("stag_agg_bwd_dp per-channel Normal(loc, 0)", "bwd_dp", S("normal", T.c0, zc)),
        Case("stag_agg_bwd_edge Normal(loc, 0)", "bwd_edge", S("normal", T.e0, z1)),
        # ---- Uniform with low == high: w == low ----
        Case("stag_agg_fwd Uniform(0.7, 0.7)", "fwd", S("uniform", 0.7, 0.7)),
        _plain("stag_agg_fwd Uniform(0.7, 0.7)", S("uniform", 0.7, 0.7)),
        Case("stag_agg_fwd [E,1] Uniform(low, low) in-norm", "fwd", S("uniform", T.e0, T.e0, in_norm=True)),
        Case("stag_agg_fwd [E,D] Uniform(low, low)", "fwd", S("uniform", T.q0, T.q0)),
        Case("stag_agg_fwd_mc per-channel Uniform(low, low)", "mc", S("uniform", T.c0, T.c0)),
        Case("stag_agg_fwd_w1 [E,1] Uniform(low, low)", "w1", S("uniform", T.e0, T.e0, dn=1)),
        Case("stag_agg_fwd_mc_edge Uniform(low, low)", "mc_edge", S("uniform", T.e0, T.e0)),
        Case("stag_agg_fwd_mc_pedge Uniform(low, low)", "mc_pedge", S("uniform", T.q0, T.q0)),
        Case("stag_agg_bwd Uniform(0.7, 0.7), derivatives", "bwd", S("uniform", 0.7, 0.7), want_dp=True),
        Case("stag_agg_bwd_dp per-channel Uniform(low, low)", "bwd_dp", S("uniform", T.c0, T.c0)),
        Case("stag_agg_bwd_edge Uniform(low, low)", "bwd_edge", S("uniform", T.e0, T.e0)),
        # ---- a relu that clamps almost everything: Normal(-2, 1); and everything: Normal(0, 0) ----
        Case("stag_agg_fwd Normal(-2, 1) relu", "fwd", S("normal", -2.0, 1.0, relu=True)),
        _plain("stag_agg_fwd Normal(-2, 1) relu", S("normal", -2.0, 1.0, relu=True)),
        Case("stag_agg_fwd_mc Normal(-2, 1) relu", "mc", S("normal", -2.0, 1.0, relu=True)),
        Case("stag_agg_fwd_w1 Normal(-2, 1) relu", "w1", S("normal", -2.0, 1.0, relu=True, dn=1)),
        Case("stag_agg_fwd_mc_edge Normal(-2, 1) relu", "mc_edge", S("normal", z1 - f(2.0), z1 + f(1.0), relu=True)),
        Case("stag_agg_fwd_mc_pedge Normal(-2, 1) relu", "mc_pedge", S("normal", zD - f(2.0), zD + f(1.0), relu=True)),
        Case("stag_agg_bwd Normal(-2, 1) relu, derivatives", "bwd", S("normal", -2.0, 1.0, relu=True), want_dp=True),
        Case("stag_agg_bwd_dp Normal(-2, 1) relu", "bwd_dp", S("normal", -2.0, 1.0, relu=True)),
        Case("stag_agg_bwd_edge Normal(-2, 1) relu", "bwd_edge", S("normal", z1 - f(2.0), z1 + f(1.0), relu=True)),
        Case("stag_agg_fwd Normal(0, 0) relu", "fwd", S("normal", 0.0, 0.0, relu=True), zero=True),
        _plain("stag_agg_fwd Normal(0, 0) relu", S("normal", 0.0, 0.0, relu=True), zero=True),
        Case("stag_agg_fwd_w1 Normal(0, 0) relu", "w1", S("normal", 0.0, 0.0, relu=True, dn=1), zero=True),
        Case("stag_agg_bwd Normal(0, 0) relu, derivatives", "bwd", S("normal", 0.0, 0.0, relu=True), want_dp=True, zero=True),
        Case("stag_agg_bwd_dp Normal(0, 0) relu", "bwd_dp", S("normal", 0.0, 0.0, relu=True), zero=True),
        Case("stag_agg_bwd_edge Normal(0, 0) relu", "bwd_edge", S("normal", z1, z1, relu=True), zero=True),
    ]
    # ---- log-scales of +-16, loc 0: everything divided by e^{+-16} ----
    for sign in LOG_SCALES:
        nm, norm = f"log-scale {sign:+.0f}", float(np.exp(np.float64(sign)))
        l1, lD = log_table(sign, (N_EDGES, 1)), log_table(sign, (N_EDGES, D))
        out += [
            Case(f"stag_agg_fwd scalar {nm}", "fwd", S("normal", 0.0, sign, p1_log=True), norm=norm),
            Case(f"stag_agg_fwd [E,1] {nm}", "fwd", S("normal", z1, l1, p1_log=True), norm=norm),
            Case(f"stag_agg_fwd [E,D] {nm}", "fwd", S("normal", zD, lD, p1_log=True), norm=norm),
            Case(f"stag_agg_fwd_mc_edge {nm}", "mc_edge", S("normal", z1, l1, p1_log=True), norm=norm),
            Case(f"stag_agg_fwd_mc_pedge {nm}", "mc_pedge", S("normal", zD, lD, p1_log=True), norm=norm),
            Case(f"stag_agg_bwd_edge {nm}", "bwd_edge", S("normal", z1, l1, p1_log=True), norm=norm),
        ]
    return out


def cases_D_half(D):
    T, S = tables(D), Spec
    pc = np.where(np.arange(D) % 3 == 0, 0.0, np.where(np.arange(D) % 3 == 1, 1.0, T.cb)).astype(np.float32)
    return [
        Case("stag_agg_fwd_half Bernoulli(0)", "half", S("bernoulli", 0.0), zero=True),
        Case("stag_agg_fwd_half Bernoulli(1)", "half", S("bernoulli", 1.0)),
        Case("stag_agg_fwd_half per-channel Bernoulli 0 | 1 | p", "half", S("bernoulli", pc)),
        Case("stag_agg_fwd_half Normal(0.75, 0)", "half", S("normal", 0.75, 0.0)),
        Case("stag_agg_fwd_half per-channel Uniform(low, low)", "half", S("uniform", T.c0, T.c0)),
        Case("stag_agg_fwd_half Normal(-2, 1) relu", "half", S("normal", -2.0, 1.0, relu=True)),
    ]


def only(cases, D):
    return [c for c in cases if D in c.widths()]


# ---- references --------------------------------------------------------------------------------------------------------
def graph_of(st, case):
    return st.ogf if case.view == "f" else st.ogt


def _scales(case, T):
    return (T.ss if case.ss else None), (T.ds if case.ds else None)


def weights(O, st, case, D, deriv=0, offset=OFFSET, in_norm=None):
    """The oracle's materialised weights [E, D] by edge id (a width-1 description repeated over the channels)."""
    g, sp = graph_of(st, case), case.spec
    dn = sp.dn or D
    W = O.noise_materialize(g, sp.o(O, D, deriv=deriv, offset=offset, in_norm=in_norm), dn)
    return np.ascontiguousarray(np.repeat(W, D, 1)) if dn != D else W


def _offsets(case):
    if case.entry == "mc":
        return [OFFSET + s * MC_STRIDE for s in range(MC_S)]
    if case.entry in ("mc_edge", "mc_pedge"):
        return [OFFSET + s * MCE_STRIDE for s in range(MCE_S)]
    return None


def reference(O, st, case, T):
    """The oracle's outputs of the case on the tables T, in the order the launch returns them."""
    g, sp, D = graph_of(st, case), case.spec, T.D
    ss, ds = _scales(case, T)
    red = O.REDUCE_MEAN if case.reduce == "mean" else O.REDUCE_SUM
    with np.errstate(all="ignore"):
        if case.entry == "max":
            return [numpy_max(g, T.x, weights(O, st, case, D))]
        if sp.dn and sp.dn != D:             # a weight of width 1: the same sum with its column repeated
            agg = lambda deriv=0, offset=OFFSET: O.agg_fwd(g, T.x, O.make_spec("explicit", weights(O, st, case, D, deriv, offset)),
                                                           reduce=red, src_scale=ss, dst_scale=ds)
        else:
            agg = lambda deriv=0, offset=OFFSET: O.agg_fwd(g, T.x, sp.o(O, D, deriv=deriv, offset=offset), reduce=red,
                                                           src_scale=ss, dst_scale=ds)
        if _offsets(case):
            return [np.stack([agg(offset=o) for o in _offsets(case)], 0)]
        if case.entry == "bwd" and case.want_dp:
            return [agg(dv) for dv in (0, 1, 2)]
        if case.entry == "bwd_dp":
            return [agg(0)] + [(T.own.astype(np.float64) * agg(dv).astype(np.float64)).sum(0) for dv in (1, 2)]
        if case.entry == "bwd_edge":
            assert case.view == "t"
            gx = T.x * (ss[:, None] if ss is not None else np.float32(1.0))
            return [agg(0)] + [O.agg_bwd_w(st.og, T.own, gx, src_scale=ds, spec=sp.o(O, D, deriv=dv)).astype(np.float64)
                               .sum(1, keepdims=True) for dv in (1, 2)]
        return [agg(0)]


def numpy_agg(g, x, W, ss=None, ds=None, mean=False):
    """out[v] = ds[v] (sum | mean) over the in-edges p of v of W[eid[p]] * ss[u_p] * x[u_p], in float64"""
    out = np.zeros((g.n_dst, x.shape[1]), np.float64)
    with np.errstate(all="ignore"):
        for v in range(g.n_dst):
            for p in range(g.indptr[v], g.indptr[v + 1]):
                u = g.indices[p]
                out[v] += W[g.eid[p]].astype(np.float64) * (x[u].astype(np.float64) * (1.0 if ss is None else float(ss[u])))
            out[v] *= (1.0 if ds is None else float(ds[v])) / (max(g.indptr[v + 1] - g.indptr[v], 1) if mean else 1)
    return out


def numpy_max(g, x, W):
    """stag_agg_max_fwd: the largest fp32 product over a row's in-edges (NaN if any is NaN), +0 for a row without any"""
    out = np.zeros((g.n_dst, x.shape[1]), np.float32)
    for v in range(g.n_dst):
        p = np.arange(g.indptr[v], g.indptr[v + 1])
        if len(p):
            out[v] = (W[g.eid[p]] * x[g.indices[p]]).astype(np.float32).max(0)
    return out


def numpy_reference(O, st, case, T):
    """reference() again from the float64 loop above on the oracle's materialised weights (in-norm included in them)."""
    with np.errstate(all="ignore"):
        return _numpy_reference(O, st, case, T)


def _numpy_reference(O, st, case, T):
    g, D = graph_of(st, case), T.D
    ss, ds = _scales(case, T)
    agg = lambda deriv=0, offset=OFFSET: numpy_agg(g, T.x, weights(O, st, case, D, deriv, offset), ss, ds, case.reduce == "mean")
    if case.entry == "max":
        return [numpy_max(g, T.x, weights(O, st, case, D)).astype(np.float64)]
    if _offsets(case):
        return [np.stack([agg(offset=o) for o in _offsets(case)], 0)]
    if case.entry == "bwd" and case.want_dp:
        return [agg(dv) for dv in (0, 1, 2)]
    if case.entry == "bwd_dp":
        return [agg(0)] + [(T.own.astype(np.float64) * agg(dv)).sum(0) for dv in (1, 2)]
    if case.entry == "bwd_edge":
        outs = [agg(0)]
        rows, cols = st.row_of_pos, g.indices
        for dv in (1, 2):
            W = weights(O, st, case, D, dv).astype(np.float64)
            term = (T.x[cols].astype(np.float64) * (1.0 if ss is None else ss[cols, None].astype(np.float64))
                    * T.own[rows].astype(np.float64) * (1.0 if ds is None else ds[rows, None].astype(np.float64)))
            eg = np.zeros((N_EDGES, 1), np.float64)
            eg[g.eid, 0] = (W[g.eid] * term).sum(1)
            outs.append(eg)
        return outs
    return [agg(0)]


def out_scale(kind, ref):
    """What an output and its reference are divided by before the 1e-5 bar: nothing for sums over one row; the largest
    entry for the gradients of parameters, which add every edge of the graph (as tests/test_gpu_address_forms.py does)."""
    ref = np.asarray(ref, np.float64)
    finite = np.abs(ref[np.isfinite(ref)])
    return max(1.0, float(finite.max()) if finite.size else 0.0) if kind in ("chan", "edge") else 1.0


def subnormal_bar(st, ref, kind):
    """Group B: 1e-5 |ref| + 2 (indeg(v) + 2) 2^-149 — every term and every scaling is rounded once to the subnormal
    grid, at most 2^-150 each, twice over for margin"""
    deg = st.indeg.astype(np.float64)[:, None]
    bar = 1e-5 * np.abs(np.asarray(ref, np.float64)) + 2.0 * (deg + 2.0) * TINY
    assert kind in ("rows", "mc")
    return bar


# ======================================================================================================================
# The per-edge gradient entry points (stag_agg_bwd_w, _bwd_w_mc, _bwd_pedge), the max reducer's backward and count, and
# the small reductions (stag_coldot, stag_segment_reduce): tests/test_gpu_value_range_grad.py, host proofs in
# tests/test_value_range_host.py.
#
# ONE LAYOUT serves the three gradient entry points, all launched on the view "t" (ogt: eid and nidx permutations):
#   `x`     [N, D]     the table an edge GATHERS through the column id c (stag_agg_bwd_w's x with src_scale = ss;
#                      stag_agg_bwd_pedge's g with g_scale = ss)
#   `g_all` [S, N, D]  the rows the units OWN, one table per sample (stag_agg_bwd_w's g: sample 0, no scale of its own;
#                      stag_agg_bwd_w_mc's g with g_scale = ds; stag_agg_bwd_pedge's x with row_scale = ds: sample 0)
#   dw_i[eid_p, k] = sum_s D_i,s[p, k] (ss[c_p] x[c_p, k]) (ds[r_p] g_all[s, r_p, k])         (then summed over k: reduce_k)
#   dx[r, k]       = ds[r] sum_{p in row r} w[p, k] ss[c_p] x[c_p, k]                           (stag_agg_bwd_pedge only)
# D_i,s: the oracle's derivative weights at offset OFFSET + s GRAD_STRIDE (weights(..., deriv=i + 1)).
# ======================================================================================================================
GRAD_S, GRAD_STRIDE = 7, 2                 # stag_agg_bwd_w_mc, group A, C, D: passes of 4, 2 and 1 samples
GRAD_S_SMALL = 3                           # group B: passes of 2 and 1
GRAD_POISON_SAMPLE = 5                     # group C: in the second pass (samples 4 and 5), which reads the first one back
V0 = ROW20                                 # group C: the owned row that is poisoned (20 in-edges; row V0 + 1 follows it)
MARGIN = 4.0                               # group A: no intermediate of the 2^-100 launch below MARGIN 2^-126, none of
FLT_MAX = float(np.finfo(np.float32).max)  # the 2^100 launch above FLT_MAX / MARGIN
COLDOT_N = 300


class GradTables:
    """Group A's tables are kept away from zero (as x16 is): an output is a product of up to three factors, and the
    smallest of them, a Uniform derivative u = 2^-24, must stay normal under c = 2^-100.  |x| in [1, 4), |g| in [4, 16)."""

    def __init__(self, D):
        rng = np.random.default_rng(5000 + D)
        T = tables(D)
        away = lambda lo, hi, shape: (rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
        self.D = D
        self.x = away(1.0, 4.0, (N, D))
        self.g_all = away(4.0, 16.0, (GRAD_S, N, D))
        self.ss, self.ds = T.ss, T.ds
        self.qlog = rng.uniform(-1.0, 0.0, (N_EDGES, D)).astype(np.float32)
        self.gint = rng.integers(-3, 4, (N, D)).astype(np.float32)          # group B: small integers
        self.xint = rng.integers(-2, 3, (N, D)).astype(np.float32)          # max ties: few distinct values
        self.grand = rng.standard_normal((GRAD_S, N, D)).astype(np.float32)   # groups B (drawn), C, D: ordinary rows


def grad_tables(D):
    if ("GT", D) not in _CACHE:
        _CACHE[("GT", D)] = GradTables(D)
    return _CACHE[("GT", D)]


class GradCase:
    """entry: bwd_w | bwd_w_mc | bwd_pedge.  mode: "plain" (no spec: D = 1) | 1 | 2 (one derivative, spec.deriv) | "both".
    outputs(): (name, derivative) in launch order; derivative None: D = 1, 0: the weight itself (dx)."""

    def __init__(self, name, entry, spec=None, mode="both", reduce_k=False, ss=True, S=1, norm=1.0, zero=False):
        self.name, self.entry, self.spec, self.mode, self.reduce_k, self.ss, self.S = name, entry, spec, mode, reduce_k, ss, S
        self.norm, self.zero = norm, zero
        assert entry in ("bwd_w", "bwd_w_mc", "bwd_pedge") and (entry == "bwd_w" or mode == "both")
        assert (spec is None) == (mode == "plain") and (S == 1 or entry == "bwd_w_mc")
        if entry == "bwd_pedge":
            assert not reduce_k and spec.p0.ndim == 2 and spec.p0.shape[1] > 1
        if entry == "bwd_w_mc":
            assert reduce_k == (spec.p0.shape[1] == 1)
        self.ds = entry != "bwd_w"                      # stag_agg_bwd_w's g already carries the destination scale

    def outputs(self):
        if self.entry == "bwd_pedge":
            return [("dx", 0), ("dp0", 1), ("dp1", 2)]
        if self.mode == "plain":
            return [("dw", None)]
        if self.mode == "both":
            return [("dw0", 1), ("dw1", 2)]
        return [(f"dw (deriv {self.mode})", self.mode)]

    def kinds(self):
        """dx: rows (the 1e-5 (1 + |ref|) bar of a sum over one row); a gradient table: relative to its largest entry"""
        return ["rows" if d == 0 else "edge" for _, d in self.outputs()]

    def norms(self):
        """d/dloc does not carry the scale; the weight and d/dlog_scale do"""
        return [1.0 if d in (None, 1) else self.norm for _, d in self.outputs()]


def cases_grad_A(D):
    GT, T, S = grad_tables(D), tables(D), Spec
    nD, n1 = lambda: S("normal", T.q0, GT.qlog, p1_log=True), lambda: S("normal", T.e0, T.e1log, p1_log=True)
    uD, u1 = lambda: S("uniform", T.q0, T.q0 + T.q1), lambda: S("uniform", T.e0, T.e0 + T.e1)
    G = GradCase
    return [
        G("stag_agg_bwd_w no spec", "bwd_w", None, "plain"),
        G("stag_agg_bwd_w no spec reduce_k", "bwd_w", None, "plain", reduce_k=True),
        G("stag_agg_bwd_w [E,D] Normal p1_log d/dp0", "bwd_w", nD(), 1),
        G("stag_agg_bwd_w [E,D] Normal p1_log d/dp1", "bwd_w", nD(), 2),
        G("stag_agg_bwd_w [E,D] Normal p1_log both", "bwd_w", nD(), "both"),
        G("stag_agg_bwd_w [E,1] Normal p1_log reduce_k d/dp0", "bwd_w", n1(), 1, reduce_k=True),
        G("stag_agg_bwd_w [E,1] Normal p1_log reduce_k d/dp1", "bwd_w", n1(), 2, reduce_k=True),
        G("stag_agg_bwd_w [E,1] Normal p1_log reduce_k both", "bwd_w", n1(), "both", reduce_k=True),
        G("stag_agg_bwd_w [E,D] Uniform both", "bwd_w", uD(), "both"),
        G("stag_agg_bwd_w [E,D] Uniform d/dp1", "bwd_w", uD(), 2),
        G("stag_agg_bwd_w [E,1] Uniform reduce_k both", "bwd_w", u1(), "both", reduce_k=True),
        G("stag_agg_bwd_w_mc [E,D] Normal p1_log", "bwd_w_mc", nD(), S=GRAD_S),
        G("stag_agg_bwd_w_mc [E,1] Normal p1_log reduce_k", "bwd_w_mc", n1(), reduce_k=True, S=GRAD_S),
        G("stag_agg_bwd_w_mc [E,D] Uniform", "bwd_w_mc", uD(), S=GRAD_S),
        G("stag_agg_bwd_w_mc [E,1] Uniform reduce_k", "bwd_w_mc", u1(), reduce_k=True, S=GRAD_S),
        G("stag_agg_bwd_pedge [E,D] Normal p1_log", "bwd_pedge", nD()),
        G("stag_agg_bwd_pedge [E,D] Uniform", "bwd_pedge", uD()),
    ]


def cases_grad_B(D):
    """Group B, drawn: Normal(1, 0.5) in [E, D] and [E, 1] tables."""
    T, S = tables(D), Spec
    half = np.float32(0.5)
    nD = lambda: S("normal", np.ones_like(T.q0), np.full_like(T.q0, half))
    n1 = lambda: S("normal", np.ones_like(T.e0), np.full_like(T.e0, half))
    G = GradCase
    return [
        G("stag_agg_bwd_w [E,D] Normal both", "bwd_w", nD(), "both"),
        G("stag_agg_bwd_w [E,1] Normal reduce_k both", "bwd_w", n1(), "both", reduce_k=True),
        G("stag_agg_bwd_w_mc [E,D] Normal", "bwd_w_mc", nD(), S=GRAD_S_SMALL),
        G("stag_agg_bwd_w_mc [E,1] Normal reduce_k", "bwd_w_mc", n1(), reduce_k=True, S=GRAD_S_SMALL),
        G("stag_agg_bwd_pedge [E,D] Normal", "bwd_pedge", nD()),
    ]


def cases_grad_C(D):
    """Group C: Normal tables without relu, loc from the tables, scale 0.5 (log-scale log 0.5 where p1_log)."""
    T, S = tables(D), Spec
    half = np.float32(0.5)
    nD = lambda: S("normal", T.q0, np.full_like(T.q0, half))
    nDlog = lambda: S("normal", T.q0, np.full_like(T.q0, np.log(half)), p1_log=True)
    n1 = lambda: S("normal", T.e0, np.full_like(T.e0, half))
    G = GradCase
    return [
        G("stag_agg_bwd_w no spec", "bwd_w", None, "plain"),
        G("stag_agg_bwd_w no spec reduce_k", "bwd_w", None, "plain", reduce_k=True),
        G("stag_agg_bwd_w [E,D] Normal d/dp1", "bwd_w", nD(), 2),
        G("stag_agg_bwd_w [E,D] Normal p1_log both", "bwd_w", nDlog(), "both"),
        G("stag_agg_bwd_w [E,1] Normal reduce_k both", "bwd_w", n1(), "both", reduce_k=True),
        G("stag_agg_bwd_w_mc [E,D] Normal p1_log", "bwd_w_mc", nDlog(), S=GRAD_S),
        G("stag_agg_bwd_w_mc [E,1] Normal reduce_k", "bwd_w_mc", n1(), reduce_k=True, S=GRAD_S),
        G("stag_agg_bwd_pedge [E,D] Normal p1_log", "bwd_pedge", nDlog()),
    ]


def cases_grad_D(D):
    T, S = tables(D), Spec
    f = np.float32
    z1, zD = np.zeros_like(T.e0), np.zeros_like(T.q0)
    G = GradCase

    def trio(name, sD, s1, **kw):
        return [G(f"stag_agg_bwd_w [E,D] {name} both", "bwd_w", sD(), "both", **kw),
                G(f"stag_agg_bwd_w [E,1] {name} reduce_k both", "bwd_w", s1(), "both", reduce_k=True, **kw),
                G(f"stag_agg_bwd_w_mc [E,D] {name}", "bwd_w_mc", sD(), S=GRAD_S, **kw),
                G(f"stag_agg_bwd_w_mc [E,1] {name} reduce_k", "bwd_w_mc", s1(), reduce_k=True, S=GRAD_S, **kw),
                G(f"stag_agg_bwd_pedge [E,D] {name}", "bwd_pedge", sD(), **kw)]

    out = trio("Normal(loc, 0)", lambda: S("normal", T.q0, zD), lambda: S("normal", T.e0, z1))
    out += trio("Normal(loc, log-scale -16)", lambda: S("normal", T.q0, zD - f(16.0), p1_log=True),
                lambda: S("normal", T.e0, z1 - f(16.0), p1_log=True))
    out += trio("Uniform(low, low)", lambda: S("uniform", T.q0, T.q0), lambda: S("uniform", T.e0, T.e0))
    out += trio("Normal(-2, 1) relu", lambda: S("normal", zD - f(2.0), zD + f(1.0), relu=True),
                lambda: S("normal", z1 - f(2.0), z1 + f(1.0), relu=True))
    out += trio("Normal(0, 0) relu", lambda: S("normal", zD, zD, relu=True), lambda: S("normal", z1, z1, relu=True), zero=True)
    for sign in LOG_SCALES:
        norm = float(np.exp(np.float64(sign)))
        out += trio(f"log-scale {sign:+.0f}", lambda: S("normal", zD, log_table(sign, (N_EDGES, D)), p1_log=True),
                    lambda: S("normal", z1, log_table(sign, (N_EDGES, 1)), p1_log=True), norm=norm)
    return out


def _wcase(spec):
    return Case("weights", "fwd", spec, view="t")


def grad_reference(O, st, gc, D, x, g_all, ss, ds, track=None, f32=False):
    """The outputs of the case in launch order.  float64: the header's formula.  f32=True: the same in fp32, every product
    and every sum rounded where the kernels round (ss x, ds g, their product, times the derivative; samples added in
    increasing s from sample 0's term; the sum over k in channel order) — the emulation group B's bars are proved on.
    track: a dict that receives lo / hi, the smallest non-zero and the largest magnitude of any intermediate."""
    g = st.ogt
    rows, cols, eid = st.row_of_pos, g.indices, g.eid
    ft = np.float32 if f32 else np.float64
    mags = []

    def see(a):
        a = np.abs(np.asarray(a, np.float64))
        a = a[np.isfinite(a) & (a > 0)]
        if track is not None and a.size:
            mags.append((a.min(), a.max()))
        return a

    with np.errstate(all="ignore"):
        a = x[cols].astype(ft)
        if gc.ss:
            a = (ss[cols, None].astype(ft) * a).astype(ft)
        see(a)
        acc = {}
        for s in range(gc.S):
            b = g_all[s][rows].astype(ft)
            if gc.ds:
                b = (ds[rows, None].astype(ft) * b).astype(ft)
            val = (a * b).astype(ft)
            see(b), see(val)
            for _, d in gc.outputs():
                if d == 0:
                    continue
                if d is None:
                    term = val
                else:
                    Wd = weights(O, st, _wcase(gc.spec), D, deriv=d, offset=OFFSET + s * GRAD_STRIDE)[eid].astype(ft)
                    term = (Wd * val).astype(ft)
                see(term)
                acc[d] = term if s == 0 else (acc[d] + term).astype(ft)
                see(acc[d])
        outs = []
        for _, d in gc.outputs():
            if d == 0:
                W = weights(O, st, _wcase(gc.spec), D)
                if f32:
                    dx = np.zeros((N, D), np.float32)
                    for p in range(N_EDGES):
                        dx[rows[p]] += W[eid[p]] * a[p]
                    dx = dx * ds[:, None]
                else:
                    dx = numpy_agg(g, x, W, ss if gc.ss else None, ds)
                see(W[eid].astype(np.float64) * np.asarray(a, np.float64)), see(dx)
                outs.append(dx)
                continue
            o = np.zeros((N_EDGES, D), ft)
            o[eid] = acc[d]
            if gc.reduce_k:
                if f32:
                    tot = np.zeros(N_EDGES, np.float32)
                    for k in range(D):
                        tot = tot + o[:, k]
                    o = tot[:, None]
                else:
                    see(np.cumsum(o, 1))
                    o = o.sum(1, keepdims=True)
            see(o)
            outs.append(o)
    if track is not None:
        track["lo"], track["hi"] = min(m[0] for m in mags), max(m[1] for m in mags)
    return outs


def grad_subnormal_bars(O, st, gc, D, g_all, ds, refs):
    """Group B: 1e-5 |ref| + r 2^-149 f per output.
    dw_i: a term D (ss x) (ds g) of a subnormal x is rounded r0 = 3 times on its way (ss x; times ds g; times D), each by at
    most 2^-150, and what is later multiplied into a rounded value is ds g and D: f = max(1, |ds g|) max(1, |D|), the
    largest over the element's terms.  Sums of subnormals are exact, a sum that reaches the normal range is rounded by at
    most 2^-150 per addition while it stays below 2^-125: r = (r0 + 1) x the number of terms (S samples, x D with reduce_k).
    dx: a term w (ss x) is rounded twice (f = max(1, |w|)), the block sums and the Kahan folds add at most three roundings
    per term, the row scale one more: r = 5 indeg + 1, f = max(1, max |w|) max(1, ds)."""
    rows, eid = st.row_of_pos, st.ogt.eid
    bars = []
    for (_, d), ref in zip(gc.outputs(), refs):
        if d == 0:
            W = np.abs(weights(O, st, _wcase(gc.spec), D).astype(np.float64))
            f = np.ones((N, D))
            np.maximum.at(f, rows, W[eid])
            f *= np.maximum(1.0, ds.astype(np.float64))[:, None]
            r = 5.0 * st.indeg[:, None] + 1.0
        else:
            f = np.zeros((N_EDGES, D))
            for s in range(gc.S):
                b = np.abs(g_all[s][rows].astype(np.float64) * (ds[rows, None] if gc.ds else 1.0))
                Wd = np.abs(weights(O, st, _wcase(gc.spec), D, deriv=d, offset=OFFSET + s * GRAD_STRIDE)[eid].astype(np.float64))
                f[eid] = np.maximum(f[eid], np.maximum(1.0, b) * np.maximum(1.0, Wd))
            r = 4.0 * gc.S
            if gc.reduce_k:
                f, r = f.max(1, keepdims=True), r * D
        bars.append(1e-5 * np.abs(np.asarray(ref, np.float64)) + r * TINY * f)
    return bars


# ---- group C: where the poison goes --------------------------------------------------------------------------------
def poison_edge(st):
    """EP: the edge id whose parameter row is poisoned — the hub's 11th in-edge; the row of edge EP + 1 follows it in
    memory, and that edge belongs to another CSR row."""
    g = st.ogt
    return int(g.eid[g.indptr[HUB] + 10])


def poison_sets(st, D, reduce_k):
    """The affected sets of group C as masks over an [E, D] (or [E, 1]) gradient table, by edge id."""
    g = st.ogt
    cols = 1 if reduce_k else D
    ch = [0] if reduce_k else list(POISON[D])
    from_u, into_v0, at_ep = (np.zeros((N_EDGES, cols), bool) for _ in range(3))
    from_u[np.ix_(st.eid_from_u, ch)] = True
    into_v0[np.ix_(g.eid[g.indptr[V0]:g.indptr[V0 + 1]], ch)] = True
    at_ep[poison_edge(st), ch] = True
    return from_u, into_v0, at_ep


def poisoned_row(a, row, D):
    b = np.array(a, np.float32)
    b[row, list(POISON[D])] = POISON_VALUES
    return b


def poisoned_param(spec, st, D, which):
    """A copy of a Normal spec with one edge's parameters poisoned: which = "p0" (NaN) | "p1" (+inf: a log-scale, or a
    scale), in the poisoned channels of an [E, D] table, in the edge's one entry of an [E, 1] table."""
    p0, p1 = np.array(spec.p0, np.float32), np.array(spec.p1, np.float32)
    ch = [0] if p0.shape[1] == 1 else list(POISON[D])
    (p0 if which == "p0" else p1)[poison_edge(st), ch] = np.nan if which == "p0" else np.inf
    return Spec(spec.kind, p0, p1, relu=spec.relu, p1_log=spec.p1_log)


# ---- the max reducer: forward count and backward --------------------------------------------------------------------
def max_fwd_reference(st, x, W):
    """(m [E positions, D] the fp32 messages in CSR order, out, cnt) of stag_agg_max_fwd on ogt; W by edge id (None: no weight)"""
    g = st.ogt
    with np.errstate(all="ignore"):
        xs = np.asarray(x, np.float32)[g.indices]
        m = xs if W is None else (np.asarray(W, np.float32)[g.eid] * xs).astype(np.float32)
        out = np.zeros((N, x.shape[1]), np.float32)
        cnt = np.zeros((N, x.shape[1]), np.int32)
        for v in range(N):
            p = slice(g.indptr[v], g.indptr[v + 1])
            if g.indptr[v + 1] > g.indptr[v]:
                mv = m[p]
                out[v] = mv.max(0)                                  # NaN if any is NaN
                first = (mv == out[v]).argmax(0)                    # ties keep the bits of the first maximal message
                fb = mv[first, np.arange(mv.shape[1])]
                out[v] = np.where(np.isnan(out[v]), out[v], fb)
                cnt[v] = (mv == out[v]).sum(0)                      # a NaN out compares equal to nothing: 0
    return m, out, cnt


def max_bwd_reference(st, x, W, out, cnt, gr, D0=None, D1=None, track=None):
    """The header's three lines as a loop over the edges, in float64; [m == out] selects (a message that is not maximal
    receives 0, whatever g holds).  Returns dx [N, D], dw [E, D] by edge id, dp0_rows, dp1_rows (zeros without D0 / D1) and
    the ties by CSR position.  track: a list that receives every intermediate (messages, g / cnt, terms, running sums)."""
    g = st.ogt
    Dw = x.shape[1]
    with np.errstate(all="ignore"):
        m, _, _ = max_fwd_reference(st, x, W)
        gq = np.where(cnt > 0, np.asarray(gr, np.float64) / np.maximum(cnt, 1), 0.0)
        dx, dp0, dp1 = (np.zeros((N, Dw), np.float64) for _ in range(3))
        dw = np.zeros((N_EDGES, Dw), np.float64)
        tied = np.zeros((N_EDGES, Dw), bool)                        # by CSR position
        x64 = np.asarray(x, np.float64)
        for p in range(N_EDGES):
            v, u, e = st.row_of_pos[p], g.indices[p], g.eid[p]
            tie = m[p] == out[v]
            tied[p] = tie
            t = np.where(tie, gq[v], 0.0)
            w = 1.0 if W is None else W[e].astype(np.float64)
            dx[u] += w * t
            dw[e] = x64[u] * t
            if D0 is not None:
                dp0[u] += D0[e].astype(np.float64) * t
                dp1[u] += D1[e].astype(np.float64) * t
            if track is not None:
                track += [w * t, dw[e], dx[u].copy()] + ([D0[e] * t, D1[e] * t, dp0[u].copy(), dp1[u].copy()] if D0 is not None else [])
        if track is not None:
            track += [m, gq]
    return dx, dw, dp0, dp1, tied


def max_specs_A(D):
    """Group A of the max reducer: the kinds stag_agg_max_bwd takes, EXPLICIT with weights of both signs"""
    T = tables(D)
    return {"none": Spec("none"), "explicit": Spec("explicit", T.w), "per-channel Normal": Spec("normal", T.c0, T.c1),
            "scalar Uniform": Spec("uniform", 0.2, 1.8)}


def planted_duplicates(st, D):
    """Group D: EXPLICIT weights and a table x with exact duplicates of the hub's maximum planted across a segment boundary
    at seg_len 4 — hub positions 2, 3 (segment 0), 4 (segment 1) and 41 (segment 10) carry w x = 64 in every channel, far
    above every other message; (W by edge id, x, the four positions)."""
    T, g = tables(D), st.ogt
    W = np.array(T.wpos, np.float32)
    x = np.array(T.x, np.float32)
    pos = g.indptr[HUB] + np.array([2, 3, 4, 41])
    srcs = g.indices[pos]
    x[srcs] = 8.0
    W[g.eid[pos]] = 8.0
    return W, x, pos


# ---- stag_coldot, stag_segment_reduce -------------------------------------------------------------------------------
SEGMENT_OFFSETS = np.array([0, 0, 1, 4, 8, 13, 13, 22, 39, 48, 48], np.int32)      # empty, 1, 3, 4, 5, empty, 9, 17, 9, empty


def coldot_big_n(D):
    """a row count past the second grid-stride trip of stag_coldot's first stage: 1024 blocks x R rows, twice, and some"""
    elems = D // 4 if D % 4 == 0 else D
    cw = 1
    while cw < elems and cw < 256:
        cw <<= 1
    return 2 * 1024 * (256 // cw) + 37


def away_table(seed, shape, lo=1.0, hi=4.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
