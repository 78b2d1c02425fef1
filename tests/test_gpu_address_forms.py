"""Every aggregation entry point on both sides of its address-form switch.

The host picks how a kernel addresses the gathered table x and the per-edge tables (csrc/entry_args.hpp: narrow_rows for
agg_half / agg_w1 / agg_mc_edge / agg_mc_pedge, agg_forms for the kernels of agg_common): a 32-bit buffer descriptor with a
24-bit multiply, a 32-bit global offset, or 64-bit addresses.  The switch changes which load every lane issues and no
arithmetic, so each launch here is checked twice: against the float64 oracle on the compact graph (the gathered rows
relabelled 0..m-1; the Philox position is the CSR position or nidx, never the source id, so the draws are the same) at
util.TOL under the device's normal tables, and bit for bit (torch.equal) against the same launch on the compact layout,
which takes the narrow form.  The tables are random everywhere, so a wrongly addressed row does not read zero.

FORMS: the smallest tables that flip each reason of the switch — (a) rows past 2^24, (b) a row stride of 2^24 bytes,
(c) an extent past 2^32 bytes with few rows and a small stride — and (d) the top of the narrow form, where 32-bit offsets,
the descriptor's record count and the 24-bit products use all their bits.  tests/test_address_forms_host.py puts every one
of them through the rules themselves, so the shapes and the rules cannot drift apart."""
import numpy as np
import pytest
import torch

from util import TOL, assert_close, assert_close_cond, hw_normals

pytestmark = pytest.mark.gpu

K24 = 1 << 24
FORMS = {
    # stride_bytes: of the fp32 table and of the half tables alike; widths: a vectorised one and one with D % 4 != 0 inside
    # the same stride (row_at's 32-bit global form in agg_kernel, load4's fallback in the plan-order clients)
    "a": dict(n_src=K24 + 5, stride_bytes=32, widths=(8, 6), sources=[0, 5, K24 - 1, K24, K24 + 4], wide=True, straddles=()),
    "b": dict(n_src=6, stride_bytes=1 << 24, widths=(8, 6), sources=[0, 1, 2, 3, 4, 5], wide=True, straddles=()),
    "c": dict(n_src=(1 << 20) + 3, stride_bytes=4096, widths=(8, 6), wide=True, straddles=(1 << 31, 1 << 32),
              sources=[0, (1 << 19) - 1, 1 << 19, (1 << 20) - 1, 1 << 20, (1 << 20) + 2]),
    "d": dict(n_src=K24 - 1, stride_bytes=256, widths=(64, 6), wide=False, straddles=(1 << 31,),
              sources=[0, (1 << 23) - 1, 1 << 23, K24 - 2]),
}
DEG = (5, 0, 40, 1)          # the destination side: five edges, none, a hub of three segments at seg_len 16, one edge
N_EDGES = sum(DEG)
SEGS = (0, 16)
HALF_D = 8
SEED, OFFSET = 11, 2

PE_EDGES, PE_N_DST, PE_N_SRC = K24 + 64, 8000, 1000          # the per-edge forms: CSR positions and edge ids past 2^24
PE_A1, PE_B1, PE_A2, PE_B2 = 1000003, 12345, 7919, 777       # eid = (p A1 + B1) mod E, nidx = (p A2 + B2) mod E


@pytest.fixture(autouse=True)
def _ctypes_front_end(monkeypatch):
    """The raw helpers through ctypes, which takes a strided table as it is (the dispatcher ops want contiguous ones)."""
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


def _mode(p, D):
    from stag_amd import _lib
    if not isinstance(p, np.ndarray):
        return _lib.PARAM_SCALAR
    if p.ndim == 1:
        return _lib.PARAM_PER_CHANNEL
    return _lib.PARAM_PER_EDGE1 if p.shape[1] == 1 else _lib.PARAM_PER_EDGE


class _Spec:
    """One noise description in both forms: .c the library's stag_noise_spec (parameters on the device), .o(deriv, offset)
    the oracle's.  p0 / p1: python floats, [D], [E, 1] or [E, D] float32 arrays (by edge id)."""

    def __init__(self, O, dev, kind, p0=None, p1=None, D=None, n_edges=None, relu=False, in_norm=False, p1_log=False,
                 seed=SEED, offset=OFFSET):
        from stag_amd import _lib
        self.O, self.kind, self.p0, self.p1, self.D, self.E = O, kind, p0, p1, D, n_edges
        self.kw = dict(relu=relu, in_norm=in_norm, seed=seed, p1_log=p1_log)
        self.offset = offset
        s = _lib.NoiseSpec()
        s.kind = {"none": _lib.NOISE_NONE, "explicit": _lib.NOISE_EXPLICIT, "normal": _lib.NOISE_NORMAL,
                  "uniform": _lib.NOISE_UNIFORM}[kind]
        self.keep = [_dev(p, dev) if isinstance(p, np.ndarray) else None for p in (p0, p1)]
        s.p0, s.p1 = _lib.ptr(self.keep[0]), _lib.ptr(self.keep[1])
        if s.kind >= _lib.NOISE_NORMAL:
            s.param_mode = max(_mode(p0, D), _mode(p1, D))
            if s.param_mode == _lib.PARAM_SCALAR:
                s.p0_scalar, s.p1_scalar = float(p0), float(p1)
        s.relu, s.in_norm, s.p1_log, s.seed, s.offset = int(relu), int(in_norm), int(p1_log), seed, offset
        self.c = s

    def o(self, deriv=0, offset=None):
        if self.kind in ("none", "explicit"):
            return self.O.make_spec(self.kind, self.p0, relu=self.kw["relu"], in_norm=self.kw["in_norm"])
        return self.O.make_spec(self.kind, self.p0, self.p1, Dn=self.D, n_edges=self.E, deriv=deriv,
                                offset=self.offset if offset is None else offset, **self.kw)


def _structure(O, m, seed):
    """The four destination rows of DEG over m sources, as the oracle's pair of graphs: og — rows = the m table rows,
    columns = the four — and its transpose ogt, the view every launch here walks (rows = the four, columns = table rows,
    eid a permutation, nidx = the positions of og, another permutation: what a backward launch is handed).  The hub and
    the row of five gather every source."""
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(4), DEG)
    v = rng.integers(0, m, N_EDGES)
    v[DEG[0]:DEG[0] + m] = rng.permutation(m)
    v[:min(DEG[0], m)] = rng.permutation(m)[:DEG[0]]
    order = rng.permutation(N_EDGES)
    u, v = u[order], v[order]
    indptr, indices, eid, _, _ = O.csr_build(u, v, 4, m)
    og = O.CsrGraph(indptr, indices, eid=eid, n_src=4)
    ogt = og.transpose()
    assert tuple(np.diff(ogt.indptr)) == DEG and ogt.n_src == m
    assert sorted(ogt.eid) == sorted(ogt.nidx) == list(range(N_EDGES))
    assert list(ogt.eid) != list(range(N_EDGES)) and list(ogt.nidx) != list(range(N_EDGES))
    assert set(ogt.indices[ogt.indptr[2]:ogt.indptr[3]]) == set(range(m))
    return og, ogt


def _views(ogt, sources, n_src, dev):
    """(the view on the table as it lies, the view on the m gathered rows packed)"""
    from stag_amd.graph import CsrView
    src = np.asarray(sources, np.int64)
    indptr, eid, nidx = (_dev(a, dev) for a in (ogt.indptr, ogt.eid, ogt.nidx))
    views = (CsrView(4, n_src, indptr, _dev(src[ogt.indices].astype(np.int32), dev), eid=eid, nidx=nidx),
             CsrView(4, len(sources), indptr, _dev(ogt.indices, dev), eid=eid, nidx=nidx))
    for v in views:
        plan = v.plan(16, need=True)
        assert plan["n_seg"] >= 3 and plan["n_long"] == 1, "the hub is cut into three segments"
    return views


class _Checker:
    def __init__(self, what):
        self.what, self.errs = what, []

    def __call__(self, name, got_table, got_packed, refs):
        """got_*: the outputs of one launch on either layout; refs: (oracle value, scale) per output"""
        for i, (gt, gp, (ref, sc)) in enumerate(zip(got_table, got_packed, refs)):
            what = f"{self.what} {name}[{i}]"
            if not torch.equal(gt, gp):
                self.errs.append(f"{what}: not the bits of the packed layout (max |diff| {float((gt - gp).abs().max()):.3e})")
            try:
                assert_close(gt.detach().cpu().numpy() / sc, np.asarray(ref, np.float64) / sc, what=what)
            except AssertionError as e:
                self.errs.append(str(e))


def _sc(ref):
    return max(1.0, float(np.abs(ref).max()))


def _fp32_cases(O, dev, og, ogt, D, xt, xp, sst, ssp, views, check, rng):
    """Every fp32 entry point at width D.  xt / xp: the table view [n_src, D] and the packed rows [m, D]; sst / ssp: the
    source-side scale over the table's rows and packed."""
    from stag_amd import ops
    E = N_EDGES
    xn, ssn = xp.cpu().numpy(), ssp.cpu().numpy()
    ds = rng.uniform(0.5, 1.5, 4).astype(np.float32)
    own = rng.standard_normal((4, D)).astype(np.float32)             # the rows the units own (the backward's x)
    dsd, ownd = _dev(ds, dev), _dev(own, dev)
    w = rng.standard_normal((E, D)).astype(np.float32)
    e0, e1 = rng.uniform(0.2, 1.2, (E, 1)).astype(np.float32), rng.uniform(-1.0, 0.0, (E, 1)).astype(np.float32)
    q0, q1 = rng.uniform(0.2, 1.2, (E, D)).astype(np.float32), rng.uniform(0.3, 0.9, (E, D)).astype(np.float32)
    c0, c1 = rng.uniform(0.2, 1.0, D).astype(np.float32), rng.uniform(0.3, 0.9, D).astype(np.float32)
    w1 = rng.standard_normal((E, 1)).astype(np.float32)
    mk = lambda kind, p0=None, p1=None, **kw: _Spec(O, dev, kind, p0, p1, D=D, n_edges=E, **kw)
    layouts = ((views[0], xt, sst), (views[1], xp, ssp))

    def both(name, launch, refs):
        for seg in SEGS:
            check(f"D={D} {name} seg_len={seg}", *(launch(v, x, ss, seg) for v, x, ss in layouts), refs)

    fwd = lambda sp: O.agg_fwd(ogt, xn, sp, src_scale=ssn, dst_scale=ds)
    # ---- stag_agg_fwd ------------------------------------------------------------------------------------------------
    for name, sp in (("none", mk("none")), ("explicit [E,D]", mk("explicit", w)),
                     ("scalar Normal relu", mk("normal", 1.0, 0.5, relu=True)),
                     ("scalar Uniform in-norm", mk("uniform", 0.5, 1.5, in_norm=True)),
                     ("[E,1] Normal p1_log", mk("normal", e0, e1, p1_log=True)), ("[E,D] Normal", mk("normal", q0, q1))):
        ref = fwd(sp.o())
        both(f"stag_agg_fwd {name}", lambda v, x, ss, seg, sp=sp: [ops._agg_raw(v, x, D, sp.c, 0, ss, dsd, seg)[0]],
             [(ref, 1.0)])
    # ---- stag_agg_fwd_mc: S = 3, offset stride 3 ----------------------------------------------------------------------
    sp = mk("normal", 1.0, 0.5)
    ref = O.agg_fwd_mc(ogt, xn, sp.o(), 3, offset_stride=3, src_scale=ssn, dst_scale=ds)
    both("stag_agg_fwd_mc", lambda v, x, ss, seg: [ops._agg_fwd_mc_raw(v, x, _Noise(sp.c), 3, 3, 0, ss, dsd, seg)], [(ref, 1.0)])
    # ---- the backward entry points: the table is g, the view the source-major one ------------------------------------
    sp = mk("normal", c0, c1, relu=True)
    T = [O.agg_fwd(ogt, xn, sp.o(deriv=dv), src_scale=ssn, dst_scale=ds) for dv in (0, 1, 2)]
    both("stag_agg_bwd", lambda v, x, ss, seg: list(ops._agg_bwd_raw(v, x, D, sp.c, ss, dsd, seg, True)), [(t, 1.0) for t in T])
    dp = [(own.astype(np.float64) * t.astype(np.float64)).sum(0) for t in T[1:]]
    both("stag_agg_bwd_dp", lambda v, x, ss, seg: list(ops._agg_bwd_dp_raw(v, x, ownd, D, sp.c, ss, dsd, seg)),
         [(T[0], 1.0)] + [(r, _sc(r)) for r in dp])
    sp = mk("normal", e0, np.exp(e1))
    eg = [O.agg_bwd_w(og, own, xn * ssn[:, None], src_scale=ds, spec=sp.o(deriv=dv)).astype(np.float64).sum(1, keepdims=True)
          for dv in (1, 2)]
    both("stag_agg_bwd_edge", lambda v, x, ss, seg: list(ops._agg_bwd_edge_raw(v, x, ownd, D, sp.c, ss, dsd, seg)),
         [(fwd(sp.o()), 1.0)] + [(r, _sc(r)) for r in eg])
    # ---- stag_agg_fwd_w1: an explicit w[E], and a Normal of width 1 ---------------------------------------------------
    wide1 = lambda w1: fwd(O.make_spec("explicit", p0=np.ascontiguousarray(np.repeat(w1, D, 1))))
    sp = _Spec(O, dev, "explicit", w1)
    both("stag_agg_fwd_w1 explicit", lambda v, x, ss, seg: [ops._agg_w1_raw(v, x, D, sp.c, 0, ss, dsd, seg)], [(wide1(w1), 1.0)])
    sp1 = _Spec(O, dev, "normal", 1.0, 0.5, D=1, n_edges=E)
    both("stag_agg_fwd_w1 Normal dn=1", lambda v, x, ss, seg: [ops._agg_w1_raw(v, x, D, sp1.c, 0, ss, dsd, seg)],
         [(wide1(O.noise_materialize(ogt, sp1.o(), 1)), 1.0)])
    # ---- stag_agg_fwd_mc_edge / _pedge: S = 7, passes of 4, 2 and 1 ---------------------------------------------------
    for name, raw, sp in (("stag_agg_fwd_mc_edge", ops._agg_fwd_mc_edge_raw, mk("normal", e0, e1, p1_log=True)),
                          ("stag_agg_fwd_mc_pedge", ops._agg_fwd_mc_pedge_raw, mk("normal", q0, q1))):
        ref = O.agg_fwd_mc(ogt, xn, sp.o(), 7, offset_stride=2, src_scale=ssn, dst_scale=ds)
        both(name, lambda v, x, ss, seg, raw=raw, sp=sp: [raw(v, x, _Noise(sp.c), 7, 2, 0, ss, dsd, seg)], [(ref, 1.0)])


def _table(n_rows, ld, dtype, dev):
    """n_rows rows of ld elements, random everywhere, as one flat buffer"""
    return torch.empty(n_rows * ld, dtype=dtype, device=dev).normal_()


@pytest.mark.parametrize("form", list(FORMS))
def test_every_entry_point_in_each_form(dev, oracle, form):
    """stag_agg_fwd (none, explicit [E, D], scalar Normal with relu, scalar Uniform with in-norm, [E, 1] Normal with a
    log-scale, [E, D] Normal), stag_agg_fwd_mc, stag_agg_bwd with the derivative aggregates, stag_agg_bwd_dp,
    stag_agg_bwd_edge with its eg0[eid] / eg1[eid] stores, stag_agg_fwd_w1, stag_agg_fwd_mc_edge, stag_agg_fwd_mc_pedge at
    two widths, and stag_agg_fwd_half on bf16 and fp16 rows — each with seg_len 0 and 16 (unit walk | segment partials and
    the merge or combine kernels), on the table of this form and on its gathered rows packed."""
    from stag_amd import ops
    f = FORMS[form]
    n_src, src = f["n_src"], torch.tensor(f["sources"], device=dev)
    og, ogt = _structure(oracle, len(f["sources"]), seed=ord(form))
    views = _views(ogt, f["sources"], n_src, dev)
    check = _Checker(f"form ({form})")
    rng = np.random.default_rng(ord(form))
    ds = rng.uniform(0.5, 1.5, 4).astype(np.float32)
    dsd = _dev(ds, dev)
    sst = 0.5 + torch.rand(n_src, device=dev)
    ssp = sst[src].contiguous()
    with hw_normals(oracle, dev):
        ld = f["stride_bytes"] // 4
        flat = _table(n_src, ld, torch.float32, dev)
        for D in f["widths"]:
            xt = flat.as_strided((n_src, D), (ld, 1))
            assert xt.stride(0) * 4 == f["stride_bytes"] and xt.data_ptr() % 16 == 0
            xp = xt[src].contiguous()
            _fp32_cases(oracle, dev, og, ogt, D, xt, xp, sst, ssp, views, check, rng)
        del flat, xt
        ld = f["stride_bytes"] // 2
        sp = _Spec(oracle, dev, "normal", 1.0, 0.5, D=HALF_D, n_edges=N_EDGES)
        for dtype in (torch.bfloat16, torch.float16):
            flat = _table(n_src, ld, dtype, dev)
            xt = flat.as_strided((n_src, HALF_D), (ld, 1))
            xp = xt[src].contiguous()
            ref = oracle.agg_fwd(ogt, xp.float().cpu().numpy(), sp.o(), src_scale=ssp.cpu().numpy(), dst_scale=ds)
            for seg in SEGS:
                check(f"stag_agg_fwd_half {dtype} seg_len={seg}",
                      [ops._agg_half_raw(views[0], xt, HALF_D, sp.c, 0, sst, dsd, seg)],
                      [ops._agg_half_raw(views[1], xp, HALF_D, sp.c, 0, ssp, dsd, seg)], [(ref, 1.0)])
            del flat, xt
    assert not check.errs, "\n".join(check.errs)


# ---- a row stride of 2^32 bytes ----------------------------------------------------------------------------------------
def test_rows_2_32_bytes_apart(dev, oracle):
    """Three rows 2^30 floats apart in a buffer that is otherwise untouched.  The kernels take the stride as 32 bits of
    bytes, so the entry point refuses it (it used to truncate it to 0: every source then read row 0); ops.aggregate packs
    the rows and must give the oracle's sums."""
    import stag_amd
    from stag_amd import _lib, ops
    D, ld = 8, 1 << 30
    flat = torch.empty(2 * ld + D, device=dev)
    x = flat.as_strided((3, D), (ld, 1))
    vals = torch.randn(3, D, device=dev)
    x.copy_(vals)
    src, dst = torch.tensor([0, 1, 2, 2, 1, 0, 1]), torch.tensor([0, 0, 0, 1, 1, 2, 2])
    g = stag_amd.Graph(src, dst, 3, device=dev)
    noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=7, offset=3)
    og = oracle.CsrGraph(g.csr.indptr.cpu().numpy(), g.csr.indices.cpu().numpy(), g.csr.eid.cpu().numpy(), n_src=3)
    with hw_normals(oracle, dev):
        ref = oracle.agg_fwd(og, vals.cpu().numpy(), oracle.make_spec("normal", 1.0, 0.5, seed=7, offset=3, Dn=D, n_edges=7))
        ref0 = oracle.agg_fwd(og, vals.cpu().numpy(), oracle.make_spec("none"))
    with torch.no_grad():
        assert_close(ops.aggregate(g, x, noise), ref, what="rows 2^32 bytes apart, Normal")
        assert_close(ops.aggregate(g, x), ref0, what="rows 2^32 bytes apart, plain sum")
    x.requires_grad_(True)                    # the autograd route packs it too
    assert x.stride(0) == ld
    assert_close(ops.aggregate(g, x, noise), ref, what="rows 2^32 bytes apart, with an autograd node")
    x = x.detach()
    spec = ops._targs_or_c(ops._noise_spec(noise))
    for seg in SEGS:
        with pytest.raises(_lib.StagHipError, match="rc=-38"):
            ops._agg_raw(g.csr, x, D, spec, 0, None, None, seg)
        with pytest.raises(_lib.StagHipError, match="rc=-38"):
            ops._agg_bwd_raw(g.csr_t, x, D, spec, None, None, seg, True)


# ---- per-edge tables: CSR positions and edge ids past 2^24, [E, D] parameter tables past 2^32 bytes ------------------------
def _pe_graph(dev):
    """E = 2^24 + 64 positions over PE_N_DST rows, built on the device without a sort: random columns, eid and nidx two
    affine permutations of the positions.  Checked rows (host): the first, the last, the one that holds position 2^24 and
    rows that hold edge ids on both sides of 2^24."""
    from stag_amd.graph import CsrView
    E = PE_EDGES
    indptr_h = (np.arange(PE_N_DST + 1, dtype=np.int64) * E // PE_N_DST).astype(np.int32)
    pos = torch.arange(E, device=dev, dtype=torch.int64)
    eid = ((pos * PE_A1 + PE_B1) % E).to(torch.int32)
    nidx = ((pos * PE_A2 + PE_B2) % E).to(torch.int32)
    indices = torch.randint(0, PE_N_SRC, (E,), device=dev, dtype=torch.int32)
    del pos
    view = CsrView(PE_N_DST, PE_N_SRC, _dev(indptr_h, dev), indices, eid=eid, nidx=nidx)
    row_of = lambda p: int(np.searchsorted(indptr_h, p, side="right") - 1)
    inv = pow(PE_A1, -1, E)
    high = [row_of(((i - PE_B1) * inv) % E) for i in range(K24, K24 + 64)]      # the rows of the 64 ids past 2^24
    rows = [0, PE_N_DST - 1]
    for r in [row_of(K24)] + high:
        if r not in rows and len(rows) < 12:
            rows.append(r)
    rows = np.array(sorted(rows))
    return view, indptr_h, rows


def _pe_compact(O, view, indptr_h, rows):
    """The oracle's graph of the checked rows — nidx = the original nidx, edge ids relabelled 0..k-1 in position order —
    its positions in the whole graph and the original edge ids of its edges."""
    pos = np.concatenate([np.arange(indptr_h[r], indptr_h[r + 1]) for r in rows])
    pos_d = torch.from_numpy(pos).to(view.indices.device)
    indptr = np.concatenate([[0], np.cumsum(indptr_h[rows + 1] - indptr_h[rows])]).astype(np.int32)
    eid = view.eid[pos_d].cpu().numpy().astype(np.int64)
    og = O.CsrGraph(indptr, view.indices[pos_d].cpu().numpy(), eid=np.arange(len(pos), dtype=np.int32),
                    nidx=view.nidx[pos_d].cpu().numpy(), n_src=PE_N_SRC)
    return og, pos, eid


def _oracle_cond(O, og, xn, ssn, dsn, spec=None, W=None):
    """(the oracle's sums for a spec or for explicit weights W by edge id, sum |terms| of each sum): the rows of this graph
    add some 2000 terms of both signs each, so their comparisons take util.assert_close_cond, as the sweeps of
    test_gpu_parity.py do."""
    if W is None:
        W = O.noise_materialize(og, spec, xn.shape[1])
    else:
        spec = O.make_spec("explicit", p0=np.ascontiguousarray(W))
    ref = O.agg_fwd(og, xn, spec, src_scale=ssn, dst_scale=dsn)
    ab = O.agg_fwd(og, np.abs(xn), O.make_spec("explicit", p0=np.ascontiguousarray(np.abs(W))), src_scale=ssn, dst_scale=dsn)
    return ref, ab


def _rest(n, rows, dev):
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[torch.from_numpy(rows).to(dev)] = False
    return keep


def test_per_edge_tables_past_2_24_ids(dev, oracle):
    """D = 4: [E, 1] and [E, 4] tables below 2^32 bytes, read at edge ids and CSR positions on both sides of 2^24 (wide
    bit 1 of agg_common; the plan-order clients index them in 64 bits).  stag_agg_fwd_w1, stag_agg_fwd_mc_edge,
    stag_agg_bwd_edge (dx and eg0 / eg1 at the checked rows' edge ids), stag_agg_fwd with [E, 1] and [E, 4] parameters and
    stag_agg_fwd_mc_pedge against the oracle on the checked rows; every other row against stag_agg_fwd on materialised
    weights, device to device, at the bar tests/test_gpu_large.py holds that comparison to (5 TOL)."""
    from stag_amd import _lib, ops
    E, D, SEG = PE_EDGES, 4, 64
    view, indptr_h, rows = _pe_graph(dev)
    og, pos, ids = _pe_compact(oracle, view, indptr_h, rows)
    rows_d, ids_d = torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev)
    # what the rows were chosen for
    assert rows[0] == 0 and rows[-1] == PE_N_DST - 1 and len(rows) >= 10
    assert any(indptr_h[r] <= K24 < indptr_h[r + 1] for r in rows) and pos.max() == E - 1 and (pos >= K24).sum() >= 64
    per_row = np.split(ids, np.cumsum(np.diff(og.indptr))[:-1])
    assert sum(1 for r in per_row if r.min() < K24 <= r.max()) >= 8, "rows with edge ids on both sides of 2^24"
    assert (ids >= K24).sum() >= 8 and sorted(set(ids)) == sorted(ids)
    assert int(view.eid.max()) == E - 1 and int(view.nidx.max()) == E - 1
    rest = _rest(PE_N_DST, rows, dev)
    x = torch.randn(PE_N_SRC, D, device=dev)
    own = torch.randn(PE_N_DST, D, device=dev)
    ss, ds = 0.5 + torch.rand(PE_N_SRC, device=dev), 0.5 + torch.rand(PE_N_DST, device=dev)
    xn, ssn, dsn, ownn = x.cpu().numpy(), ss.cpu().numpy(), ds[rows_d].cpu().numpy(), own[rows_d].cpu().numpy()
    e0, e1 = 0.2 + torch.rand(E, 1, device=dev), 0.3 + 0.6 * torch.rand(E, 1, device=dev)
    q0, q1 = 0.2 + torch.rand(E, D, device=dev), 0.3 + 0.6 * torch.rand(E, D, device=dev)
    w1 = torch.randn(E, 1, device=dev)
    gather = lambda t: t[ids_d].cpu().numpy()

    def cspec(kind, mode, p0, p1):
        s = _lib.NoiseSpec()
        s.kind, s.param_mode, s.p0, s.p1, s.seed, s.offset = kind, mode, _lib.ptr(p0), _lib.ptr(p1), SEED, OFFSET
        return s

    def ospec(p0, p1, Dn, **kw):
        return oracle.make_spec("normal", gather(p0), gather(p1), seed=SEED, Dn=Dn, n_edges=len(ids), **{"offset": OFFSET, **kw})

    def explicit(w):          # stag_agg_fwd on materialised weights: the reference of the rows the oracle does not walk
        s = _lib.NoiseSpec()
        s.kind, s.p0 = _lib.NOISE_EXPLICIT, _lib.ptr(w)
        return ops._agg_raw(view, x, D, s, 0, ss, ds, SEG)[0]

    def materialised(spec, Dn):
        import ctypes as C
        w = torch.empty(E, Dn, device=dev)
        cs = view.struct()
        with _lib.on_device(dev):
            _lib.check(_lib.lib().stag_noise_materialize(C.byref(cs), None, C.byref(spec), Dn, _lib.ptr(w), Dn, None,
                                                         _lib.stream_of(dev)), "stag_noise_materialize")
        return w.expand(E, D).contiguous() if Dn != D else w

    cond = lambda **kw: _oracle_cond(oracle, og, xn, ssn, dsn, **kw)
    with hw_normals(oracle, dev):
        # stag_agg_fwd_w1, explicit w[E]
        got = ops._agg_w1_raw(view, x, D, cspec(_lib.NOISE_EXPLICIT, 0, w1, None), 0, ss, ds, SEG)
        assert_close_cond(got[rows_d], *cond(W=np.repeat(gather(w1), D, 1)), what="stag_agg_fwd_w1 explicit, checked rows")
        assert_close(got[rest], explicit(w1.expand(E, D).contiguous())[rest].cpu().numpy(), tol=5 * TOL, what="stag_agg_fwd_w1 explicit, the rest")
        # [E, 1] Normal: stag_agg_fwd, stag_agg_fwd_mc_edge (sample s = stag_agg_fwd at offset + 2 s), stag_agg_bwd_edge
        sp1 = cspec(_lib.NOISE_NORMAL, _lib.PARAM_PER_EDGE1, e0, e1)
        got = ops._agg_raw(view, x, D, sp1, 0, ss, ds, SEG)[0]
        assert_close_cond(got[rows_d], *cond(spec=ospec(e0, e1, D)), what="stag_agg_fwd [E,1], checked rows")
        mat = explicit(materialised(sp1, D))
        assert_close(got[rest], mat[rest].cpu().numpy(), tol=5 * TOL, what="stag_agg_fwd [E,1], the rest")
        mc = ops._agg_fwd_mc_edge_raw(view, x, _Noise(sp1), 7, 2, 0, ss, ds, SEG)
        for s in range(7):
            assert_close_cond(mc[s][rows_d], *cond(spec=ospec(e0, e1, D, offset=OFFSET + 2 * s)),
                              what=f"stag_agg_fwd_mc_edge sample {s}, checked rows")
        sp1.offset = OFFSET + 12
        assert_close(mc[6][rest], ops._agg_raw(view, x, D, sp1, 0, ss, ds, SEG)[0][rest].cpu().numpy(), tol=5 * TOL,
                     what="stag_agg_fwd_mc_edge sample 6, the rest")
        sp1.offset = OFFSET
        dx, g0, g1 = ops._agg_bwd_edge_raw(view, x, own, D, sp1, ss, ds, SEG)
        assert_close_cond(dx[rows_d], *cond(spec=ospec(e0, e1, D)), what="stag_agg_bwd_edge dx, checked rows")
        assert_close(dx[rest], got[rest].cpu().numpy(), tol=5 * TOL, what="stag_agg_bwd_edge dx vs stag_agg_fwd, the rest")
        # the oracle's per-edge sums want the transpose of the checked rows: rows = table rows, columns = checked rows,
        # drawn at the same positions (nidx) and read at the same relabelled ids
        k = len(ids)
        u = np.repeat(np.arange(len(rows)), np.diff(og.indptr))
        ip, ix, eid_f, _, _ = oracle.csr_build(u, og.indices, len(rows), PE_N_SRC)
        ogf = oracle.CsrGraph(ip, ix, eid=eid_f, nidx=og.nidx[eid_f], n_src=len(rows))
        for dv, gi in ((1, g0), (2, g1)):
            ref = oracle.agg_bwd_w(ogf, ownn, xn * ssn[:, None], src_scale=dsn, spec=ospec(e0, e1, D, deriv=dv))
            ref = ref.astype(np.float64).sum(1, keepdims=True)
            assert ref.shape == (k, 1)
            assert_close(gi[ids_d] / _sc(ref), ref / _sc(ref), what=f"stag_agg_bwd_edge d p{dv - 1}, checked rows' edge ids")
        # ... and every other edge id: the same sums from the materialised derivative, device to device
        v_of = view.indices.long()
        u_of = torch.repeat_interleave(torch.arange(PE_N_DST, device=dev), view.degrees.long())
        eid_l = view.eid.long()
        term = (x[v_of] * ss[v_of, None]).double() * (own[u_of] * ds[u_of, None]).double()
        for dv, gi in ((1, g0), (2, g1)):
            sp1.deriv = dv
            dw = materialised(sp1, D)
            sp1.deriv = 0
            all_ids = torch.zeros(E, 1, device=dev, dtype=torch.float64)
            all_ids[eid_l] = (dw[eid_l].double() * term).sum(1, keepdim=True)
            sc = max(1.0, float(all_ids.abs().max()))
            assert_close(gi / sc, (all_ids / sc).cpu().numpy(), tol=5 * TOL, what=f"stag_agg_bwd_edge d p{dv - 1}, every edge id")
        del term, all_ids, dw, v_of, u_of, eid_l, mat
        # stag_agg_fwd_w1, Normal of width 1 with [E, 1] parameters
        got = ops._agg_w1_raw(view, x, D, sp1, 0, ss, ds, SEG)
        wref = oracle.noise_materialize(og, ospec(e0, e1, 1), 1)
        assert_close_cond(got[rows_d], *cond(W=np.repeat(wref, D, 1)), what="stag_agg_fwd_w1 Normal dn=1, checked rows")
        assert_close(got[rest], explicit(materialised(sp1, 1))[rest].cpu().numpy(), tol=5 * TOL, what="stag_agg_fwd_w1 Normal dn=1, the rest")
        # [E, 4] Normal: stag_agg_fwd and stag_agg_fwd_mc_pedge
        sp = cspec(_lib.NOISE_NORMAL, _lib.PARAM_PER_EDGE, q0, q1)
        got = ops._agg_raw(view, x, D, sp, 0, ss, ds, SEG)[0]
        assert_close_cond(got[rows_d], *cond(spec=ospec(q0, q1, D)), what="stag_agg_fwd [E,D], checked rows")
        assert_close(got[rest], explicit(materialised(sp, D))[rest].cpu().numpy(), tol=5 * TOL, what="stag_agg_fwd [E,D], the rest")
        mc = ops._agg_fwd_mc_pedge_raw(view, x, _Noise(sp), 7, 2, 0, ss, ds, SEG)
        for s in range(7):
            assert_close_cond(mc[s][rows_d], *cond(spec=ospec(q0, q1, D, offset=OFFSET + 2 * s)),
                              what=f"stag_agg_fwd_mc_pedge sample {s}, checked rows")
        sp.offset = OFFSET + 12
        assert_close(mc[6][rest], ops._agg_raw(view, x, D, sp, 0, ss, ds, SEG)[0][rest].cpu().numpy(), tol=5 * TOL,
                     what="stag_agg_fwd_mc_pedge sample 6, the rest")


def test_per_edge_tables_past_2_32_bytes(dev, oracle):
    """D = 64: the [E, 64] parameter tables are 4.3 GB each.  stag_agg_fwd and stag_agg_fwd_mc_pedge against the oracle on the
    checked rows, and the documented equalities on every row: sample s of stag_agg_fwd_mc_pedge is stag_agg_fwd at offset
    + s * stride (at the oracle bar), and constant parameter rows give stag_agg_fwd_mc_edge's samples bit for bit.
    The oracle bar here is util.assert_close_cond's: a row adds some 2097 terms of both signs, the two kernels add the
    same weights (bit for bit) in different orders, and over 8000 x 64 sums the plain bar read up to 1.70e-05 (seven samples) for one that
    cancels (the checked rows: 5.1e-06 against the oracle).  sum |terms| of every sum comes from the kernel itself: two
    launches under relu on |x|, with the parameters and with their negatives, checked against the oracle's on the
    checked rows."""
    from stag_amd import _lib, ops
    E, D, SEG, S, STRIDE = PE_EDGES, 64, 64, 7, 2
    assert E * D * 4 >= 1 << 32
    view, indptr_h, rows = _pe_graph(dev)
    og, pos, ids = _pe_compact(oracle, view, indptr_h, rows)
    rows_d, ids_d = torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev)
    x = torch.randn(PE_N_SRC, D, device=dev)
    ss, ds = 0.5 + torch.rand(PE_N_SRC, device=dev), 0.5 + torch.rand(PE_N_DST, device=dev)
    xn, ssn, dsn = x.cpu().numpy(), ss.cpu().numpy(), ds[rows_d].cpu().numpy()
    q0 = torch.empty(E, D, device=dev).uniform_(0.2, 1.2)
    q1 = torch.empty(E, D, device=dev).uniform_(0.3, 0.9)
    assert (ids >= K24).sum() >= 8 and int(ids.max()) * D * 4 >= 1 << 32, "parameter rows past 2^32 bytes are read"

    def cspec(mode, p0, p1, offset=OFFSET):
        s = _lib.NoiseSpec()
        s.kind, s.param_mode, s.p0, s.p1, s.seed, s.offset = _lib.NOISE_NORMAL, mode, _lib.ptr(p0), _lib.ptr(p1), SEED, offset
        return s

    def abs_terms(offset):
        """sum |w| |ss x| ds of every (row, channel) at this offset without an [E, D] tensor: two launches under relu, on
        the weights and on their negatives (p0 + p1 z negates exactly with its parameters)"""
        sp = cspec(_lib.PARAM_PER_EDGE, q0, q1, offset)
        sp.relu = 1
        out = ops._agg_raw(view, x.abs(), D, sp, 0, ss, ds, SEG)[0]
        q0.neg_(), q1.neg_()
        out += ops._agg_raw(view, x.abs(), D, sp, 0, ss, ds, SEG)[0]
        q0.neg_(), q1.neg_()
        return out.cpu().numpy()

    p0n, p1n = q0[ids_d].cpu().numpy(), q1[ids_d].cpu().numpy()
    mc = ops._agg_fwd_mc_pedge_raw(view, x, _Noise(cspec(_lib.PARAM_PER_EDGE, q0, q1)), S, STRIDE, 0, ss, ds, SEG)
    with hw_normals(oracle, dev):
        for s in range(S):
            off = OFFSET + s * STRIDE
            osp = oracle.make_spec("normal", p0n, p1n, seed=SEED, offset=off, Dn=D, n_edges=len(ids))
            ref, ab = _oracle_cond(oracle, og, xn, ssn, dsn, spec=osp)
            assert_close_cond(mc[s][rows_d], ref, ab, what=f"stag_agg_fwd_mc_pedge D=64 sample {s}, checked rows")
            one = ops._agg_raw(view, x, D, cspec(_lib.PARAM_PER_EDGE, q0, q1, off), 0, ss, ds, SEG)[0]
            assert_close_cond(one[rows_d], ref, ab, what=f"stag_agg_fwd [E,D] D=64 at offset {off}, checked rows")
            every = abs_terms(off)
            assert_close(every[rows], ab, tol=5 * TOL, what="sum |terms| from the two relu launches vs the oracle's")
            assert_close_cond(mc[s], one.cpu().numpy(), every,
                              what=f"stag_agg_fwd_mc_pedge sample {s} vs stag_agg_fwd at its offset, every row")
    del mc, one
    # constant rows: the [E, 1] tables broadcast into the same two buffers
    e0, e1 = 0.2 + torch.rand(E, 1, device=dev), 0.3 + 0.6 * torch.rand(E, 1, device=dev)
    q0.copy_(e0.expand(E, D))
    q1.copy_(e1.expand(E, D))
    mc = ops._agg_fwd_mc_pedge_raw(view, x, _Noise(cspec(_lib.PARAM_PER_EDGE, q0, q1)), S, STRIDE, 0, ss, ds, SEG)
    del q0, q1
    edge = ops._agg_fwd_mc_edge_raw(view, x, _Noise(cspec(_lib.PARAM_PER_EDGE1, e0, e1)), S, STRIDE, 0, ss, ds, SEG)
    assert torch.equal(mc, edge), "constant parameter rows: stag_agg_fwd_mc_edge's samples, bit for bit"
