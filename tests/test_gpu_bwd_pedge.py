"""dx and both [E, D] parameter gradients of one draw from ONE pass over the source-major CSR: stag_agg_bwd_pedge and the
two backward routes around it (ops._AggregateVI, the per-sample loop of ops._AggregateMCPEdge).  Values against the CPU
oracle under the device's normal tables (util.hw_normals) at util.TOL: dx against oracle.agg_bwd on the transposed view,
d p_i against oracle.agg_bwd_w with deriv = i + 1 on the scaled rows.  Bits against the two entries whose arithmetic it
restates: stag_agg_fwd_mc_pedge on csr_t at one sample (dx) and stag_agg_bwd_w_mc at one sample (d p0, d p1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import row_ladder_cases as rl
from test_gpu_mc_pedge import _kinds, _noise
from util import TOL, assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
SEG = 64
KAHAN_MIN_LEN = 16     # kKahanMinLen (csrc/agg_kernel.hpp)
COMBINE_GROUP = 16     # kCombineGroup: partials per merge group of a long row
KINDS = ("normal_log", "normal_scale", "uniform", "relu_normal")


def _reversed(g, dev):
    """The same edges, by edge id, with src and dst swapped."""
    import stag_amd
    src, dst = (t.cpu() for t in g.edges())
    return stag_amd.Graph(dst, src, g.number_of_nodes(), device=dev)


@pytest.fixture(scope="module")
def graph_a(dev):
    """test_gpu_mc_edge's graph A reversed: the hub is a SOURCE of more than 18 segments at seg_len 64 (more than one merge
    group), sources with more than kKahanMinLen out-edges, multi-edges, a node without out-edges."""
    g = _reversed(random_graph(67, 400, seed=11, hub=1100, device=dev), dev)
    plan = g.csr_t.plan(SEG, need=True)
    seg = np.diff(plan["long_seg_ptr"].cpu().numpy())
    assert int(seg.max()) >= 18 > COMBINE_GROUP
    out_deg = g.csr_t.degrees.cpu().numpy()
    assert int(out_deg.max()) >= 1100 > KAHAN_MIN_LEN and 1100 // int(seg.max()) > KAHAN_MIN_LEN   # (its segments are too)
    assert int(out_deg.min()) == 0, "a node without out-edges"
    src, dst = (t.cpu().numpy().astype(np.int64) for t in g.edges())
    assert len(np.unique(src * 67 + dst)) < len(src), "multi-edges"
    return g


@pytest.fixture(scope="module")
def graph_c(dev):
    return random_graph(300, 600, seed=12, device=dev)


@pytest.fixture(autouse=True)
def _fused(monkeypatch):
    """These tests are about the one-pass backward whatever the shipped default of the switches is; the Monte-Carlo node
    keeps its per-sample loop (the batched parameter call is test_gpu_mc_bwd's)."""
    from stag_amd import ops
    monkeypatch.setattr(ops, "PEDGE_BWD_FUSED", True)
    monkeypatch.setattr(ops, "PEDGE_BWD_MC_LOOP", True)
    monkeypatch.setattr(ops, "MC_PEDGE_FUSED", True)
    monkeypatch.setattr(ops, "MC_BWD_FUSED", False)


def _np(p):
    return p.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _call(g, G, x, noise, gs=None, rs=None, seg_len=SEG, want_dx=True, want_p1=True):
    """The entry point itself, through ops' raw helper: (dx, d p0, d p1)."""
    from stag_amd import ops
    return ops._agg_bwd_pedge_raw(g.csr_t, G, x, x.shape[1], noise.spec(), gs, rs, seg_len, want_dx, want_p1)


def _inputs(n, D, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=gen).to(dev)
    G = torch.randn(n, D, generator=gen).to(dev)
    gs = (0.5 + torch.rand(n, generator=gen)).to(dev)
    rs = (0.5 + torch.rand(n, generator=gen)).to(dev)
    return x, G, gs, rs


def _oref(O, g, xn, gn, kind, p0, p1, relu, p1_log, gs=None, rs=None, **kw):
    """(dx, d p0, d p1) of the oracle: agg_bwd on the transposed view, agg_bwd_w per derivative on the scaled rows."""
    E, D = g.number_of_edges(), xn.shape[1]
    mk = lambda deriv: O.make_spec(kind, _np(p0), _np(p1), relu=relu, p1_log=p1_log, Dn=D, n_edges=E, deriv=deriv, **kw)
    dx = O.agg_bwd(oracle_graph(O, g, transposed=True), gn, mk(0), gs, rs, want_dp=False)[0]
    og = oracle_graph(O, g)
    xs = xn if rs is None else xn * rs[:, None]
    gg = gn if gs is None else gn * gs[:, None]
    return dx, O.agg_bwd_w(og, xs, gg, spec=mk(1)), O.agg_bwd_w(og, xs, gg, spec=mk(2))


# ---- 1. values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 7, 20, 128, 260])
def test_values_against_the_oracle(dev, oracle, graph_a, D):
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, G, gsd, rsd = _inputs(n, D, dev, 100 + D)
    xn, gn, gs, rs = _np(x), _np(G), _np(gsd), _np(rsd)
    epoch = torch.full((1,), 5, dtype=torch.int64, device=dev)
    kinds = _kinds(E, D, dev)
    assert tuple(kinds) == KINDS
    with hw_normals(oracle, dev):
        for name, (kind, p0, p1, relu, plog) in kinds.items():
            for pos_base, ep in ((0, None), ((7 << 32) + 12345, epoch)):
                noise = _noise(g, D, kind, p0, p1, relu, plog, seed=21, offset=3, pos_base=pos_base, epoch=ep)
                off = 3 + (5 if ep is not None else 0)
                for scaled in (True, False):
                    sd, sn = ((gsd, rsd), (gs, rs)) if scaled else ((None, None), (None, None))
                    ref = _oref(oracle, g, xn, gn, kind, p0, p1, relu, plog, *sn, seed=21, offset=off, pos_base=pos_base)
                    for seg_len, tag in ((SEG, "plan"), (0, "no plan")):
                        got = _call(g, G, x, noise, *sd, seg_len=seg_len)
                        assert got[0].shape == (n, D) and got[1].shape == got[2].shape == (E, D)
                        for t, r, nm in zip(got, ref, ("dx", "d p0", "d p1")):
                            assert_close(t, r, what=f"{name} D={D} pos_base={pos_base} scaled={scaled} {tag} {nm}")


# ---- 2. bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "c"])
@pytest.mark.parametrize("D", [20, 7, 260])
def test_bits_are_those_of_the_two_entries_it_restates(dev, graph_a, graph_c, which, D):
    """dx: stag_agg_fwd_mc_pedge(csr_t, x = g, one sample, SUM, src_scale = g_scale, dst_scale = row_scale).
    d p0 / d p1: stag_agg_bwd_w_mc(csr, one sample, reduce_k = 0, src_scale = row_scale, the same g_scale)."""
    from stag_amd import _lib, ops
    g = graph_a if which == "a" else graph_c
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, G, gs, rs = _inputs(n, D, dev, 7 + D)
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
        noise = _noise(g, D, kind, p0, p1, relu, plog, seed=9, offset=11)
        for seg_len in (SEG, 0):
            for g_, r_ in ((gs, rs), (None, None)):
                what = f"graph {which} {name} D={D} seg_len={seg_len} scales={g_ is not None}"
                dx, d0, d1 = _call(g, G, x, noise, g_, r_, seg_len=seg_len)
                fwd = ops._agg_fwd_mc_pedge_raw(g.csr_t, G, noise, 1, 1, _lib.REDUCE_SUM, g_, r_, seg_len)
                _same_bits(dx, fwd[0], f"{what}: dx vs stag_agg_fwd_mc_pedge on csr_t")
                w0, w1 = ops._bwd_w_mc_raw(g.csr, x, G.unsqueeze(0), D, r_, g_, noise.spec(), 1, 1, reduce_k=False, seg_len=seg_len)
                _same_bits(d0, w0, f"{what}: d p0 vs stag_agg_bwd_w_mc")
                _same_bits(d1, w1, f"{what}: d p1 vs stag_agg_bwd_w_mc")


# ---- 3. outputs left out, repeatability ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [20, 260])
def test_outputs_left_out_and_two_runs(dev, graph_a, D):
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, G, gs, rs = _inputs(n, D, dev, 3 + D)
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
        noise = _noise(g, D, kind, p0, p1, relu, plog, seed=6, offset=2)
        a = _call(g, G, x, noise, gs, rs)
        b = _call(g, G, x, noise, gs, rs)
        for i, nm in enumerate(("dx", "d p0", "d p1")):
            _same_bits(a[i], b[i], f"{name} D={D}: two calls, different bits of {nm}")
        no_dx = _call(g, G, x, noise, gs, rs, want_dx=False)
        assert no_dx[0] is None
        _same_bits(no_dx[1], a[1], f"{name} D={D}: dx == NULL changed d p0")
        _same_bits(no_dx[2], a[2], f"{name} D={D}: dx == NULL changed d p1")
        no_p1 = _call(g, G, x, noise, gs, rs, want_p1=False)
        assert no_p1[2] is None
        _same_bits(no_p1[0], a[0], f"{name} D={D}: dp1 == NULL changed dx")
        _same_bits(no_p1[1], a[1], f"{name} D={D}: dp1 == NULL changed d p0")
        # the gradient rows are stored where the edge is walked: they do not depend on how the rows are cut
        for seg_len in (0, 4, 16):
            c = _call(g, G, x, noise, gs, rs, seg_len=seg_len)
            _same_bits(c[1], a[1], f"{name} D={D}: d p0 depends on seg_len {seg_len}")
            _same_bits(c[2], a[2], f"{name} D={D}: d p1 depends on seg_len {seg_len}")


# ---- 4. padded strides, pointers offset by 4 bytes ----------------------------------------------------------------------------
def _shifted(t):
    """The same values one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device)
    assert buf.data_ptr() % 16 == 0
    q = buf[1:].view(t.shape)
    q.copy_(t)
    assert q.data_ptr() % 16 == 4
    return q


def _padded(t, pad=3):
    """(buffer, view): the same rows D + pad floats apart, starting one float into the buffer; NaN around them."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=t.device)
    v = buf[:, 1:1 + t.shape[1]]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.stride(0) == t.shape[1] + pad
    return buf, v


@pytest.mark.parametrize("D", [20, 260])
def test_padded_strides_and_offset_pointers_give_the_same_bits(dev, graph_a, D):
    from stag_amd import _lib, ops
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, G, gs, rs = _inputs(n, D, dev, 5 + D)
    csrv = g.csr_t
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
        packed = _call(g, G, x, _noise(g, D, kind, p0, p1, relu, plog, seed=12, offset=5), gs, rs)
        assert x.data_ptr() % 16 == 0 and packed[1].data_ptr() % 16 == 0
        noise = _noise(g, D, kind, _shifted(p0), _shifted(p1), relu, plog, seed=12, offset=5)
        (_, Gv), (_, xv) = _padded(G), _padded(x)
        bufs = [torch.full((r, D + 3), float("nan"), device=dev) for r in (n, E, E)]
        outs = [b[:, 1:1 + D] for b in bufs]
        plan_t = csrv.plan(SEG)
        nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], D, 0)
        plan_c, _keep = ops._plan_struct(csrv, SEG, (D + 255) // 256, nbytes, dev, plan_t=plan_t)
        cs, spec = csrv.struct(), noise.spec()
        rc = _lib.lib().stag_agg_bwd_pedge(C.byref(cs), C.byref(plan_c), _lib.ptr(Gv), Gv.stride(0), D, C.byref(spec),
                                           _lib.ptr(gs), _lib.ptr(rs), _lib.ptr(xv), xv.stride(0), _lib.ptr(outs[0]), D + 3,
                                           _lib.ptr(outs[1]), _lib.ptr(outs[2]), D + 3, _lib.stream_of(dev))
        _lib.check(rc, "stag_agg_bwd_pedge")
        for i, nm in enumerate(("dx", "d p0", "d p1")):
            _same_bits(outs[i], packed[i], f"{name} D={D}: padded {nm}")
            assert bool(torch.isnan(bufs[i][:, 0]).all()) and bool(torch.isnan(bufs[i][:, 1 + D:]).all()), \
                f"{name} D={D}: the padding around {nm} was written"


# ---- 5. the row-length ladder -----------------------------------------------------------------------------------------------
def _ladder_check(oracle, dev, g, seg_lens, what):
    """Every source row of g at D = 8 against the oracle; a failure names the LENGTHS of the rows that differ."""
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 8
    rng = np.random.default_rng(1000 + E)
    f = np.float32
    xn, gn = rng.standard_normal((n, D)).astype(f), rng.standard_normal((n, D)).astype(f)
    gs, rs = rng.uniform(0.5, 1.5, n).astype(f), rng.uniform(0.5, 1.5, n).astype(f)
    q0, q1 = rng.uniform(0.2, 1.2, (E, D)).astype(f), rng.uniform(0.3, 0.9, (E, D)).astype(f)
    t = lambda a: torch.from_numpy(a).to(dev)
    p0, p1 = t(q0), t(q1)
    noise = _noise(g, D, "normal", p0, p1, False, False, seed=rl.SEED, offset=rl.OFFSET)
    with hw_normals(oracle, dev):
        ref = _oref(oracle, g, xn, gn, "normal", p0, p1, False, False, gs, rs, seed=rl.SEED, offset=rl.OFFSET)
    ct = g.csr_t
    out_deg = ct.degrees.cpu().numpy()
    len_of_eid = np.empty(E, np.int64)
    len_of_eid[ct.eid.cpu().numpy()] = np.repeat(out_deg, out_deg)
    bad = []
    for seg_len in seg_lens:
        got = _call(g, t(gn), t(xn), noise, t(gs), t(rs), seg_len=seg_len)
        for arr, r, lens, nm in ((got[0], ref[0], out_deg, "dx"), (got[1], ref[1], len_of_eid, "d p0"),
                                 (got[2], ref[2], len_of_eid, "d p1")):
            err = np.abs(_np(arr).astype(np.float64) - r) / (1.0 + np.abs(r))
            rows = np.flatnonzero(err.max(1) > TOL) if err.size else []
            if len(rows):
                bad.append(f"{what} seg_len={seg_len} {nm}: rows of length {sorted(set(int(lens[i]) for i in rows))}")
    assert not bad, bad
    return out_deg


def test_row_ladder_on_the_reversed_graph(dev, oracle):
    """tests/row_ladder_cases.py's graph with src and dst swapped: its destination-row lengths (0..40, 63..65, 68, 69,
    127..129, 132) are the SOURCE rows the pass walks."""
    import stag_amd
    st = rl.structure(oracle)
    g = stag_amd.Graph(torch.from_numpy(st.coo_dst), torch.from_numpy(st.coo_src), rl.N, device=dev)
    out_deg = _ladder_check(oracle, dev, g, rl.SEGS, "ladder")
    assert sorted(out_deg.tolist()) == sorted(rl.DEGREES)


def test_every_source_row_length_to_seventy(dev, oracle):
    """A source row of every length 0 .. 70 and of 126 .. 130 (around 2 * seg_len): every residue of the block of 4, the
    Kahan threshold, whole rows up to seg_len, rows cut in 2 and 3."""
    import stag_amd
    lengths = list(range(71)) + [126, 127, 128, 129, 130]
    rng = np.random.default_rng(70)
    n = len(lengths)
    order = rng.permutation(n)                                  # length and row id are unrelated
    deg = np.zeros(n, np.int64)
    deg[order] = lengths
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, len(src))
    perm = rng.permutation(len(src))                            # ... and so are edge id and position
    g = stag_amd.Graph(torch.from_numpy(src[perm]), torch.from_numpy(dst[perm]), n, device=dev)
    out_deg = _ladder_check(oracle, dev, g, (0, SEG, 4), "0..70")
    assert sorted(out_deg.tolist()) == sorted(lengths)


# ---- 6. degenerate graphs ----------------------------------------------------------------------------------------------
def test_no_edges_one_edge_and_one_source(dev, oracle):
    import stag_amd
    from stag_amd import _lib
    D = 20
    # no edges: the helper returns the zero rows; the entry point itself stores them (no per-edge array is read)
    g0 = random_graph(5, 0, seed=3, device=dev)
    x, G, gs, rs = _inputs(5, D, dev, 9)
    empty = torch.zeros(0, D, device=dev)
    noise = _noise(g0, D, "uniform", empty, empty, False, False, seed=2, offset=1)
    dx, d0, d1 = _call(g0, G, x, noise, gs, rs)
    assert d0.shape == d1.shape == (0, D) and torch.equal(dx, torch.zeros(5, D, device=dev))
    raw = torch.full((5, D), float("nan"), device=dev)
    dummy = torch.zeros(4, device=dev)
    cs, spec = g0.csr_t.struct(), noise.spec()
    rc = _lib.lib().stag_agg_bwd_pedge(C.byref(cs), None, _lib.ptr(G), D, D, C.byref(spec), _lib.ptr(gs), _lib.ptr(rs),
                                       _lib.ptr(x), D, _lib.ptr(raw), D, _lib.ptr(dummy), None, D, _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd_pedge")
    assert torch.equal(raw, torch.zeros(5, D, device=dev))
    # one edge; all edges from one source (one row of 200: four segments at seg_len 64)
    rng = np.random.default_rng(5)
    one = random_graph(5, 1, seed=3, device=dev)
    fan = stag_amd.Graph(torch.zeros(200, dtype=torch.int64), torch.from_numpy(rng.integers(0, 9, 200)), 9, device=dev)
    assert int(fan.csr_t.degrees.max()) == 200 and int((fan.csr_t.degrees > 0).sum()) == 1
    with hw_normals(oracle, dev):
        for g, tag in ((one, "one edge"), (fan, "one source")):
            n, E = g.number_of_nodes(), g.number_of_edges()
            x, G, gs, rs = _inputs(n, D, dev, 11 + E)
            for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
                noise = _noise(g, D, kind, p0, p1, relu, plog, seed=2, offset=1)
                ref = _oref(oracle, g, _np(x), _np(G), kind, p0, p1, relu, plog, _np(gs), _np(rs), seed=2, offset=1)
                for seg_len in (SEG, 0):
                    got = _call(g, G, x, noise, gs, rs, seg_len=seg_len)
                    for t, r, nm in zip(got, ref, ("dx", "d p0", "d p1")):
                        assert_close(t, r, what=f"{tag} {name} seg_len={seg_len} {nm}")


# ---- 7. autograd -----------------------------------------------------------------------------------------------------------
def _rel(got, ref, what):
    ref = np.asarray(ref, np.float64)
    sc = max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    assert_close(_np(got) / sc, ref / sc, what=what)


def _gcn_scales(g):
    """GCN's two degree scalings: out-degree^-1/2 on the source side, in-degree^-1/2 on the destination side."""
    ss = g.csr_t.degrees.clamp(min=1).to(torch.float32).pow(-0.5)
    ds = g.csr.degrees.clamp(min=1).to(torch.float32).pow(-0.5)
    return ss, ds


def _live(g, D, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    E = g.number_of_edges()
    return (torch.rand(E, D, generator=gen) + 0.5).to(dev), (torch.rand(E, D, generator=gen) - 1.0).to(dev)


@pytest.mark.parametrize("D", [20, 260])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("S", [1, 3])
def test_gradients_with_the_switch_on_and_off(dev, graph_a, monkeypatch, reduce, D, S):
    """ops.aggregate with live [E, D] loc / log_scale and an x that needs a gradient: the one-pass backward against
    stag_agg_bwd + g * dvec + stag_agg_bwd_w.  Both routes form the same products, so d loc and d log_scale have the same
    bits; dx (another summation order) at TOL relative to max(1, max |ref|).  S = 3: the per-sample loop of
    _AggregateMCPEdge."""
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    ss, ds = _gcn_scales(g)
    x0, _, _, _ = _inputs(n, D, dev, 31 + D)
    G = torch.randn((S, n, D) if S > 1 else (n, D), generator=torch.Generator().manual_seed(8)).to(dev)
    loc0, ls0 = _live(g, D, dev, 4)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "PEDGE_BWD_FUSED", fused)
        loc, ls = loc0.clone().requires_grad_(True), ls0.clone().requires_grad_(True)
        x = x0.clone().requires_grad_(True)
        noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, loc, ls, p1_log=True, differentiable=True, seed=3, offset=17)
        assert noise.param_mode == _lib.PARAM_PER_EDGE
        if S > 1:
            noise.n_samples, noise.offset_stride = S, 2
        out = ops.aggregate(g, x, noise, reduce=reduce, src_scale=ss, dst_scale=ds)
        assert ("_AggregateMCPEdge" if S > 1 else "_AggregateVI") in type(out.grad_fn).__name__
        out.backward(G)
        res.append((out.detach(), x.grad, loc.grad, ls.grad))
    assert torch.equal(res[0][0], res[1][0])
    _same_bits(res[0][2], res[1][2], f"{reduce} D={D} S={S}: d loc")
    _same_bits(res[0][3], res[1][3], f"{reduce} D={D} S={S}: d log_scale")
    _rel(res[0][1], _np(res[1][1]), f"{reduce} D={D} S={S} dx")
    assert res[0][2].shape == (E, D) and float(res[0][2].abs().max()) > 0 and float(res[0][3].abs().max()) > 0


def test_layer_step_with_the_switch_on_and_off(dev, graph_c, monkeypatch):
    """StagLayer(GCN(16, 8), AmortizedDistribution(16, 16), vi=True) on an input that needs a gradient."""
    import stag_amd
    from stag_amd import distributions, layers, ops, zoo
    g = graph_c
    n = g.number_of_nodes()
    gen = torch.Generator().manual_seed(2)
    feat0 = torch.randn(n, 16, generator=gen).to(dev)
    torch.manual_seed(5)
    layer = layers.StagLayer(zoo.GCN(16, 8), q_a=distributions.AmortizedDistribution(16, 16), vi=True).to(dev).train()
    calls = {"pedge": 0}
    real = ops._agg_bwd_pedge_raw

    def counted(*a, **kw):
        calls["pedge"] += 1
        return real(*a, **kw)
    monkeypatch.setattr(ops, "_agg_bwd_pedge_raw", counted)

    def grads(fused):
        monkeypatch.setattr(ops, "PEDGE_BWD_FUSED", fused)
        layer.zero_grad(set_to_none=True)
        stag_amd.manual_seed(41)
        feat = feat0.clone().requires_grad_(True)
        calls["pedge"] = 0
        out = layer(g, feat)
        (out.square().mean() + layer.kl_divergence()).backward()
        return out.detach(), feat.grad, {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}, calls["pedge"]
    out, dfeat, got, n_on = grads(True)
    out_ref, dfeat_ref, ref, n_off = grads(False)
    assert n_on == 1 and n_off == 0
    assert torch.equal(out, out_ref)
    assert set(got) == set(ref) and any(k.startswith("q_a.") for k in got)
    for k in got:
        if k.startswith("q_a."):        # behind d loc and d log_scale alone, whose bits the two routes share
            _same_bits(got[k], ref[k], f"d {k}")
        _rel(got[k], _np(ref[k]), f"d {k}")
    _rel(dfeat, _np(dfeat_ref), "d feat")


# ---- 8. routing ------------------------------------------------------------------------------------------------------------
class _Spy:
    """Counts the calls of every entry point of the library."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("stag_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_backward_routes(dev, graph_a, monkeypatch):
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_a
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 20
    ss, ds = _gcn_scales(g)
    x0, G, _, _ = _inputs(n, D, dev, 13)
    gen = torch.Generator().manual_seed(8)      # positive weights: in-norm divides by their row sums
    loc0, ls0 = (0.8 + 0.4 * torch.rand(E, D, generator=gen)).to(dev), (-3.0 + torch.rand(E, D, generator=gen)).to(dev)
    real = _lib.lib()
    g.csr.plan(ops.DEFAULT_SEG_LEN), g.csr_t.plan(ops.DEFAULT_SEG_LEN)
    monkeypatch.setattr(ops._torch_ext, "available", lambda: False)       # the ctypes binding is what the spy sees

    def run(in_norm=False, need_x=True, S=1):
        loc, ls = loc0.clone().requires_grad_(True), ls0.clone().requires_grad_(True)
        x = x0.clone().requires_grad_(need_x)
        noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, loc, ls, p1_log=True, differentiable=True, seed=3, offset=17,
                                   in_norm=in_norm)
        if S > 1:
            noise.n_samples, noise.offset_stride = S, 2
        out = ops.aggregate(g, x, noise, src_scale=ss, dst_scale=ds)
        assert ("_AggregateMCPEdge" if S > 1 else "_AggregateVI") in type(out.grad_fn).__name__
        spy = _Spy(real)
        monkeypatch.setattr(_lib, "_lib", spy)
        try:
            out.backward(G if S == 1 else G.unsqueeze(0).expand(S, n, D).contiguous())
        finally:
            monkeypatch.setattr(_lib, "_lib", real)
        assert loc.grad is not None and ls.grad is not None and (x.grad is not None) == need_x
        return {k: v for k, v in spy.calls.items() if k.startswith("stag_agg_")}

    assert run() == {"stag_agg_bwd_pedge": 1}
    calls = run(in_norm=True)
    assert "stag_agg_bwd_pedge" not in calls and calls.get("stag_agg_bwd", 0) == 1 and calls.get("stag_agg_bwd_w", 0) == 2
    assert run(need_x=False) == {"stag_agg_bwd_w": 1}
    # the per-sample loop of the Monte-Carlo node: one call per sample, or, with its own switch off, the old launches
    assert run(S=2) == {"stag_agg_bwd_pedge": 2}
    monkeypatch.setattr(ops, "PEDGE_BWD_MC_LOOP", False)
    assert run(S=2) == {"stag_agg_bwd": 2, "stag_agg_bwd_w": 2}
    assert run() == {"stag_agg_bwd_pedge": 1}
    monkeypatch.setattr(ops, "PEDGE_BWD_MC_LOOP", True)
    monkeypatch.setattr(ops, "PEDGE_BWD_FUSED", False)
    assert run() == {"stag_agg_bwd": 1, "stag_agg_bwd_w": 1}
    assert run(S=2) == {"stag_agg_bwd": 2, "stag_agg_bwd_w": 2}
