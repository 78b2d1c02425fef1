"""One weight per edge, shared by all channels (noise width 1 on rows of width D > 1; an explicit [E] / [E, 1] weight):
stag_agg_fwd_w1 and the routes of ops.aggregate around it, against the CPU oracle.  The oracle needs no form of its own:
w1 = noise_materialize(spec, Dn = 1), then agg_fwd with explicit weights np.repeat(w1, D, 1).  Bars: util.TOL, the bar
of every fp32 aggregation here (the sums are Kahan-compensated past 16 edges; the hub row has 1100); gradients relative
to max(1, max |ref|)."""
import numpy as np
import pytest
import torch

from util import TOL, assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
SEG = 64


@pytest.fixture(scope="module")
def graph_a(dev):
    """A hub row of 18 segments (more than one group of 16), multi-edges, a node without in-edges."""
    g = random_graph(67, 400, seed=11, hub=1100, device=dev)
    plan = g.csr.plan(SEG, need=True)
    seg = plan["long_seg_ptr"].cpu().numpy()
    assert int(np.diff(seg).max()) >= 18
    assert int(g.csr.degrees.min()) == 0
    return g


@pytest.fixture(scope="module")
def graph_c(dev):
    return random_graph(300, 600, seed=12, device=dev)


@pytest.fixture(autouse=True)
def _fused(monkeypatch):
    """These tests are about the fused launch whatever the shipped default of the switch is."""
    from stag_amd import ops
    monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", True)
    monkeypatch.setattr(ops, "EDGE_WEIGHT_TENSORS", True)


def _kinds(E, dev, seed=0):
    """name -> (kind, p0, p1, relu, p1_log): python floats, or [E, 1] device tensors."""
    gen = torch.Generator().manual_seed(77 + seed)
    loc = (0.2 + torch.rand(E, 1, generator=gen)).to(dev)
    ls = (-1.0 + torch.rand(E, 1, generator=gen)).to(dev)
    return {
        "normal": ("normal", 1.0, 0.5, False, False),
        "normal_edge_log": ("normal", loc, ls, False, True),
        "uniform": ("uniform", -0.5, 1.5, False, False),
        "bernoulli": ("bernoulli", 0.5, None, False, False),
        "relu_normal": ("normal", 0.0, 1.0, True, False),
    }


def _noise(g, kind, p0, p1, relu, p1_log, **kw):
    import stag_amd
    from stag_amd import _lib
    k = {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM, "bernoulli": _lib.NOISE_BERNOULLI}[kind]
    return stag_amd.EdgeNoise(g, 1, k, p0, p1, relu=relu, p1_log=p1_log, **kw)


def _np(p):
    return p.detach().cpu().numpy() if torch.is_tensor(p) else p


def _ow1(O, og, E, kind, p0, p1, relu, p1_log, **kw):
    """The oracle's [E, 1] weights of a width-1 spec (by edge id)."""
    spec = O.make_spec(kind, _np(p0), _np(p1), relu=relu, p1_log=p1_log, Dn=1, n_edges=E, **kw)
    return O.noise_materialize(og, spec, 1)


def _oref(O, og, x, w1, reduce="sum", ss=None, ds=None):
    D = x.shape[1]
    if og.n_edges == 0:
        return np.zeros((og.n_dst, D), np.float32)
    spec = O.make_spec("explicit", p0=np.ascontiguousarray(np.repeat(w1, D, 1)))
    return O.agg_fwd(og, x, spec, reduce=O.REDUCE_MEAN if reduce == "mean" else O.REDUCE_SUM, src_scale=ss, dst_scale=ds)


def _raw(csrv, x, noise=None, w=None, reduce="sum", ss=None, ds=None, seg_len=SEG):
    """The entry point itself."""
    from stag_amd import ops
    spec = ops._targs_or_c(ops._noise_spec(noise)) if noise is not None else ops._targs_or_c(ops._explicit_spec(w))
    return ops._agg_w1_raw(csrv, x, x.shape[1], spec, ops._REDUCE[reduce], ss, ds, seg_len)


# ---- 1. values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 4, 7, 20, 128, 260])
def test_values_against_the_oracle(dev, oracle, graph_a, D):
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    og = oracle_graph(oracle, g)
    x = torch.randn(n, D, device=dev)
    xn = x.cpu().numpy()
    rng = np.random.default_rng(D)
    ss, ds = (rng.uniform(0.5, 1.5, n).astype(np.float32) for _ in range(2))
    ssd, dsd = torch.from_numpy(ss).to(dev), torch.from_numpy(ds).to(dev)
    epoch = torch.full((1,), 5, dtype=torch.int64, device=dev)
    with hw_normals(oracle, dev):
        for name, (kind, p0, p1, relu, plog) in _kinds(E, dev).items():
            for pos_base, ep in ((0, None), ((7 << 32) + 12345, epoch)):
                noise = _noise(g, kind, p0, p1, relu, plog, seed=21, offset=3, pos_base=pos_base, epoch=ep)
                w1 = _ow1(oracle, og, E, kind, p0, p1, relu, plog, seed=21, offset=3 + (5 if ep is not None else 0),
                          pos_base=pos_base)
                for reduce in ("sum", "mean"):
                    got = _raw(g.csr, x, noise, reduce=reduce, ss=ssd, ds=dsd)
                    assert_close(got, _oref(oracle, og, xn, w1, reduce, ss, ds), what=f"{name} D={D} {reduce} pos={pos_base}")
                if pos_base == 0:
                    assert_close(_raw(g.csr, x, noise), _oref(oracle, og, xn, w1), what=f"{name} D={D} unscaled")
    wt = torch.randn(E, 1, device=dev)
    wt[::3] = 0.0                                                                   # explicit zeros are skipped
    for reduce in ("sum", "mean"):
        got = _raw(g.csr, x, w=wt, reduce=reduce, ss=ssd, ds=dsd)
        assert_close(got, _oref(oracle, og, xn, wt.cpu().numpy(), reduce, ss, ds), what=f"explicit D={D} {reduce}")


def test_device_scalars_and_padded_rows(dev, oracle, graph_a):
    """Parameters that live on the device travel as one-element rows (PER_CHANNEL); x may have a padded row stride and
    start at an address that is no multiple of 16 (the scalar row form)."""
    from stag_amd import _lib
    g = graph_a
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 12
    og = oracle_graph(oracle, g)
    big = torch.randn(n, 20, device=dev)
    p0, p1 = torch.tensor(0.8, device=dev), torch.tensor(0.4, device=dev)
    noise = _noise(g, "normal", p0, p1, False, False, seed=4, offset=9)
    assert noise.param_mode == _lib.PARAM_PER_CHANNEL and noise.p0.shape == (1,)
    with hw_normals(oracle, dev):
        w1 = _ow1(oracle, og, E, "normal", 0.8, 0.4, False, False, seed=4, offset=9)
    for x in (big[:, :D], big[:, 1:D + 1], big[:, 4:4 + D]):
        assert_close(_raw(g.csr, x, noise), _oref(oracle, og, x.contiguous().cpu().numpy(), w1), what=f"offset {x.storage_offset()}")


def test_no_edges_and_one_edge(dev, oracle):
    for e in (0, 1):
        g = random_graph(5, e, seed=3, device=dev)
        og = oracle_graph(oracle, g)
        x = torch.randn(5, 20, device=dev)
        noise = _noise(g, "uniform", 0.5, 1.5, False, False, seed=2, offset=1)
        w1 = _ow1(oracle, og, e, "uniform", 0.5, 1.5, False, False, seed=2, offset=1)
        for csrv in (g.csr,):
            got = _raw(csrv, x, noise, reduce="mean")
            assert_close(got, _oref(oracle, og, x.cpu().numpy(), w1, "mean"), what=f"{e} edges")
        from stag_amd import ops
        assert_close(ops.aggregate(g, x, noise), _oref(oracle, og, x.cpu().numpy(), w1), what=f"{e} edges, ops")


# ---- 2. Bernoulli counts, exactly ----------------------------------------------------------------------------------------
def test_bernoulli_counts_are_exact_forward_and_transposed(dev, oracle, graph_a):
    from stag_amd import ops
    g = graph_a
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 20
    og = oracle_graph(oracle, g)
    noise = _noise(g, "bernoulli", 0.5, None, False, False, seed=8, offset=2)
    w1 = _ow1(oracle, og, E, "bernoulli", 0.5, None, False, False, seed=8, offset=2)[:, 0]
    assert 0.3 < w1.mean() < 0.7
    src, dst = (t.cpu().numpy() for t in g.edges())
    kept_in = np.bincount(dst, weights=w1, minlength=n)
    kept_out = np.bincount(src, weights=w1, minlength=n)
    x = torch.ones(n, D, device=dev, requires_grad=True)
    out = ops.aggregate(g, x, noise)
    assert np.array_equal(out.detach().cpu().numpy(), np.repeat(kept_in[:, None], D, 1).astype(np.float32))
    out.backward(torch.ones_like(out))                                     # dx of g = 1: csr_t with nidx
    assert np.array_equal(x.grad.cpu().numpy(), np.repeat(kept_out[:, None], D, 1).astype(np.float32))


# ---- 3. the skip rule ------------------------------------------------------------------------------------------------
def test_a_zero_weight_does_not_read_its_row(dev, oracle, graph_a, graph_c):
    g = graph_a
    x = torch.full((g.number_of_nodes(), 20), float("nan"), device=dev)
    out = _raw(g.csr, x, _noise(g, "bernoulli", 0.0, None, False, False, seed=1, offset=1), reduce="mean")
    assert torch.equal(out, torch.zeros_like(out)) and not torch.signbit(out).any()
    out = _raw(g.csr, x, w=torch.zeros(g.number_of_edges(), 1, device=dev))
    assert torch.equal(out, torch.zeros_like(out))
    out = _raw(g.csr, x, _noise(g, "normal", -50.0, 1.0, True, False, seed=1, offset=1))    # relu'd: all non-positive
    assert torch.equal(out, torch.zeros_like(out))

    g = graph_c
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 20
    og = oracle_graph(oracle, g)
    noise = _noise(g, "bernoulli", 0.2, None, False, False, seed=31, offset=6)
    w1 = _ow1(oracle, og, E, "bernoulli", 0.2, None, False, False, seed=31, offset=6)
    src = g.edges()[0].cpu().numpy()
    kept_out = np.bincount(src, weights=w1[:, 0], minlength=n)
    dead = np.nonzero((kept_out == 0) & (np.bincount(src, minlength=n) > 0))[0]     # every out-edge dropped
    assert len(dead) >= 5
    xn = np.random.default_rng(0).standard_normal((n, D)).astype(np.float32)
    xz = xn.copy()
    xz[dead] = 0.0
    xn[dead] = np.nan
    for reduce in ("sum", "mean"):
        got = _raw(g.csr, torch.from_numpy(xn).to(dev), noise, reduce=reduce)
        assert torch.isfinite(got).all()
        assert_close(got, _oref(oracle, og, xz, w1, reduce), what=f"rows never read, {reduce}")


# ---- 4. gradients ------------------------------------------------------------------------------------------------------
def _rel(got, ref, what):
    ref = np.asarray(ref, np.float64)
    sc = max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    assert_close(got.detach().cpu().numpy() / sc, ref / sc, what=what)


def test_dx_against_the_oracle_on_the_transposed_view(dev, oracle, graph_a):
    from stag_amd import ops
    g = graph_a
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 20
    og, ogt = oracle_graph(oracle, g), oracle_graph(oracle, g, transposed=True)
    rng = np.random.default_rng(4)
    ss, ds = (rng.uniform(0.5, 1.5, n).astype(np.float32) for _ in range(2))
    ssd, dsd = torch.from_numpy(ss).to(dev), torch.from_numpy(ds).to(dev)
    G = torch.randn(n, D, device=dev)
    with hw_normals(oracle, dev):
        for name, (kind, p0, p1, relu, plog) in _kinds(E, dev).items():
            noise = _noise(g, kind, p0, p1, relu, plog, seed=13, offset=4)
            w1 = _ow1(oracle, og, E, kind, p0, p1, relu, plog, seed=13, offset=4)
            for reduce in ("sum", "mean"):
                x = torch.randn(n, D, device=dev, requires_grad=True)
                ops.aggregate(g, x, noise, reduce=reduce, src_scale=ssd, dst_scale=dsd).backward(G)
                dvec = ds / np.maximum(g.csr.degrees.cpu().numpy(), 1) if reduce == "mean" else ds
                # dx[u] = ss[u] sum_{p: src_p = u} w1[p] dvec[v_p] G[v_p]: the forward on the transposed view
                ref = _oref(oracle, ogt, G.cpu().numpy(), w1, "sum", dvec.astype(np.float32), ss)
                _rel(x.grad, ref, f"dx {name} {reduce}")


def _composed(graph, x, w1, **kw):
    """The composed torch route: the [E, 1] sample expanded to [E, D] into the per-channel aggregation (ops._Aggregate)."""
    from stag_amd import ops
    return ops.aggregate(graph, x, w1.expand(w1.shape[0], x.shape[1]), **kw)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_dw_and_live_parameter_gradients_against_the_composed_route(dev, graph_a, reduce):
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_a
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 20
    ss, ds = torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) + 0.5
    G = torch.randn(n, D, device=dev)
    x0, w0 = torch.randn(n, D, device=dev), torch.randn(E, 1, device=dev)
    grads = []
    for route in (lambda x, w: ops.aggregate(g, x, w, reduce=reduce, src_scale=ss, dst_scale=ds),
                  lambda x, w: ops.aggregate(g, x, w[:, 0], reduce=reduce, src_scale=ss, dst_scale=ds),
                  lambda x, w: _composed(g, x, w, reduce=reduce, src_scale=ss, dst_scale=ds)):
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        route(x, w).backward(G)
        assert w.grad.shape == (E, 1)
        grads.append((x.grad, w.grad))
    for i in (0, 1):
        _rel(grads[i][0], grads[2][0].cpu().numpy(), f"dx, explicit w, route {i}")
        _rel(grads[i][1], grads[2][1].cpu().numpy(), f"dw [E, 1], route {i}")

    loc0, ls0 = torch.rand(E, 1, device=dev) + 0.5, torch.rand(E, 1, device=dev) - 1.0
    for in_norm in (False, True):
        res = []
        for composed in (False, True):
            loc, ls = loc0.clone().requires_grad_(True), ls0.clone().requires_grad_(True)
            x = x0.clone().requires_grad_(True)
            noise = stag_amd.EdgeNoise(g, 1, _lib.NOISE_NORMAL, loc, ls, p1_log=True, differentiable=True, in_norm=in_norm,
                                       seed=3, offset=17)
            if composed:
                out = _composed(g, x, noise.materialize(), reduce=reduce, src_scale=ss, dst_scale=ds)
            else:
                out = ops.aggregate(g, x, noise, reduce=reduce, src_scale=ss, dst_scale=ds)
            out.backward(G)
            res.append((out.detach(), x.grad, loc.grad, ls.grad))
        for got, ref, nm in zip(res[0], res[1], ("out", "dx", "d loc", "d log_scale")):
            _rel(got, ref.cpu().numpy(), f"vi in_norm={in_norm} {nm}")
        assert float(res[0][2].abs().max()) > 0 and float(res[0][3].abs().max()) > 0


# ---- 5. determinism and the routes ---------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_every_route_agrees(dev, graph_a, monkeypatch):
    from stag_amd import ops
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    ss, ds = torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) + 0.5
    for D in (20, 260):
        x = torch.randn(n, D, device=dev)
        weights = {name: _noise(g, *v, seed=6, offset=2) for name, v in _kinds(E, dev).items()}
        weights["explicit"] = torch.randn(E, 1, device=dev)
        for name, wt in weights.items():
            for reduce in ("sum", "mean"):
                kw = dict(reduce=reduce, src_scale=ss, dst_scale=ds)
                monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", True)
                a, b = ops.aggregate(g, x, wt, **kw), ops.aggregate(g, x, wt, **kw)
                assert torch.equal(a, b), f"{name} D={D}: two launches, different bits"
                monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", False)
                two = ops.aggregate(g, x, wt, **kw)
                assert_close(two, a.cpu().numpy(), what=f"{name} D={D} {reduce}: two-launch route")
                w1 = wt if torch.is_tensor(wt) else wt.materialize()
                assert w1.shape == (E, 1)
                assert_close(_composed(g, x, w1, **kw), a.cpu().numpy(), what=f"{name} D={D} {reduce}: expanded route")
                # the fused launch's weights are the materialised ones, bit for bit: the explicit launch on them is the same sum
                monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", True)
                assert torch.equal(ops.aggregate(g, x, w1, **kw), a), f"{name} D={D}: draw != materialize()"
    # a broadcast row takes the two-launch route, whatever the switch says
    row = torch.randn(1, 20, device=dev)
    wt = torch.randn(E, 1, device=dev)
    got = ops.aggregate(g, row, wt, _broadcast_x=True)
    ref = ops.aggregate(g, row.expand(n, 20).contiguous(), wt.expand(E, 20).contiguous())
    assert_close(got, ref.cpu().numpy(), what="broadcast row")


@pytest.mark.parametrize("kind", ["normal", "explicit"])
@pytest.mark.parametrize("D", [256, 16])
def test_merge_of_more_segments_than_one_round(dev, oracle, graph_a, D, kind):
    """seg_len = 4 cuts the hub row into at least 275 segments.  The merge (unit_sum.hpp's seg_merge at 4 channels a
    lane) adds them in groups of 16, one group per team and round, T = 256 / LPE teams: at D = 256 (LPE = 64, T = 4)
    a round takes 64 segments, so the hub needs five and ends on a partial group; at D = 16 (LPE = 4, T = 64) one."""
    g, seg_len = graph_a, 4
    n, E = g.number_of_nodes(), g.number_of_edges()
    T = 256 // max(4, min(64, D // 4))
    plan = g.csr.plan(seg_len, need=True)
    hub_segs = int(np.diff(plan["long_seg_ptr"].cpu().numpy()[:plan["n_long"] + 1]).max())
    assert hub_segs >= 275 and hub_segs % 16 != 0, "the last group of the hub row is partial"
    if D == 256:
        assert T == 4 and plan["n_seg"] > 16 * T and hub_segs > 4 * 16 * T, "five rounds"
    og = oracle_graph(oracle, g)
    x = torch.randn(n, D, device=dev)
    ds = np.random.default_rng(D).uniform(0.5, 1.5, n).astype(np.float32)
    dsd = torch.from_numpy(ds).to(dev)
    if kind == "explicit":
        wt = torch.randn(E, 1, device=dev)
        how, w1 = dict(w=wt), wt.cpu().numpy()
    else:
        v = _kinds(E, dev)[kind]
        how = dict(noise=_noise(g, *v, seed=8, offset=5))
        with hw_normals(oracle, dev):
            w1 = _ow1(oracle, og, E, *v, seed=8, offset=5)
    for reduce in ("sum", "mean"):
        got = _raw(g.csr, x, reduce=reduce, ds=dsd, seg_len=seg_len, **how)
        assert_close(got, _oref(oracle, og, x.cpu().numpy(), w1, reduce, None, ds), what=f"D={D} {kind} {reduce} seg_len=4")
        again = _raw(g.csr, x, reduce=reduce, ds=dsd, seg_len=seg_len, **how)
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)), "two launches, the same bits"
        whole = _raw(g.csr, x, reduce=reduce, ds=dsd, seg_len=0, **how)             # no plan: the hub row is one unit
        assert_close(got, whole.cpu().numpy(), what=f"D={D} {kind} {reduce} seg_len=4 against no plan")


def test_other_widths_keep_their_error(dev, graph_c):
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_c
    x = torch.randn(g.number_of_nodes(), 20, device=dev)
    for dn in (2, 5, 40):
        with pytest.raises(ValueError, match=f"noise width {dn} != feature width 20"):
            ops.aggregate(g, x, stag_amd.EdgeNoise(g, dn, _lib.NOISE_NORMAL, 1.0, 0.5))
    noise = _noise(g, "normal", 1.0, 0.5, False, False)
    noise.n_samples = 3
    with pytest.raises(ValueError, match="Monte-Carlo"):
        ops.aggregate(g, x, noise)


# ---- 6. layers -----------------------------------------------------------------------------------------------------------
def _base_layers():
    from stag_amd import zoo
    return {
        "gcn": lambda: zoo.GCN(20, 8),
        "sage_mean": lambda: zoo.GraphSAGE(20, 8, aggregator_type="mean"),
        "sage_pool": lambda: zoo.GraphSAGE(20, 8, aggregator_type="pool"),
        "gin": lambda: zoo.GIN(20, 8, "sum"),
    }


@pytest.mark.parametrize("q", ["normal", "bernoulli_norm"])
@pytest.mark.parametrize("base", ["gcn", "sage_mean", "sage_pool", "gin"])
def test_layer_with_sample_dimension_one(dev, graph_c, base, q):
    """(ValueError("noise width 1 != feature width 20") before this entry point existed.)"""
    import stag_amd
    g = graph_c
    feat = torch.randn(g.number_of_nodes(), 20, device=dev)
    kw = (dict(q_a=torch.distributions.Normal(1.0, 0.5)) if q == "normal"
          else dict(q_a=torch.distributions.Bernoulli(0.5), norm=True))
    layer = stag_amd.layers.StagLayer(_base_layers()[base](), **kw).to(dev)
    layer.base_layer.sample_dimension = 1
    stag_amd.manual_seed(99)
    with torch.no_grad():
        out = layer(g, feat)
        w = layer._edge_weight_sample
        assert w.shape == (g.number_of_edges(), 1)
        if q != "normal":
            assert float((w == 0).float().mean()) > 0.2
        ref = layer.base_layer(g, feat, edge_weight=w)
    assert torch.isfinite(out).all()
    assert_close(out, ref.cpu().numpy(), what=f"{base} {q}")
    assert layer.forward_mc(g, feat, 3) is None                            # no batched form at width 1: the caller loops
    # and under autograd (x = h carries a gradient wherever the layer transforms before it aggregates)
    stag_amd.manual_seed(99)
    out2 = layer(g, feat)
    assert_close(out2, out.cpu().numpy(), what=f"{base} {q} under autograd")
    out2.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in layer.base_layer.parameters())


@pytest.mark.parametrize("q", ["normal", "bernoulli_norm"])
def test_gated_gcn_with_a_descriptor_of_width_one(dev, graph_c, q):
    """GatedGCN takes its input as `h`: it is handed the descriptor directly, as its own tests hand it one."""
    import stag_amd
    g = graph_c
    feat = torch.randn(g.number_of_nodes(), 20, device=dev)
    layer = stag_amd.zoo.GatedGCN(20, 20, dropout=0.0).to(dev)
    noise = (_noise(g, "normal", 1.0, 0.5, False, False, seed=3, offset=8) if q == "normal"
             else _noise(g, "bernoulli", 0.5, None, False, False, in_norm=True, seed=3, offset=8))
    with torch.no_grad():
        out = layer(g, feat, edge_weight=noise)
        ref = layer(g, feat, edge_weight=noise.materialize())
    assert_close(out, ref.cpu().numpy(), what=f"gated gcn {q}")
    h = feat.clone().requires_grad_(True)
    layer(g, h, edge_weight=noise).square().mean().backward()              # (with an edge weight B is not on the path)
    assert torch.isfinite(h.grad).all() and float(h.grad.abs().max()) > 0
    assert all(torch.isfinite(p.grad).all() for p in layer.A.parameters())


def test_amortized_width_one_reaches_the_mlp(dev, graph_c, monkeypatch):
    import stag_amd
    from stag_amd import ops, zoo
    g = graph_c
    feat = torch.randn(g.number_of_nodes(), 20, device=dev)
    torch.manual_seed(5)
    layer = stag_amd.layers.StagLayer(zoo.GCN(20, 8), q_a=stag_amd.distributions.AmortizedDistribution(20, 1), vi=True).to(dev)
    layer.base_layer.sample_dimension = 1

    def grads():
        stag_amd.manual_seed(41)
        layer.zero_grad(set_to_none=True)
        out = layer(g, feat)
        (out.square().mean() + layer.kl_divergence()).backward()
        return out.detach(), {k: p.grad.clone() for k, p in layer.named_parameters()}
    out, got = grads()
    assert isinstance(layer._edge_weight_handle, stag_amd.EdgeNoise) and layer._edge_weight_handle.dn == 1

    def composed(graph, x, noise, w, reduce, src_scale, dst_scale, seg_len, broadcast_x):
        w1 = noise.materialize() if noise is not None else w
        return ops.aggregate(graph, x, w1.expand(w1.shape[0], x.shape[1]), reduce=reduce, src_scale=src_scale,
                             dst_scale=dst_scale, seg_len=seg_len)
    monkeypatch.setattr(ops, "_aggregate_w1", composed)
    out_c, ref = grads()
    assert_close(out, out_c.cpu().numpy(), what="amortised forward")
    mlp = [k for k in got if k.startswith("q_a.")]
    assert mlp and set(got) == set(ref)
    for k in got:
        _rel(got[k], ref[k].cpu().numpy(), f"d {k}")
    assert all(float(got[k].abs().max()) > 0 for k in mlp), "the loss reaches every parameter of the MLP"


# ---- 7. no [E, D] tensor ---------------------------------------------------------------------------------------------------
def test_no_edge_by_channel_tensor_is_allocated(dev, monkeypatch):
    from stag_amd import ops
    N, E, D = 2000, 32000, 64
    g = random_graph(N, E, seed=9, device=dev)
    x = torch.randn(N, D, device=dev)
    w = torch.rand(E, 1, device=dev)
    noise = _noise(g, "normal", 1.0, 0.5, False, False, seed=2, offset=2)
    bar = E * D * 4 // 2

    def rise(fn):
        fn()                                                               # plans, cached structure
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del keep
        return peak

    def train(weight):
        def fn():
            xg = x.clone().requires_grad_(True)
            ops.aggregate(g, xg, weight).square().sum().backward()
            return xg.grad
        return fn
    for fused in (True, False):
        monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", fused)
        with torch.no_grad():
            assert rise(lambda: ops.aggregate(g, x, w)) < bar, f"[E, 1] tensor, fused={fused}"
            assert rise(lambda: ops.aggregate(g, x, noise)) < bar, f"noise of width 1, fused={fused}"
        assert rise(train(noise)) < bar, f"noise of width 1, forward and backward, fused={fused}"
        assert rise(train(w)) < bar, f"[E, 1] tensor, forward and backward, fused={fused}"
    monkeypatch.setattr(ops, "EDGE_WEIGHT_TENSORS", False)                 # the expanded route does build it
    with torch.no_grad():
        assert rise(lambda: ops.aggregate(g, x, w)) >= 2 * bar
