"""Monte-Carlo samples of amortised [E, D] edge noise from one pass over the rows and the parameter tables:
stag_agg_fwd_mc_pedge and the routes of ops.aggregate_mc / StagLayer.forward_mc / StagModel around it.  Values against
the CPU oracle, called per sample at offset + s * stride under the device's normal tables (util.hw_normals), at util.TOL
— the bar of every fp32 aggregation here (the sums are Kahan-compensated past 16 edges; the hub row has 1100); gradients
against the loop route, relative to max(1, max |ref|)."""
import copy

import numpy as np
import pytest
import torch

from util import TOL, assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
SEG = 64
KAHAN_MIN_LEN = 16     # kKahanMinLen (csrc/agg_kernel.hpp)


@pytest.fixture(scope="module")
def graph_a(dev):
    """A hub row of 18 segments (more than one merge group of 16), rows longer than kKahanMinLen, multi-edges, a node
    without in-edges."""
    g = random_graph(67, 400, seed=11, hub=1100, device=dev)
    plan = g.csr.plan(SEG, need=True)
    seg = plan["long_seg_ptr"].cpu().numpy()
    assert int(np.diff(seg).max()) >= 18
    deg = g.csr.degrees.cpu().numpy()
    assert int(deg.min()) == 0
    assert SEG > KAHAN_MIN_LEN and int(deg.max()) >= 1100
    src, dst = (t.cpu().numpy().astype(np.int64) for t in g.edges())
    assert len(np.unique(src * 67 + dst)) < len(src), "multi-edges"
    return g


@pytest.fixture(scope="module")
def graph_c(dev):
    return random_graph(300, 600, seed=12, device=dev)


@pytest.fixture(autouse=True)
def _fused(monkeypatch):
    """These tests are about the batched launch whatever the shipped default of the switches is."""
    from stag_amd import ops
    monkeypatch.setattr(ops, "MC_PEDGE_FUSED", True)
    monkeypatch.setattr(ops, "MC_EDGE_FUSED", True)


def _kinds(E, D, dev, seed=0):
    """name -> (kind, p0, p1, relu, p1_log) with [E, D] device tensors in the ranges of test_gpu_mc_edge._kinds, a
    different value per edge and channel."""
    gen = torch.Generator().manual_seed(77 + seed)
    loc = (0.2 + torch.rand(E, D, generator=gen)).to(dev)
    ls = (-1.0 + torch.rand(E, D, generator=gen)).to(dev)
    scale = (0.2 + torch.rand(E, D, generator=gen)).to(dev)
    low = (-0.5 * torch.rand(E, D, generator=gen)).to(dev)
    high = (1.0 + torch.rand(E, D, generator=gen)).to(dev)
    return {
        "normal_log": ("normal", loc, ls, False, True),
        "normal_scale": ("normal", loc, scale, False, False),
        "uniform": ("uniform", low, high, False, False),
        "relu_normal": ("normal", loc - 0.7, scale, True, False),
    }


def _noise(g, D, kind, p0, p1, relu, p1_log, **kw):
    import stag_amd
    from stag_amd import _lib
    k = {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM}[kind]
    n = stag_amd.EdgeNoise(g, D, k, p0, p1, relu=relu, p1_log=p1_log, **kw)
    if D == 1 or g.number_of_edges() <= 1:
        # the descriptor calls an [E, 1] table PER_EDGE1, and one edge's row SCALAR | PER_CHANNEL; the same memory is
        # the [E, D] table of this entry point
        assert tuple(p0.shape) == (g.number_of_edges(), D)
        n.param_mode = _lib.PARAM_PER_EDGE
        n.p0, n.p1 = p0.contiguous(), p1.contiguous()
    assert n.param_mode == _lib.PARAM_PER_EDGE
    return n


def _np(p):
    return p.detach().cpu().numpy()


def _oref(O, og, E, xn, kind, p0, p1, relu, p1_log, S, stride, offset, reduce="sum", ss=None, ds=None, **kw):
    """[S, n, D]: oracle.agg_fwd per sample at offset + s * stride."""
    D = xn.shape[1]
    outs = []
    for s in range(S):
        if og.n_edges == 0:
            outs.append(np.zeros((og.n_dst, D), np.float32))
            continue
        spec = O.make_spec(kind, _np(p0), _np(p1), relu=relu, p1_log=p1_log, Dn=D, n_edges=E, offset=offset + s * stride, **kw)
        outs.append(O.agg_fwd(og, xn, spec, reduce=O.REDUCE_MEAN if reduce == "mean" else O.REDUCE_SUM, src_scale=ss,
                              dst_scale=ds))
    return np.stack(outs, 0)


def _raw(csrv, x, noise, S, stride=1, reduce="sum", ss=None, ds=None, seg_len=SEG):
    """The entry point itself."""
    from stag_amd import ops
    return ops._agg_fwd_mc_pedge_raw(csrv, x, noise, S, stride, ops._REDUCE[reduce], ss, ds, seg_len)


# ---- 1. values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,S", [(1, 5), (7, 5), (20, 5), (128, 5), (260, 5), (20, 1), (20, 2), (20, 3), (20, 4), (20, 7)])
def test_values_against_the_oracle(dev, oracle, graph_a, D, S):
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
        for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
            for stride, pos_base, ep in ((1, 0, None), (3, (7 << 32) + 12345, epoch)):
                noise = _noise(g, D, kind, p0, p1, relu, plog, seed=21, offset=3, pos_base=pos_base, epoch=ep)
                off = 3 + (5 if ep is not None else 0)
                for reduce in ("sum", "mean"):
                    ref = _oref(oracle, og, E, xn, kind, p0, p1, relu, plog, S, stride, off, reduce, ss, ds, seed=21,
                                pos_base=pos_base)
                    got = _raw(g.csr, x, noise, S, stride, reduce, ssd, dsd)
                    assert got.shape == (S, n, D)
                    assert_close(got, ref, what=f"{name} D={D} S={S} {reduce} stride={stride} plan")
                    got = _raw(g.csr, x, noise, S, stride, reduce, ssd, dsd, seg_len=0)
                    assert_close(got, ref, what=f"{name} D={D} S={S} {reduce} stride={stride} no plan")
                if pos_base == 0 and name == "normal_log":
                    ref = _oref(oracle, og, E, xn, kind, p0, p1, relu, plog, S, stride, off, seed=21)
                    assert_close(_raw(g.csr, x, noise, S, stride), ref, what=f"{name} D={D} S={S} unscaled")


# ---- 2. the weights, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [20, 7, 260])
def test_weights_are_the_materialised_ones_bit_for_bit(dev, D):
    """Every node has exactly one in-edge, x is all ones, no scales: out_s[v, :] is the weight row of v's edge."""
    import stag_amd
    from stag_amd import ops
    n = 97
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n))
    g = stag_amd.Graph(perm, torch.arange(n), n, device=dev)
    E = g.number_of_edges()
    x = torch.ones(n, D, device=dev)
    dst = g.edges()[1].long()
    S, stride = 7, 3
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
        noise = _noise(g, D, kind, p0, p1, relu, plog, seed=9, offset=11)
        out = _raw(g.csr, x, noise, S, stride)
        for s in range(S):
            one = copy.copy(noise)
            one.offset = noise.offset + s * stride
            w = ops.materialize_noise(g, one)                      # [E, D] by edge id
            want = torch.empty_like(w)
            want[dst] = w
            assert torch.equal(out[s], want), f"{name} D={D} sample {s}"


# ---- 3. a sample does not depend on its pass -----------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_pass(dev, graph_a):
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    ss, ds = torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) + 0.5
    for D in (20, 260):
        x = torch.randn(n, D, device=dev)
        for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
            noise = _noise(g, D, kind, p0, p1, relu, plog, seed=6, offset=2)
            for reduce in ("sum", "mean"):
                a = _raw(g.csr, x, noise, 7, 2, reduce, ss, ds)
                b = _raw(g.csr, x, noise, 7, 2, reduce, ss, ds)
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} D={D}: two launches, different bits"
                for s in range(7):                                 # the passes of 7 samples carry more than one each
                    one = copy.copy(noise)
                    one.offset = noise.offset + 2 * s
                    alone = _raw(g.csr, x, one, 1, 2, reduce, ss, ds)
                    assert torch.equal(alone[0].view(torch.int32), a[s].view(torch.int32)), f"{name} D={D} {reduce} sample {s}"


# ---- 4. constant parameter rows: the [E, 1] family's sums and draws ---------------------------------------------------------
@pytest.mark.parametrize("D", [20, 260])
def test_constant_rows_equal_the_edge1_launch_bit_for_bit(dev, graph_a, D):
    """p[e, :] = q[e]: stag_agg_fwd_mc_edge on the [E, 1] tensors gives the same bits, plan or no plan."""
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_a
    n, E, S = g.number_of_nodes(), g.number_of_edges(), 7
    x = torch.randn(n, D, device=dev)
    ss, ds = torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) + 0.5
    for name, (kind, q0, q1, relu, plog) in _kinds(E, 1, dev).items():          # [E, 1] tensors
        wide = _noise(g, D, kind, q0.expand(E, D).contiguous(), q1.expand(E, D).contiguous(), relu, plog, seed=8, offset=4)
        narrow = stag_amd.EdgeNoise(g, D, {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM}[kind], q0, q1,
                                    relu=relu, p1_log=plog, seed=8, offset=4)
        assert narrow.param_mode == _lib.PARAM_PER_EDGE1
        for reduce in ("sum", "mean"):
            for seg_len in (SEG, 0):
                got = _raw(g.csr, x, wide, S, 3, reduce, ss, ds, seg_len=seg_len)
                ref = ops._agg_fwd_mc_edge_raw(g.csr, x, narrow, S, 3, ops._REDUCE[reduce], ss, ds, seg_len)
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{name} D={D} {reduce} seg_len={seg_len}"


# ---- 5. edge cases ---------------------------------------------------------------------------------------------------------
def test_no_edges_and_one_edge(dev, oracle):
    for e in (0, 1):
        g = random_graph(5, e, seed=3, device=dev)
        og = oracle_graph(oracle, g)
        x = torch.randn(5, 20, device=dev)
        p0 = torch.linspace(0.3, 0.6, 20, device=dev).repeat(e, 1)
        p1 = torch.linspace(1.2, 1.7, 20, device=dev).repeat(e, 1)
        noise = _noise(g, 20, "uniform", p0, p1, False, False, seed=2, offset=1)
        ref = _oref(oracle, og, e, x.cpu().numpy(), "uniform", p0, p1, False, False, 3, 1, 1, "mean", seed=2)
        assert_close(_raw(g.csr, x, noise, 3, reduce="mean"), ref, what=f"{e} edges")


def test_a_row_without_edges_is_exactly_zero(dev, graph_a):
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    empty = torch.nonzero(g.csr.degrees == 0).flatten()
    assert len(empty) >= 1
    x = torch.randn(n, 20, device=dev)
    ds = torch.rand(n, device=dev) + 0.5
    kind, p0, p1, relu, plog = _kinds(E, 20, dev)["normal_log"]
    noise = _noise(g, 20, kind, p0, p1, relu, plog, seed=1, offset=1)
    for reduce in ("sum", "mean"):
        out = _raw(g.csr, x, noise, 5, reduce=reduce, ds=ds)
        rows = out[:, empty]
        assert torch.equal(rows, torch.zeros_like(rows)), reduce


@pytest.mark.parametrize("D", [20, 260])
def test_a_table_at_four_byte_alignment_gives_the_same_bits(dev, graph_a, D):
    """Parameter tables that start one float past a 16-byte boundary take the scalar row forms."""
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    x = torch.randn(n, D, device=dev)
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D, dev).items():
        aligned = _noise(g, D, kind, p0, p1, relu, plog, seed=12, offset=5)
        assert aligned.p0.data_ptr() % 16 == 0 and aligned.p1.data_ptr() % 16 == 0
        shifted = []
        for p in (p0, p1):
            buf = torch.empty(E * D + 1, device=dev)
            assert buf.data_ptr() % 16 == 0
            q = buf[1:].view(E, D)
            q.copy_(p)
            shifted.append(q)
        off = _noise(g, D, kind, shifted[0], shifted[1], relu, plog, seed=12, offset=5)
        assert off.p0.data_ptr() % 16 == 4 and off.p1.data_ptr() % 16 == 4
        for seg_len in (SEG, 0):
            a = _raw(g.csr, x, aligned, 7, 2, "mean", seg_len=seg_len)
            b = _raw(g.csr, x, off, 7, 2, "mean", seg_len=seg_len)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} D={D} seg_len={seg_len}"


# ---- 6. routing ------------------------------------------------------------------------------------------------------------
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


def _spied(monkeypatch, fn):
    """(fn(), the library calls it made) with the ctypes binding in front of every entry point."""
    from stag_amd import _lib, ops
    real = _lib.lib()
    monkeypatch.setattr(ops._torch_ext, "available", lambda: False)       # the ctypes binding is what the spy sees
    spy = _Spy(real)
    monkeypatch.setattr(_lib, "_lib", spy)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(_lib, "_lib", real)
    return out, spy.calls


def test_aggregate_routes_per_edge_samples_to_the_batched_launch(dev, oracle, graph_a, monkeypatch):
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_a
    n, E, D = g.number_of_nodes(), g.number_of_edges(), 20
    og = oracle_graph(oracle, g)
    x = torch.randn(n, D, device=dev)
    xn = x.cpu().numpy()
    kind, p0, p1, relu, plog = _kinds(E, D, dev)["normal_log"]
    g.csr.plan(ops.DEFAULT_SEG_LEN)

    def run(S, p0, p1, in_norm=False, bernoulli=False):
        if bernoulli:
            noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_BERNOULLI, p0, None, seed=4, offset=7)
            assert noise.param_mode == _lib.PARAM_PER_EDGE
        else:
            noise = _noise(g, D, kind, p0, p1, relu, plog, seed=4, offset=7, in_norm=in_norm)
        noise.n_samples, noise.offset_stride = S, 2
        return _spied(monkeypatch, lambda: ops.aggregate(g, x, noise))

    with hw_normals(oracle, dev):
        for S in (4, 7):
            out, calls = run(S, p0, p1)
            assert out.shape == (S, n, D)
            # one call covers all passes: the entry point cuts them itself
            assert calls.get("stag_agg_fwd_mc_pedge", 0) == 1
            assert "stag_agg_fwd" not in calls and "stag_agg_fwd_mc" not in calls and "stag_agg_fwd_mc_edge" not in calls
            ref = _oref(oracle, og, E, xn, kind, p0, p1, relu, plog, S, 2, 7, seed=4)
            assert_close(out, ref, what=f"ops.aggregate S={S}")
        # the switch off: the loop
        monkeypatch.setattr(ops, "MC_PEDGE_FUSED", False)
        out, calls = run(4, p0, p1)
        assert "stag_agg_fwd_mc_pedge" not in calls and calls.get("stag_agg_fwd", 0) == 4
        ref = _oref(oracle, og, E, xn, kind, p0, p1, relu, plog, 4, 2, 7, seed=4)
        assert_close(out, ref, what="switch off")
        monkeypatch.setattr(ops, "MC_PEDGE_FUSED", True)
        # Bernoulli with per-edge probabilities: the loop
        probs = (0.2 + 0.6 * torch.rand(E, D, generator=torch.Generator().manual_seed(3))).to(dev)
        out, calls = run(3, probs, None, bernoulli=True)
        assert "stag_agg_fwd_mc_pedge" not in calls and calls.get("stag_agg_fwd", 0) == 3
        refs = [oracle.agg_fwd(og, xn, oracle.make_spec("bernoulli", _np(probs), None, Dn=D, n_edges=E, offset=7 + 2 * s, seed=4))
                for s in range(3)]
        assert_close(out, np.stack(refs, 0), what="Bernoulli takes the loop")
        # in-norm: the loop, to the same bar.  (The factor is indeg / sum_in(w): a bar relative to the output asks for
        # weight sums that do not cancel, so these weights are positive — loc in [0.8, 1.2], scale <= e^-2.)
        gen = torch.Generator().manual_seed(8)
        q0 = (0.8 + 0.4 * torch.rand(E, D, generator=gen)).to(dev)
        q1 = (-3.0 + torch.rand(E, D, generator=gen)).to(dev)
        out, calls = run(3, q0, q1, in_norm=True)
        assert "stag_agg_fwd_mc_pedge" not in calls and calls.get("stag_agg_fwd", 0) == 3
        ref = _oref(oracle, og, E, xn, kind, q0, q1, relu, plog, 3, 2, 7, seed=4, in_norm=True)
        assert_close(out, ref, what="in-norm takes the loop")


# ---- 7. gradients ----------------------------------------------------------------------------------------------------------
def _rel(got, ref, what):
    ref = np.asarray(ref, np.float64)
    sc = max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    assert_close(got.detach().cpu().numpy() / sc, ref / sc, what=what)


@pytest.mark.parametrize("D", [20, 260])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_gradients_against_the_loop(dev, graph_a, monkeypatch, reduce, D):
    """x, loc and log_scale live: dx from stag_agg_bwd on csr_t, both [E, D] gradients from one stag_agg_bwd_w call, per
    sample, as the loop's _AggregateVI runs them."""
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_a
    n, E, S = g.number_of_nodes(), g.number_of_edges(), 3
    ss, ds = torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) + 0.5
    G = torch.randn(S, n, D, device=dev)
    x0 = torch.randn(n, D, device=dev)
    loc0, ls0 = torch.rand(E, D, device=dev) + 0.5, torch.rand(E, D, device=dev) - 1.0
    res, fns = [], []
    for fused in (True, False):
        monkeypatch.setattr(ops, "MC_PEDGE_FUSED", fused)
        loc, ls = loc0.clone().requires_grad_(True), ls0.clone().requires_grad_(True)
        x = x0.clone().requires_grad_(True)
        noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, loc, ls, p1_log=True, differentiable=True, seed=3, offset=17)
        assert noise.param_mode == _lib.PARAM_PER_EDGE
        noise.n_samples, noise.offset_stride = S, 2
        out = ops.aggregate(g, x, noise, reduce=reduce, src_scale=ss, dst_scale=ds)
        fns.append(type(out.grad_fn).__name__)
        out.backward(G)
        res.append((out.detach(), x.grad, loc.grad, ls.grad))
    assert "_AggregateMCPEdge" in fns[0] and "_AggregateMCPEdge" not in fns[1]
    for got, ref, nm in zip(res[0], res[1], ("out", "dx", "d loc", "d log_scale")):
        assert got.shape == ref.shape
        _rel(got, ref.cpu().numpy(), f"{reduce} D={D} {nm}")
    assert res[0][2].shape == (E, D) and res[0][3].shape == (E, D)
    assert float(res[0][2].abs().max()) > 0 and float(res[0][3].abs().max()) > 0
    # x alone live (fixed noise on an input that carries a gradient)
    dxs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "MC_PEDGE_FUSED", fused)
        x = x0.clone().requires_grad_(True)
        noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, loc0, ls0, p1_log=True, seed=3, offset=17)
        noise.n_samples, noise.offset_stride = S, 2
        out = ops.aggregate(g, x, noise, reduce=reduce, src_scale=ss, dst_scale=ds)
        assert ("_AggregateMCPEdge" in type(out.grad_fn).__name__) == fused
        out.backward(G)
        dxs.append(x.grad)
    _rel(dxs[0], dxs[1].cpu().numpy(), f"{reduce} D={D} dx, fixed noise")


# ---- 8. model level --------------------------------------------------------------------------------------------------------
def _model(first_q_a, dev):
    """A model as the citation_* scripts build it: dropout in front of every stochastic layer."""
    from stag_amd import layers, models, zoo
    torch.manual_seed(5)
    return models.StagModel(torch.nn.ModuleList([
        layers.FeatOnlyLayer(torch.nn.Dropout(0.5)),
        layers.StagLayer(zoo.GCN(20, 12), q_a=first_q_a()),
        layers.FeatOnlyLayer(torch.nn.Dropout(0.5)),
        layers.StagLayer(zoo.GCN(12, 5), q_a=torch.distributions.Normal(1.0, 0.5)),
    ])).to(dev)


def _watch(monkeypatch, layer):
    seen = []
    orig = layer.forward_mc

    def spy(*a, **kw):
        r = orig(*a, **kw)
        seen.append(r)
        return r
    monkeypatch.setattr(layer, "forward_mc", spy)
    return seen


def test_model_batches_behind_a_leading_dropout(dev, graph_c, monkeypatch):
    import stag_amd
    from stag_amd import distributions
    g = graph_c
    feat = torch.randn(g.number_of_nodes(), 20, device=dev)
    model = _model(lambda: distributions.AmortizedDistribution(20, 20), dev).eval()
    first = model.layers[1]
    seen = _watch(monkeypatch, first)
    gen = first._generator()
    with torch.no_grad():
        stag_amd.manual_seed(31)
        out, calls = _spied(monkeypatch, lambda: model.forward(g, feat, n_samples=4, return_parameters=True))
        after = gen.offset
        assert len(seen) == 1 and seen[0] is not None and seen[0].shape == (4, g.number_of_nodes(), 12)
        assert calls.get("stag_agg_fwd_mc_pedge", 0) == 1
        assert not getattr(model, "_mc_batching_off", False)
        samples = []
        for s in range(4):
            first.mc_select(s)
            samples.append(first._edge_weight_sample.clone())
        model._mc_batching_off = True
        stag_amd.manual_seed(31)
        ref_samples = []
        hook = first.register_forward_hook(lambda m, i, o: ref_samples.append(m._edge_weight_sample.clone()))
        ref, calls = _spied(monkeypatch, lambda: model.forward(g, feat, n_samples=4, return_parameters=True))
        hook.remove()
        assert "stag_agg_fwd_mc_pedge" not in calls
        assert gen.offset == after, "the generator ends where the loop leaves it"
    assert len(seen) == 1
    assert_close(out, ref.cpu().numpy(), what="batched against the loop")
    assert len(ref_samples) == 4
    for s in range(4):
        assert samples[s].shape == (g.number_of_edges(), 20)
        assert torch.equal(samples[s], ref_samples[s]), f"mc_select({s}) names the loop's sample"


def test_model_with_live_dropout_keeps_the_loop(dev, graph_c, monkeypatch):
    import stag_amd
    from stag_amd import distributions
    g = graph_c
    feat = torch.randn(g.number_of_nodes(), 20, device=dev)
    model = _model(lambda: distributions.AmortizedDistribution(20, 20), dev).train()
    seen = _watch(monkeypatch, model.layers[1])
    with torch.no_grad():
        stag_amd.manual_seed(31)
        out, calls = _spied(monkeypatch, lambda: model.forward(g, feat, n_samples=4, return_parameters=True))
    assert seen == [] and "stag_agg_fwd_mc_pedge" not in calls
    assert out.shape == (g.number_of_nodes(), 5) and bool(torch.isfinite(out).all())


def test_training_through_the_batched_layer(dev, graph_c, monkeypatch):
    """model.loss(n_samples = 3) in train() with vi = True on the [E, D] amortised layer behind a Dropout(0) — the identity
    in training mode too: loss and every parameter gradient against the loop."""
    import stag_amd
    from stag_amd import distributions, layers, models, zoo
    g = graph_c
    n = g.number_of_nodes()
    feat = torch.randn(n, 20, device=dev)
    y = torch.randint(0, 5, (n,), device=dev)
    torch.manual_seed(5)
    model = models.StagModel(torch.nn.ModuleList([
        layers.FeatOnlyLayer(torch.nn.Dropout(0.0)),
        layers.StagLayer(zoo.GCN(20, 12), q_a=distributions.AmortizedDistribution(20, 20), vi=True),
        layers.StagLayer(zoo.GCN(12, 5, activation=torch.nn.Softmax(-1)), q_a=torch.distributions.Normal(1.0, 0.5)),
    ])).to(dev).train()
    seen = _watch(monkeypatch, model.layers[1])
    from stag_amd import ops
    launches, raw = [], ops._agg_fwd_mc_pedge_raw
    monkeypatch.setattr(ops, "_agg_fwd_mc_pedge_raw", lambda *a, **kw: (launches.append(1), raw(*a, **kw))[1])

    def grads(off):
        model._mc_batching_off = off
        model.zero_grad(set_to_none=True)
        stag_amd.manual_seed(41)
        loss = model.loss(g, feat, y, n_samples=3)
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    loss, got = grads(False)
    assert len(seen) == 1 and seen[0] is not None and not model._mc_batching_off
    assert len(launches) == 1, "one batched forward under autograd"
    loss_ref, ref = grads(True)
    assert len(seen) == 1 and len(launches) == 1
    _rel(loss, loss_ref.cpu().numpy(), "loss")
    assert set(got) == set(ref) and any(k.startswith("layers.1.q_a.") for k in got)
    for k in got:
        _rel(got[k], ref[k].cpu().numpy(), f"d {k}")


def test_a_leading_dropout_model_reaches_the_edge1_launch(dev, graph_c, monkeypatch):
    import stag_amd
    from stag_amd import distributions
    g = graph_c
    feat = torch.randn(g.number_of_nodes(), 20, device=dev)
    model = _model(lambda: distributions.AmortizedDistribution(20, 1), dev).eval()
    with torch.no_grad():
        stag_amd.manual_seed(31)
        out, calls = _spied(monkeypatch, lambda: model.forward(g, feat, n_samples=4, return_parameters=True))
        assert calls.get("stag_agg_fwd_mc_edge", 0) == 1 and "stag_agg_fwd_mc_pedge" not in calls
        model._mc_batching_off = True
        stag_amd.manual_seed(31)
        ref = model.forward(g, feat, n_samples=4, return_parameters=True)
    assert_close(out, ref.cpu().numpy(), what="[E, 1] heads behind a dropout: batched against the loop")


def test_a_leading_dropout_model_with_fixed_noise_is_the_loop_bit_for_bit(dev, graph_c, monkeypatch):
    import stag_amd
    g = graph_c
    feat = torch.randn(g.number_of_nodes(), 20, device=dev)
    model = _model(lambda: torch.distributions.Normal(1.0, 0.5), dev).eval()
    seen = _watch(monkeypatch, model.layers[1])
    with torch.no_grad():
        stag_amd.manual_seed(31)
        out = model.forward(g, feat, n_samples=4, return_parameters=True)
        assert len(seen) == 1 and seen[0] is not None
        model._mc_batching_off = True
        stag_amd.manual_seed(31)
        ref = model.forward(g, feat, n_samples=4, return_parameters=True)
    assert len(seen) == 1
    assert torch.equal(out, ref)
