"""The per-edge parameter gradients of a Monte-Carlo batch from one pass: stag_agg_bwd_w_mc and the backward routes of
ops.aggregate_mc's two autograd nodes around it.  Values against the CPU oracle, called per sample at offset + s * stride
with deriv = 1 | 2 under the device's normal tables (util.hw_normals) and summed over the samples (and over k for [E, 1]
heads) in float64; the bar is util.TOL relative to max(1, max |ref|), the one stag_agg_bwd_edge's gradients meet in
test_gpu_counter_space.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_mc_pedge import _kinds
from util import TOL, assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
SEG = 64
MAX_K = 4              # kBwdWMcMaxK (csrc/agg_bwd_w_mc.hpp)


@pytest.fixture(scope="module")
def graph_a(dev):
    """test_gpu_mc_pedge's graph_a: a hub row of 18 segments, rows past the Kahan length, multi-edges, a node without
    in-edges."""
    g = random_graph(67, 400, seed=11, hub=1100, device=dev)
    plan = g.csr.plan(SEG, need=True)
    assert int(np.diff(plan["long_seg_ptr"].cpu().numpy()).max()) >= 18
    assert int(g.csr.degrees.min()) == 0
    return g


@pytest.fixture(autouse=True)
def _fused(monkeypatch):
    """These tests are about the batched call whatever the shipped default of the switches is."""
    from stag_amd import ops
    monkeypatch.setattr(ops, "MC_BWD_FUSED", True)
    monkeypatch.setattr(ops, "MC_PEDGE_FUSED", True)
    monkeypatch.setattr(ops, "MC_EDGE_FUSED", True)


def _np(p):
    return p.detach().cpu().numpy()


def _noise(g, D, wide, kind, p0, p1, relu, p1_log, **kw):
    """The descriptor of [E, D] (wide) or [E, 1] tables, whatever E and D are (the descriptor calls one edge's row SCALAR or
    PER_CHANNEL and an [E, 1] table PER_EDGE1; the same memory is what this entry point is told it is)."""
    import stag_amd
    from stag_amd import _lib
    k = {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM}[kind]
    n = stag_amd.EdgeNoise(g, D, k, p0, p1, relu=relu, p1_log=p1_log, **kw)
    assert tuple(p0.shape) == (g.number_of_edges(), D if wide else 1)
    n.param_mode = _lib.PARAM_PER_EDGE if wide else _lib.PARAM_PER_EDGE1
    n.p0, n.p1, n.p1_log = p0.contiguous(), p1.contiguous(), bool(p1_log)
    return n


def _call(csrv, x, g_all, noise, S, stride=1, ss=None, gs=None, reduce_k=False, seg_len=SEG, both=True, out=None):
    """The entry point itself.  out: (dw0, dw1) views to write into (their row stride is ldw), else fresh tensors."""
    from stag_amd import ops
    if out is None:
        return ops._bwd_w_mc_raw(csrv, x, g_all, x.shape[1], ss, gs, noise.spec(), S, stride, reduce_k=reduce_k,
                                 seg_len=seg_len, both=both)
    from stag_amd import _lib
    dev = x.device
    plan_c, _keep = ops._plan_struct(csrv, seg_len, 1, 0, dev)
    cs, spec = csrv.struct(), noise.spec()
    rc = _lib.lib().stag_agg_bwd_w_mc(C.byref(cs), C.byref(plan_c) if plan_c is not None else None, _lib.ptr(x), x.stride(0),
                                      _lib.ptr(g_all), g_all.stride(1), g_all.stride(0), x.shape[1], _lib.ptr(ss),
                                      _lib.ptr(gs), C.byref(spec), S, stride, int(reduce_k), _lib.ptr(out[0]),
                                      _lib.ptr(out[1]), out[0].stride(0), _lib.stream_of(dev))
    _lib.check(rc, "stag_agg_bwd_w_mc")
    return out


def _oref(O, og, E, xn, gn, kind, p0, p1, relu, p1_log, S, stride, offset, reduce_k, ss=None, gs=None, **kw):
    """(d p0, d p1) in float64: oracle.agg_bwd_w per sample and derivative, summed over s (and over k with reduce_k)."""
    D = xn.shape[1]
    refs = []
    for dv in (1, 2):
        tot = np.zeros((E, D), np.float64)
        for s in range(S):
            spec = O.make_spec(kind, _np(p0), _np(p1), relu=relu, p1_log=p1_log, Dn=D, n_edges=E, offset=offset + s * stride,
                               deriv=dv, **kw)
            gg = gn[s] if gs is None else gn[s] * gs[:, None]
            tot += O.agg_bwd_w(og, xn, gg, src_scale=ss, spec=spec).astype(np.float64)
        refs.append(tot.sum(1, keepdims=True) if reduce_k else tot)
    return refs


def _rel(got, ref, what):
    ref = np.asarray(ref, np.float64)
    sc = max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    assert_close(_np(got) / sc, ref / sc, what=what)


def _inputs(n, D, S, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=gen).to(dev)
    G = torch.randn(S, n, D, generator=gen).to(dev)
    ss = (0.5 + torch.rand(n, generator=gen)).to(dev)
    gs = (0.5 + torch.rand(n, generator=gen)).to(dev)
    return x, G, ss, gs


# ---- 1. values -----------------------------------------------------------------------------------------------------
WIDE = [(True, D, 5) for D in (1, 7, 20, 128, 260)] + [(True, 20, S) for S in (1, 2, 3, 4, 7)]
NARROW = [(False, D, 5) for D in (7, 20, 260, 300)] + [(False, 20, S) for S in (1, 2, 3, 4, 7)]


@pytest.mark.parametrize("wide,D,S", WIDE + NARROW)
def test_values_against_the_oracle(dev, oracle, graph_a, wide, D, S):
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    og = oracle_graph(oracle, g)
    x, G, ssd, gsd = _inputs(n, D, S, dev, 100 + D + S)
    xn, gn, ss, gs = _np(x), _np(G), _np(ssd), _np(gsd)
    epoch = torch.full((1,), 5, dtype=torch.int64, device=dev)
    rk = not wide
    heads = "[E, D]" if wide else "[E, 1]"
    with hw_normals(oracle, dev):
        for name, (kind, p0, p1, relu, plog) in _kinds(E, D if wide else 1, dev).items():
            for stride, pos_base, ep in ((1, 0, None), (3, (7 << 32) + 12345, epoch)):
                noise = _noise(g, D, wide, kind, p0, p1, relu, plog, seed=21, offset=3, pos_base=pos_base, epoch=ep)
                off = 3 + (5 if ep is not None else 0)
                ref = _oref(oracle, og, E, xn, gn, kind, p0, p1, relu, plog, S, stride, off, rk, ss, gs, seed=21,
                            pos_base=pos_base)
                for seg_len, tag in ((SEG, "plan"), (0, "no plan")):
                    got = _call(g.csr, x, G, noise, S, stride, ssd, gsd, reduce_k=rk, seg_len=seg_len)
                    for i in range(2):
                        assert got[i].shape == (E, 1 if rk else D)
                        _rel(got[i], ref[i], f"{heads} {name} D={D} S={S} stride={stride} {tag} d p{i}")
                if pos_base == 0:
                    # without the scales; and one gradient table alone (dw1 == NULL)
                    ref = _oref(oracle, og, E, xn, gn, kind, p0, p1, relu, plog, S, stride, off, rk, seed=21)
                    got = _call(g.csr, x, G, noise, S, stride, reduce_k=rk)
                    for i in range(2):
                        _rel(got[i], ref[i], f"{heads} {name} D={D} S={S} unscaled d p{i}")
                    one = _call(g.csr, x, G, noise, S, stride, reduce_k=rk, both=False)
                    assert one[1] is None and torch.equal(one[0], got[0]), f"{heads} {name} D={D} S={S}: dw1 == NULL"


# ---- 2. bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide,D", [(True, 20), (True, 7), (True, 260), (False, 20), (False, 7), (False, 300)])
def test_one_sample_is_stag_agg_bwd_w_bit_for_bit(dev, graph_a, wide, D):
    """n_samples == 1, g_scale == NULL: the sums start from sample 0's term, so the outputs are stag_agg_bwd_w's."""
    from stag_amd import ops
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, G, ss, _ = _inputs(n, D, 1, dev, 7 + D)
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D if wide else 1, dev).items():
        noise = _noise(g, D, wide, kind, p0, p1, relu, plog, seed=9, offset=11)
        for seg_len in (SEG, 0):
            for s_ in (ss, None):
                got = _call(g.csr, x, G, noise, 1, 1, s_, None, reduce_k=not wide, seg_len=seg_len)
                ref = ops._bwd_w_raw(g.csr, x, G[0], D, s_, spec=noise.spec(), reduce_k=not wide, both=True, seg_len=seg_len)
                for i in range(2):
                    assert torch.equal(got[i].view(torch.int32), ref[i].view(torch.int32)), f"{name} D={D} seg_len={seg_len} d p{i}"


@pytest.mark.parametrize("wide,D", [(True, 20), (True, 260), (False, 20), (False, 300)])
def test_two_runs_are_bit_identical(dev, graph_a, wide, D):
    g = graph_a
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, G, ss, gs = _inputs(n, D, 7, dev, 3 + D)
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D if wide else 1, dev).items():
        noise = _noise(g, D, wide, kind, p0, p1, relu, plog, seed=6, offset=2)
        a = _call(g.csr, x, G, noise, 7, 2, ss, gs, reduce_k=not wide)
        b = _call(g.csr, x, G, noise, 7, 2, ss, gs, reduce_k=not wide)
        for i in range(2):
            assert torch.equal(a[i].view(torch.int32), b[i].view(torch.int32)), f"{name} D={D}: two calls, different bits"


def _shifted(t):
    """The same values one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device)
    assert buf.data_ptr() % 16 == 0
    q = buf[1:].view(t.shape)
    q.copy_(t)
    assert q.data_ptr() % 16 == 4
    return q


@pytest.mark.parametrize("wide,D", [(True, 20), (True, 260), (False, 20), (False, 300)])
def test_the_scalar_row_forms_give_the_same_bits(dev, graph_a, wide, D):
    """An x view offset by one float, gradient rows and parameter tables at 4-byte alignment and an odd ldw take the scalar
    forms; S = 7 runs through a later pass too, which reads the rows back."""
    g = graph_a
    n, E, S = g.number_of_nodes(), g.number_of_edges(), 7
    x, G, ss, gs = _inputs(n, D, S, dev, 5 + D)
    cols = D if wide else 1
    for name, (kind, p0, p1, relu, plog) in _kinds(E, D if wide else 1, dev).items():
        aligned = _noise(g, D, wide, kind, p0, p1, relu, plog, seed=12, offset=5)
        a = _call(g.csr, x, G, aligned, S, 2, ss, gs, reduce_k=not wide)
        assert x.data_ptr() % 16 == 0 and a[0].data_ptr() % 16 == 0
        # x alone
        b = _call(g.csr, _shifted(x), G, aligned, S, 2, ss, gs, reduce_k=not wide)
        # the gradient rows, the tables and the outputs: rows cols + 1 floats apart, NaN between them
        off = _noise(g, D, wide, kind, _shifted(p0), _shifted(p1), relu, plog, seed=12, offset=5)
        bufs = [torch.full((E, cols + 1), float("nan"), device=dev) for _ in range(2)]
        c = _call(g.csr, x, _shifted(G), off, S, 2, ss, gs, reduce_k=not wide, out=tuple(t[:, :cols] for t in bufs))
        for i in range(2):
            assert torch.equal(a[i].view(torch.int32), b[i].view(torch.int32)), f"{name} D={D} shifted x d p{i}"
            assert torch.equal(a[i].view(torch.int32), c[i].contiguous().view(torch.int32)), f"{name} D={D} odd ldw d p{i}"
            assert bool(torch.isnan(bufs[i][:, cols]).all()), "the padding column is not written"


# ---- 3. degenerate graphs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [True, False])
def test_no_edges_and_one_edge(dev, oracle, wide):
    D, S = 20, 3
    for e in (0, 1):
        g = random_graph(5, e, seed=3, device=dev)
        og = oracle_graph(oracle, g)
        x, G, ss, gs = _inputs(5, D, S, dev, 9)
        W = D if wide else 1
        p0 = torch.linspace(0.3, 0.6, W, device=dev).repeat(e, 1).reshape(e, W)
        p1 = torch.linspace(1.2, 1.7, W, device=dev).repeat(e, 1).reshape(e, W)
        noise = _noise(g, D, wide, "uniform", p0, p1, False, False, seed=2, offset=1)
        got = _call(g.csr, x, G, noise, S, 1, ss, gs, reduce_k=not wide)
        assert got[0].shape == got[1].shape == (e, W)
        if e:
            ref = _oref(oracle, og, e, _np(x), _np(G), "uniform", p0, p1, False, False, S, 1, 1, not wide, _np(ss), _np(gs), seed=2)
            for i in range(2):
                _rel(got[i], ref[i], f"one edge d p{i}")


# ---- 4. autograd: the two nodes of ops.aggregate_mc -----------------------------------------------------------------------
def _counted(monkeypatch):
    from stag_amd import ops
    calls = {"mc": 0, "w": 0, "edge": 0}
    for key, name in (("mc", "_bwd_w_mc_raw"), ("w", "_bwd_w_raw"), ("edge", "_agg_bwd_edge_raw")):
        real = getattr(ops, name)

        def stub(*a, _real=real, _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, stub)
    return calls


@pytest.mark.parametrize("wide,D,need_x", [(True, 20, True), (True, 20, False), (True, 260, True),
                                           (False, 20, False), (False, 20, True), (False, 260, True), (False, 260, False)])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_gradients_with_the_switch_on_and_off(dev, graph_a, monkeypatch, reduce, wide, D, need_x):
    import stag_amd
    from stag_amd import _lib, ops
    g = graph_a
    n, E, S = g.number_of_nodes(), g.number_of_edges(), 3
    x0, G, ss, ds = _inputs(n, D, S, dev, 31 + D)
    W = D if wide else 1
    gen = torch.Generator().manual_seed(4)
    loc0, ls0 = (torch.rand(E, W, generator=gen) + 0.5).to(dev), (torch.rand(E, W, generator=gen) - 1.0).to(dev)
    calls = _counted(monkeypatch)
    res, seen = [], []
    for fused in (True, False):
        monkeypatch.setattr(ops, "MC_BWD_FUSED", fused)
        loc, ls = loc0.clone().requires_grad_(True), ls0.clone().requires_grad_(True)
        x = x0.clone().requires_grad_(need_x)
        noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, loc, ls, p1_log=True, differentiable=True, seed=3, offset=17)
        assert noise.param_mode == (_lib.PARAM_PER_EDGE if wide else _lib.PARAM_PER_EDGE1)
        noise.n_samples, noise.offset_stride = S, 2
        out = ops.aggregate(g, x, noise, reduce=reduce, src_scale=ss, dst_scale=ds)
        assert ("_AggregateMCPEdge" if wide else "_AggregateMCEdge") in type(out.grad_fn).__name__
        for k in calls:
            calls[k] = 0
        out.backward(G)
        seen.append(dict(calls))
        res.append((x.grad, loc.grad, ls.grad))
    # which route ran: [E, 1] heads with dx at D <= 256 keep stag_agg_bwd_edge's one gather per sample
    keeps_loop = not wide and need_x and D <= 256
    if keeps_loop:
        assert seen[0] == seen[1] == {"mc": 0, "w": 0, "edge": S}
    else:
        assert seen[0] == {"mc": 1, "w": 0, "edge": 0}
        assert seen[1]["mc"] == 0 and seen[1]["w"] + seen[1]["edge"] == S
    for got, ref, nm in zip(res[0], res[1], ("dx", "d loc", "d log_scale")):
        if nm == "dx" and not need_x:
            assert got is None and ref is None
            continue
        assert got.shape == ref.shape
        _rel(got, _np(ref), f"{reduce} D={D} {nm}")
    assert res[0][1].shape == (E, W) and float(res[0][1].abs().max()) > 0 and float(res[0][2].abs().max()) > 0


# ---- 5. one whole model ---------------------------------------------------------------------------------------------------
def test_training_a_model_with_the_switch_on_and_off(dev, monkeypatch):
    """StagLayer(GCN(20, 8), q_a = AmortizedDistribution(20, 20), vi = True) behind no dropout: StagModel.loss(n_samples = 3)
    gives the same loss and the same gradients."""
    import stag_amd
    from stag_amd import distributions, layers, models, ops, zoo
    g = random_graph(300, 600, seed=12, device=dev)
    n = g.number_of_nodes()
    gen = torch.Generator().manual_seed(2)
    feat = torch.randn(n, 20, generator=gen).to(dev)
    y = torch.randint(0, 8, (n,), generator=gen).to(dev)
    torch.manual_seed(5)
    model = models.StagModel(torch.nn.ModuleList([
        layers.StagLayer(zoo.GCN(20, 8, activation=torch.nn.Softmax(-1)), q_a=distributions.AmortizedDistribution(20, 20), vi=True),
    ])).to(dev).train()
    calls = _counted(monkeypatch)

    def grads(fused):
        monkeypatch.setattr(ops, "MC_BWD_FUSED", fused)
        model.zero_grad(set_to_none=True)
        stag_amd.manual_seed(41)
        for k in calls:
            calls[k] = 0
        loss = model.loss(g, feat, y, n_samples=3)
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, dict(calls)
    loss, got, on = grads(True)
    loss_ref, ref, off = grads(False)
    assert not getattr(model, "_mc_batching_off", False)
    assert on["mc"] == 1 and off["mc"] == 0 and off["w"] == on["w"] + 3 and on["edge"] == off["edge"]
    _rel(loss, _np(loss_ref), "loss")
    assert set(got) == set(ref) and any(k.startswith("layers.0.q_a.") for k in got)
    for k in got:
        _rel(got[k], _np(ref[k]), f"d {k}")
