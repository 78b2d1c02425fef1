"""The fused node block on the GPU — stag_node_norm_stats / _fwd / _bwd, ops.node_block, layers.FeatOnlyLayer — against
float64 numpy references (tests/node_block_cases.py), the oracle's Bernoulli field, and torch's own modules.
Tensors are held to util.assert_close at util.TOL; the column sums (dgamma, dbeta, mean * N) to util.assert_close_cond
with sum |terms|: fp32 rounding of thousands of terms is what the conditioned bar exists for."""
import numpy as np
import pytest
import torch

import node_block_cases as K
import util

pytestmark = pytest.mark.gpu
TOL = util.TOL
EPS = K.EPS


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _mask(O, N, D, p, seed, offset):
    """The oracle's materialised Bernoulli field on the N-edge identity graph (edge n at CSR position n)."""
    from stag_amd import random as srandom
    ids = np.arange(N, dtype=np.int32)
    og = O.CsrGraph(np.arange(N + 1, dtype=np.int32), ids, eid=ids, n_src=N)
    spec = O.make_spec("bernoulli", 1.0 - p, seed=seed ^ srandom.NODE_DROP_DOMAIN, offset=offset, Dn=D, n_edges=N)
    return O.noise_materialize(og, spec, D)


def _drop(p, seed, offset):
    from stag_amd import random as srandom
    return (p, seed ^ srandom.NODE_DROP_DOMAIN, offset, None)


def _check_stats(mean, rstd, x, what):
    m, v = K.stats(x)
    N = x.shape[0]
    util.assert_close(mean, m, what=f"{what} mean")
    util.assert_close_cond(_n(mean).astype(np.float64) * N, m * N, np.abs(np.asarray(x, np.float64)).sum(0), what=f"{what} mean * N")
    util.assert_close(rstd, 1.0 / np.sqrt(v + EPS), what=f"{what} rstd")


# ---- statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", K.SHAPES)
def test_statistics_every_shape(dev, N, D):
    from stag_amd import ops
    x = K.inputs(N, D, 7)[0]
    mean, rstd = ops._node_stats_raw(_t(x, dev), EPS)
    _check_stats(mean, rstd, x, f"[{N}, {D}]")


@pytest.mark.parametrize("N", [257, 1000, 4099])
def test_shifted_column_keeps_its_variance(dev, N):
    """x = 100 + N(0, 1): E[x^2] - mean^2 in fp32 misses the bar by 470x to 1400x here; the slab-wise shifted sums merged
    by Chan's formula must not."""
    from stag_amd import ops
    rng = np.random.default_rng(N)
    x = (100.0 + rng.standard_normal((N, 12))).astype(np.float32)
    mean, rstd = ops._node_stats_raw(_t(x, dev), EPS)
    _check_stats(mean, rstd, x, f"shifted N = {N}")


def test_constant_column_has_zero_variance_and_a_finite_output(dev):
    from stag_amd import ops
    x, gamma, beta, _g = K.inputs(300, 8, 5)
    x[:, 2] = 3.25
    x[:, 5] = -1e-3
    mean, rstd = ops._node_stats_raw(_t(x, dev), EPS)
    _check_stats(mean, rstd, x, "constant")
    assert _n(rstd)[2] == pytest.approx(EPS ** -0.5, rel=1e-6) and _n(rstd)[5] == pytest.approx(EPS ** -0.5, rel=1e-6)
    assert _n(mean)[2] == 3.25
    y = _n(ops._node_fwd_raw(_t(x, dev), mean, rstd, _t(gamma, dev), _t(beta, dev), True, None))
    assert np.isfinite(y).all() and (y[:, 2] == beta[2]).all()


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("track", [True, False])
def test_buffers_after_one_and_three_calls_follow_torch(dev, momentum, track):
    """FeatOnlyLayer with the switch on and off: outputs, every gradient, running_mean, running_var and num_batches_tracked
    over three optimiser-free steps."""
    import stag_amd
    from stag_amd import ops
    nn = torch.nn
    N, D = 1000, 50
    mk = lambda: nn.Sequential(nn.BatchNorm1d(D, momentum=momentum, track_running_stats=track), nn.ReLU())
    fused, plain = mk().to(dev), mk().to(dev)
    gamma, beta = K.inputs(N, D, 1)[1:3]
    for b in (fused, plain):
        with torch.no_grad():
            b[0].weight.copy_(_t(gamma, dev)); b[0].bias.copy_(_t(beta, dev))
    lf, lp = stag_amd.layers.FeatOnlyLayer(fused), stag_amd.layers.FeatOnlyLayer(plain)
    shipped = ops.NODE_BLOCK_FUSED
    try:
        for step in range(3):
            x, _, _, g = K.inputs(N, D, 10 + step)
            x = x + np.float32(0.25 * step)                      # the running mean has somewhere to go
            outs = []
            for layer, on in ((lf, True), (lp, False)):
                ops.NODE_BLOCK_FUSED = on
                assert (ops.node_block_why_not(layer.layer, _t(x, dev)) is None) == on
                xd = _t(x, dev).requires_grad_(True)
                layer.zero_grad(set_to_none=True)
                y = layer(None, xd)
                y.backward(_t(g, dev))
                outs.append((y, xd.grad, layer.layer[0].weight.grad, layer.layer[0].bias.grad))
            m, v = K.stats(x)
            ref = K.block(x, m, v, gamma, beta, True, g=g)
            assert np.abs(ref["pre"]).min() >= 0.1
            (y, dx, dg, db), (ty, tdx, tdg, tdb) = outs
            util.assert_close(y, _n(ty).astype(np.float64), what=f"step {step} y vs torch")
            util.assert_close(dx, _n(tdx).astype(np.float64), what=f"step {step} dx vs torch")
            util.assert_close(y, ref["y"], what=f"step {step} y")
            util.assert_close(dx, ref["dx"], what=f"step {step} dx")
            for got, other, name in ((dg, tdg, "dgamma"), (db, tdb, "dbeta")):
                util.assert_close_cond(got, ref[name], ref["abs_" + name], what=f"step {step} {name}")
                util.assert_close_cond(got, _n(other).astype(np.float64), ref["abs_" + name], what=f"step {step} {name} vs torch")
            if track:
                util.assert_close(fused[0].running_mean, _n(plain[0].running_mean).astype(np.float64), what=f"step {step} running_mean")
                util.assert_close(fused[0].running_var, _n(plain[0].running_var).astype(np.float64), what=f"step {step} running_var")
                assert int(fused[0].num_batches_tracked) == int(plain[0].num_batches_tracked) == step + 1
                if step == 0:                                    # ... and against the definition, after one call
                    f = 0.1 if momentum is not None else 1.0
                    util.assert_close(fused[0].running_mean, f * m, what="running_mean after one call")
                    util.assert_close(fused[0].running_var, (1 - f) * 1.0 + f * v * N / (N - 1), what="running_var after one call")
            else:
                assert fused[0].running_mean is None and fused[0].num_batches_tracked is None
    finally:
        ops.NODE_BLOCK_FUSED = shipped


# ---- forward and backward values --------------------------------------------------------------------------------------
def _run_raw(dev, x, gamma, beta, g, relu, drop, batch_stats=True, mean=None, rstd=None, xd=None, gd=None):
    from stag_amd import ops
    xd = _t(x, dev) if xd is None else xd
    gd = _t(g, dev) if gd is None else gd
    if mean is None:
        mean, rstd = ops._node_stats_raw(xd, EPS)
    y = ops._node_fwd_raw(xd, mean, rstd, _t(gamma, dev), _t(beta, dev), relu, drop)
    dx, dgamma, dbeta = ops._node_bwd_raw(xd, gd, mean, rstd, _t(gamma, dev), _t(beta, dev), relu, drop, batch_stats)
    return y, dx, dgamma, dbeta, mean, rstd


def _check_values(got, ref, what, relu=True):
    y, dx, dgamma, dbeta = got[:4]
    assert not relu or np.abs(ref["pre"]).min() >= 0.1, "the inputs must keep every ReLU decision away from 0"
    util.assert_close(y, ref["y"], what=f"{what} y")
    util.assert_close(dx, ref["dx"], what=f"{what} dx")
    util.assert_close_cond(dgamma, ref["dgamma"], ref["abs_dgamma"], what=f"{what} dgamma")
    util.assert_close_cond(dbeta, ref["dbeta"], ref["abs_dbeta"], what=f"{what} dbeta")


@pytest.mark.parametrize("N,D", K.SHAPES)
def test_values_every_shape_relu_and_dropout(dev, oracle, N, D):
    x, gamma, beta, g = K.inputs(N, D, 100 + N + D)
    mask = _mask(oracle, N, D, 0.5, 1234, 5)
    m, v = K.stats(x)
    got = _run_raw(dev, x, gamma, beta, g, True, _drop(0.5, 1234, 5))
    _check_values(got, K.block(x, m, v, gamma, beta, True, mask, 0.5, g), f"[{N}, {D}]")


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.1])
@pytest.mark.parametrize("affine", [True, False])
def test_values_relu_dropout_affine(dev, oracle, relu, p, affine):
    N, D = 1000, 132
    x, gamma, beta, g = K.inputs(N, D, 3)
    if not affine:
        gamma = beta = None
    mask = _mask(oracle, N, D, p, 99, 2) if p else None
    m, v = K.stats(x)
    got = _run_raw(dev, x, gamma, beta, g, relu, _drop(p, 99, 2) if p else None)
    ref = K.block(x, m, v, gamma, beta, relu, mask, 1.0 - p, g)
    _check_values(got, ref, f"relu {relu} p {p} affine {affine}", relu=relu)
    if not affine:
        assert got[2] is not None       # (the raw call may still be asked for the sums; the module has no parameters)


@pytest.mark.parametrize("how", ["padded", "offset"])
def test_padded_stride_and_misaligned_views(dev, oracle, how):
    """ld = D + 3 (rows off 16-byte alignment: the scalar forms of a D % 4 == 0 width) and a view that starts 4 bytes off."""
    N, D = 257, 132
    x, gamma, beta, g = K.inputs(N, D, 21)
    if how == "padded":
        xd = torch.full((N, D + 3), float("nan"), device=dev)[:, :D]
        gd = torch.full((N, D + 3), float("nan"), device=dev)[:, :D]
    else:
        xd = torch.full((N * D + 1,), float("nan"), device=dev)[1:].view(N, D)
        gd = torch.full((N * D + 1,), float("nan"), device=dev)[1:].view(N, D)
        assert xd.data_ptr() % 16 == 4
    xd.copy_(_t(x, dev)); gd.copy_(_t(g, dev))
    mask = _mask(oracle, N, D, 0.5, 8, 1)
    m, v = K.stats(x)
    got = _run_raw(dev, x, gamma, beta, g, True, _drop(0.5, 8, 1), xd=xd, gd=gd)
    _check_values(got, K.block(x, m, v, gamma, beta, True, mask, 0.5, g), how)
    _check_stats(got[4], got[5], x, how)


# ---- the mask -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,p", [(257, 50, 0.5), (1000, 1433, 0.1), (4099, 128, 0.5)])
def test_mask_is_the_oracles_bernoulli_field_bit_for_bit(dev, oracle, N, D, p):
    x, gamma, beta, g = K.inputs(N, D, 4)
    x = np.abs(x)                                   # every pre-activation... is made positive below: y != 0 where kept
    mean, rstd = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    got = _run_raw(dev, x, gamma, beta, np.abs(g) + 1.0, True, _drop(p, 77, 9), batch_stats=False, mean=mean, rstd=rstd)
    mask = _mask(oracle, N, D, p, 77, 9)
    assert np.array_equal(_n(got[0]) != 0, mask == 1)
    assert np.array_equal(_n(got[1]) != 0, mask == 1)           # dx = gamma * rstd * g': 0 on every dropped entry
    again = _run_raw(dev, x, gamma, beta, np.abs(g) + 1.0, True, _drop(p, 77, 9), batch_stats=False, mean=mean, rstd=rstd)
    assert torch.equal(got[0], again[0])                        # the same (seed, offset): the same mask
    other = _run_raw(dev, x, gamma, beta, np.abs(g) + 1.0, True, _drop(p, 77, 10), batch_stats=False, mean=mean, rstd=rstd)
    assert not np.array_equal(_n(other[0]) != 0, mask == 1)     # another offset: another one
    if N * D == 4099 * 128:
        keep = 1.0 - p
        frac = float((_n(got[0]) != 0).mean())
        assert abs(frac - keep) <= 5.0 * np.sqrt(keep * (1.0 - keep) / (N * D)), frac


def test_two_training_forwards_of_one_layer_draw_different_masks(dev):
    import stag_amd
    from stag_amd import ops, random as srandom
    nn = torch.nn
    layer = stag_amd.layers.FeatOnlyLayer(nn.Sequential(nn.BatchNorm1d(64), nn.ReLU(), nn.Dropout(0.5))).to(dev).train()
    x = torch.randn(500, 64, device=dev)
    shipped = ops.NODE_BLOCK_FUSED
    ops.NODE_BLOCK_FUSED = True
    try:
        e0, n0 = srandom.default_generator.offset, srandom.node_generator.offset
        a, b = layer(None, x), layer(None, x)
        assert (srandom.default_generator.offset, srandom.node_generator.offset) == (e0, n0 + 2)
        assert not torch.equal(a != 0, b != 0)
        stag_amd.manual_seed(5)
        c = layer(None, x)
        stag_amd.manual_seed(5)
        d = layer(None, x)
        assert torch.equal(c, d)                                # a seeded run replays
        own = srandom.NoiseGenerator(seed=123)
        layer.generator = own
        layer(None, x)
        assert own.offset == 1 and srandom.node_generator.offset == 1
        layer.eval()
        layer(None, x)                                          # no live dropout: no offset
        assert own.offset == 1
    finally:
        ops.NODE_BLOCK_FUSED = shipped


# ---- eval mode ----------------------------------------------------------------------------------------------------------
def test_eval_mode_uses_the_running_buffers_and_updates_nothing(dev):
    import stag_amd
    from stag_amd import ops
    nn = torch.nn
    N, D = 257, 50
    x, gamma, beta, g = K.inputs(N, D, 6)
    rng = np.random.default_rng(0)
    rm, rv = rng.normal(0, 0.2, D).astype(np.float32), rng.uniform(0.5, 2.0, D).astype(np.float32)
    beta = np.zeros(D, np.float32)
    x[7] = rm                                                   # x = running_mean and beta = 0: pre = 0 exactly
    block = nn.Sequential(nn.BatchNorm1d(D), nn.ReLU(), nn.Dropout(0.5)).to(dev)
    with torch.no_grad():
        block[0].weight.copy_(_t(gamma, dev)); block[0].bias.copy_(_t(beta, dev))
        block[0].running_mean.copy_(_t(rm, dev)); block[0].running_var.copy_(_t(rv, dev))
    layer = stag_amd.layers.FeatOnlyLayer(block).eval()
    shipped = ops.NODE_BLOCK_FUSED
    ops.NODE_BLOCK_FUSED = True
    try:
        xd = _t(x, dev).requires_grad_(True)
        y = layer(None, xd)
        y.backward(_t(g, dev))
    finally:
        ops.NODE_BLOCK_FUSED = shipped
    ref = K.block(x, rm.astype(np.float64), rv.astype(np.float64), gamma, beta, True, g=g, batch_stats=False)
    keepaway = np.abs(ref["pre"]); keepaway[7] = 1.0
    assert keepaway.min() >= 0.1
    util.assert_close(y, ref["y"], what="eval y")
    util.assert_close(xd.grad, ref["dx"], what="eval dx = gamma rstd g'")
    util.assert_close_cond(block[0].weight.grad, ref["dgamma"], ref["abs_dgamma"], what="eval dgamma")
    util.assert_close_cond(block[0].bias.grad, ref["dbeta"], ref["abs_dbeta"], what="eval dbeta")
    assert (_n(y)[7] == 0).all() and (_n(xd.grad)[7] == 0).all()
    assert np.array_equal(_n(block[0].running_mean), rm) and np.array_equal(_n(block[0].running_var), rv)
    assert int(block[0].num_batches_tracked) == 0


# ---- same bits, non-finite ------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(dev):
    x, gamma, beta, g = K.inputs(4099, 132, 8)
    a = _run_raw(dev, x, gamma, beta, g, True, _drop(0.5, 3, 3))
    b = _run_raw(dev, x, gamma, beta, g, True, _drop(0.5, 3, 3))
    for u, v, name in zip(a, b, ("y", "dx", "dgamma", "dbeta", "mean", "rstd")):
        assert torch.equal(u, v), name


def test_a_nan_stays_in_its_column(dev, oracle):
    N, D = 300, 20
    x, gamma, beta, g = K.inputs(N, D, 9)
    bad = x.copy()
    bad[123, 6] = np.nan
    mask = _mask(oracle, N, D, 0.5, 4, 4)
    got = _run_raw(dev, bad, gamma, beta, g, True, _drop(0.5, 4, 4))
    assert np.isnan(_n(got[0])[:, 6]).all()
    ok = np.arange(D) != 6
    m, v = K.stats(x)
    ref = K.block(x, m, v, gamma, beta, True, mask, 0.5, g)
    util.assert_close(_n(got[0])[:, ok], ref["y"][:, ok], what="y beside the NaN column")
    util.assert_close(_n(got[1])[:, ok], ref["dx"][:, ok], what="dx beside the NaN column")
    util.assert_close_cond(_n(got[2])[ok], ref["dgamma"][ok], ref["abs_dgamma"][ok], what="dgamma beside the NaN column")
    util.assert_close_cond(_n(got[3])[ok], ref["dbeta"][ok], ref["abs_dbeta"][ok], what="dbeta beside the NaN column")


# ---- routing --------------------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self, monkeypatch):
        from stag_amd import _lib
        self.calls = 0
        real = _lib.lib().stag_node_norm_fwd

        def fwd(*a):
            self.calls += 1
            return real(*a)
        monkeypatch.setattr(_lib.lib(), "stag_node_norm_fwd", fwd)


def test_one_fused_forward_where_the_predicate_allows_none_elsewhere(dev, monkeypatch):
    import stag_amd
    from stag_amd import ops
    nn = torch.nn
    monkeypatch.setattr(ops, "NODE_BLOCK_FUSED", True)
    spy = _Spy(monkeypatch)
    FO = stag_amd.layers.FeatOnlyLayer
    x = torch.randn(100, 8, device=dev)
    for block in (nn.Sequential(nn.BatchNorm1d(8), nn.ReLU(), nn.Dropout(0.5)), nn.Sequential(nn.BatchNorm1d(8), nn.ReLU()),
                  nn.Sequential(nn.BatchNorm1d(8), nn.Dropout(0.5)), nn.Sequential(nn.BatchNorm1d(8))):
        for train in (True, False):
            n0 = spy.calls
            FO(block).to(dev).train(train)(None, x)
            assert spy.calls == n0 + 1, (block, train)
    n0 = spy.calls
    for block, xin in ((nn.Sequential(nn.BatchNorm1d(8), nn.Tanh()), x), (nn.Sequential(nn.ReLU(), nn.BatchNorm1d(8)), x),
                       (nn.BatchNorm1d(8), x), (nn.Sequential(nn.BatchNorm1d(8), nn.ReLU()), torch.randn(10, 8, 5, device=dev)),
                       (nn.Sequential(nn.BatchNorm1d(8), nn.ReLU()).half(), x.half()),
                       (nn.Sequential(nn.BatchNorm1d(8), nn.ReLU()).double(), x.double()),
                       (nn.Sequential(nn.BatchNorm1d(8), nn.ReLU(), nn.Dropout(1.0)), x)):
        layer = FO(block).to(dev)
        assert ops.node_block_why_not(layer.layer, xin) is not None
        assert torch.equal(layer(None, xin), layer.layer(xin))
    monkeypatch.setattr(ops, "NODE_BLOCK_FUSED", False)
    FO(nn.Sequential(nn.BatchNorm1d(8), nn.ReLU())).to(dev)(None, x)
    assert spy.calls == n0


def test_under_graph_capture_the_torch_route_runs(dev, monkeypatch):
    import stag_amd
    from stag_amd import ops
    nn = torch.nn
    monkeypatch.setattr(ops, "NODE_BLOCK_FUSED", True)
    spy = _Spy(monkeypatch)
    layer = stag_amd.layers.FeatOnlyLayer(nn.Sequential(nn.BatchNorm1d(16), nn.ReLU())).to(dev).eval()
    x = torch.randn(64, 16, device=dev)
    ref = layer.layer(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        layer.layer(x)                                          # torch's warm-up before a capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        assert ops.node_block_why_not(layer.layer, x) == "capturing"
        y = layer(None, x)
    assert spy.calls == 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    layer(None, x)
    assert spy.calls == 1                                       # ... and outside the capture the fused one again


def test_the_edge_noise_stream_is_untouched(dev, monkeypatch):
    """StagLayer(GCN), the block, StagLayer(GCN) under loss(n_samples=2): the batched first layer stays on, and the
    edge-noise generator advances by exactly what it advances with the switch off."""
    import stag_amd
    from stag_amd import ops, random as srandom
    nn = torch.nn
    torch.distributions.Distribution.set_default_validate_args(False)
    g = util.random_graph(200, 1500, 3, device=dev)
    g = stag_amd.add_self_loop(stag_amd.remove_self_loop(g))
    x = torch.randn(200, 16, device=dev)
    y = torch.randint(0, 4, (200,), device=dev)

    def run(switch):
        monkeypatch.setattr(ops, "NODE_BLOCK_FUSED", switch)
        torch.manual_seed(0)
        SL, Z = stag_amd.layers.StagLayer, stag_amd.zoo
        q_a = torch.distributions.Normal(1.0, 0.3)
        model = stag_amd.models.StagModel(layers=nn.ModuleList([
            SL(Z.GCN(16, 8), q_a=q_a),
            stag_amd.layers.FeatOnlyLayer(nn.Sequential(nn.BatchNorm1d(8), nn.ReLU(), nn.Dropout(0.5))),
            SL(Z.GCN(8, 4, activation=lambda t: torch.nn.functional.softmax(t, dim=-1)), q_a=q_a)])).to(dev).train()
        stag_amd.manual_seed(42)
        e0, n0 = srandom.default_generator.offset, srandom.node_generator.offset
        loss = model.loss(g, x, y, n_samples=2)
        loss.backward()
        assert torch.isfinite(loss)
        return (srandom.default_generator.offset - e0, srandom.node_generator.offset - n0,
                getattr(model, "_mc_batching_off", False))

    spy = _Spy(monkeypatch)
    off = run(False)
    assert spy.calls == 0
    on = run(True)
    assert spy.calls == 2                                       # one block forward per Monte-Carlo sample
    assert on[0] == off[0] > 0 and (off[1], on[1]) == (0, 2)
    assert on[2] is False and off[2] is False
