"""The fused likelihood head on the GPU — stag_nll_categorical_fwd / _bwd, stag_nll_bernoulli_fwd / _bwd, ops.nll_mean,
Likelihood.mean_nll, model.loss — against the float64 numpy references of tests/nll_cases.py and torch's own route.
Values and gradients are held to util.assert_close at util.TOL (every term of the value's sum is non-negative: the plain
bar applies); the gradient is also compared after scaling by the number of masked rows, where the plain bar would
otherwise be wide next to entries of size 1 / count.  tests/test_nll_host.py asserts that a float32 evaluation of the
formulas meets the same bars on these inputs."""
import numpy as np
import pytest
import torch

import nll_cases as K
import util

pytestmark = pytest.mark.gpu
TOL = util.TOL


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _lk(kind):
    from stag_amd import likelihoods
    return likelihoods.CategoricalLikelihood() if kind == "categorical" else likelihoods.BernoulliLikelihood()


def _run(kind, feat, y, mask, upstream=0.25):
    """(value, d loss / d feat) of loss = upstream * nll + other: the upstream gradient reaches the kernel on the device."""
    from stag_amd import ops
    other = torch.ones(3, device=feat.device, requires_grad=True)
    v = ops.nll_mean(_lk(kind), feat, y, mask)
    assert v.shape == () and v.dtype == torch.float32
    (upstream * v + other.sum()).backward()
    return v.detach()


def _check(kind, p, y, mask, value, d, dev, what):
    feat = _t(p, dev).requires_grad_(True)
    v = _run(kind, feat, _t(y, dev), _t(mask, dev))
    n, C_ = p.shape
    count = K.count_of(mask, n)
    grad = _n(feat.grad)
    if count == 0:
        assert np.isnan(_n(v)) and not grad.any(), what                      # the mean of nothing; an all-zero gradient
        return
    util.assert_close(v.reshape(1), np.array([value]), what=f"{what} value")
    util.assert_close(grad, 0.25 * d, what=f"{what} gradient")
    per = count * (C_ if kind == "bernoulli" else 1)
    util.assert_close(grad.astype(np.float64) * (per / 0.25), d * per, what=f"{what} gradient x denom")
    if mask is not None:
        assert not grad[~mask].any(), what                                   # rows outside the mask: exact zeros


@pytest.mark.parametrize("n,C_,kind", K.cat_case_list())
def test_categorical_every_shape_and_mask(dev, n, C_, kind):
    p, y, mask, value, d = K.categorical_case(n, C_, kind)
    _check("categorical", p, y, mask, value, d, dev, f"categorical [{n}, {C_}] {kind}")


@pytest.mark.parametrize("n,C_,kind", K.bern_case_list())
def test_bernoulli_every_shape_and_mask(dev, n, C_, kind):
    p, y, mask, value, d = K.bernoulli_case(n, C_, kind)
    _check("bernoulli", p, y, mask, value, d, dev, f"bernoulli [{n}, {C_}] {kind}")


def test_host_side_mask(dev):
    from stag_amd import ops
    p, y, mask, value, d = K.categorical_case(1000, 7, "half")
    feat = _t(p, dev).requires_grad_(True)
    v = ops.nll_mean(_lk("categorical"), feat, _t(y, dev), torch.from_numpy(mask.copy()))      # the mask stays on the host
    v.backward()
    util.assert_close(v.reshape(1), np.array([value]), what="host mask value")
    util.assert_close(feat.grad, d, what="host mask gradient")


# ---- layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,C_", [("categorical", 1000, 40), ("categorical", 65, 7), ("bernoulli", 1000, 121),
                                        ("bernoulli", 65, 260)])
@pytest.mark.parametrize("pad", [8, 3])
def test_rows_of_a_wider_tensor(dev, kind, n, C_, pad):
    """ldp > C: a column slice of a wider tensor (pad 8 keeps C % 4 == 0 rows on 16 bytes, pad 3 does not)."""
    case = K.categorical_case if kind == "categorical" else K.bernoulli_case
    p, y, mask, value, d = case(n, C_, "half")
    lo = 4 if pad == 8 else 1
    wide = torch.full((n, C_ + pad), 0.5, device=dev)
    wide[:, lo:lo + C_] = _t(p, dev)
    wide.requires_grad_(True)
    yt = _t(y, dev)
    if kind == "bernoulli":                                                  # the targets from a wider tensor too
        ywide = torch.zeros((n, C_ + 5), device=dev)
        ywide[:, 1:1 + C_] = yt
        yt = ywide[:, 1:1 + C_]
    v = _run(kind, wide[:, lo:lo + C_], yt, _t(mask, dev))
    util.assert_close(v.reshape(1), np.array([value]), what="slice value")
    g = _n(wide.grad)
    util.assert_close(g[:, lo:lo + C_], 0.25 * d, what="slice gradient")
    assert not g[:, :lo].any() and not g[:, lo + C_:].any()


@pytest.mark.parametrize("kind,n,C_", [("categorical", 1000, 40), ("bernoulli", 200, 260)])
def test_pointer_off_a_16_byte_boundary_takes_the_scalar_form_with_the_same_bits(dev, kind, n, C_):
    p, y, mask, value, d = K.categorical_case(n, C_, "half") if kind == "categorical" else _small_bern(n, C_)
    yt, mt = _t(y, dev), _t(mask, dev)
    aligned = _t(p, dev).requires_grad_(True)
    assert aligned.data_ptr() % 16 == 0
    buf = torch.zeros(n * C_ + 1, device=dev)
    buf[1:] = _t(p, dev).reshape(-1)
    buf.requires_grad_(True)
    off = buf[1:].view(n, C_)
    assert off.data_ptr() % 16 == 4 and C_ % 4 == 0
    va = _run(kind, aligned, yt, mt)
    vo = _run(kind, off, yt, mt)
    assert torch.equal(va, vo)
    assert torch.equal(aligned.grad.reshape(-1), buf.grad[1:]) and float(buf.grad[0]) == 0.0
    util.assert_close(vo.reshape(1), np.array([value]), what="misaligned value")
    util.assert_close(buf.grad[1:].view(n, C_), 0.25 * d, what="misaligned gradient")


def _small_bern(n, C_):
    p, y = K.bernoulli_inputs(n, C_, 3)
    mask = K.mask_of("half", n, 3)
    return (p, y, mask) + K.bernoulli_ref(p, y, mask)


def test_gradient_rows_of_another_stride(dev):
    """lddp != ldp at the C entry: dprobs is a slice of a wider buffer; nothing outside the slice is written."""
    from stag_amd import _lib
    for kind, n, C_ in (("categorical", 200, 7), ("bernoulli", 130, 5), ("categorical", 130, 40)):
        if kind == "categorical":
            p, y = K.categorical_inputs(n, C_, 5)
            mask = K.mask_of("half", n, 5)
            value, d = K.categorical_ref(p, y, mask, g=0.5)
        else:
            p, y = K.bernoulli_inputs(n, C_, 5)
            mask = K.mask_of("half", n, 5)
            value, d = K.bernoulli_ref(p, y, mask, g=0.5)
        wide_in = torch.zeros((n, C_ + 4), device=dev)
        wide_in[:, :C_] = _t(p, dev)
        feat, yt, mt = wide_in[:, :C_], _t(y, dev), _t(mask, dev)
        out = torch.empty(2, device=dev)
        nbytes = _lib.lib().stag_nll_workspace_bytes(n, C_)
        ws = torch.empty(max(nbytes // 4, 1), device=dev)
        g = torch.tensor([0.5], device=dev)
        dwide = torch.full((n, C_ + 9), -7.0, device=dev)
        dp = dwide[:, 2:2 + C_]
        s = _lib.stream_of(dev)
        with _lib.on_device(dev):
            if kind == "categorical":
                rc = _lib.lib().stag_nll_categorical_fwd(feat.data_ptr(), C_ + 4, n, C_, yt.data_ptr(), mt.data_ptr(),
                                                         out.data_ptr(), out.data_ptr() + 4, ws.data_ptr(), nbytes, s)
                assert rc == 0
                rc = _lib.lib().stag_nll_categorical_bwd(feat.data_ptr(), C_ + 4, n, C_, yt.data_ptr(), mt.data_ptr(),
                                                         g.data_ptr(), out.data_ptr() + 4, dp.data_ptr(), C_ + 9, s)
            else:
                rc = _lib.lib().stag_nll_bernoulli_fwd(feat.data_ptr(), C_ + 4, yt.data_ptr(), C_, n, C_, mt.data_ptr(),
                                                       out.data_ptr(), out.data_ptr() + 4, ws.data_ptr(), nbytes, s)
                assert rc == 0
                rc = _lib.lib().stag_nll_bernoulli_bwd(feat.data_ptr(), C_ + 4, yt.data_ptr(), C_, n, C_, mt.data_ptr(),
                                                       g.data_ptr(), out.data_ptr() + 4, dp.data_ptr(), C_ + 9, s)
        assert rc == 0
        got = _n(dwide)
        util.assert_close(_n(out)[:1], np.array([value]), what=f"{kind} raw value")
        assert _n(out)[1] == K.count_of(mask, n) * (C_ if kind == "bernoulli" else 1)
        util.assert_close(got[:, 2:2 + C_], d, what=f"{kind} raw gradient")
        assert (got[:, :2] == -7.0).all() and (got[:, 2 + C_:] == -7.0).all()


# ---- exact edges -----------------------------------------------------------------------------------------------------
def test_categorical_clamp_edges(dev):
    p, y, inside = K.edge_categorical()
    n = len(y)
    for r in range(n):
        mask = np.arange(n) == r
        value, d = K.categorical_ref(p, y, mask)
        feat = _t(p, dev).requires_grad_(True)
        v = _run("categorical", feat, _t(y, dev), _t(mask, dev), upstream=1.0)
        util.assert_close(v.reshape(1), np.array([value]), what=f"edge row {r} value")
        g = _n(feat.grad)
        util.assert_close(g, d, what=f"edge row {r} gradient")
        assert bool(g[r].any()) == bool(inside[r]), r                        # outside the window: exactly zero
        assert not np.delete(g, r, 0).any()
        assert np.isfinite(g).all()                                          # p_y = 0 divides nothing
    feat = _t(p, dev)
    v0 = _run("categorical", feat, _t(y, dev), _t(np.arange(n) == 0, dev))
    v1 = _run("categorical", feat, _t(y, dev), _t(np.arange(n) == 1, dev))
    util.assert_close(v0.reshape(1), np.array([-np.log(K.EPS)]), what="p_y = 0")
    util.assert_close(v1.reshape(1), np.array([-np.log(1 - K.EPS)]), what="one-hot")
    value, d = K.categorical_ref(p, y, None)
    feat = _t(p, dev).requires_grad_(True)
    v = _run("categorical", feat, _t(y, dev), None, upstream=1.0)
    util.assert_close(v.reshape(1), np.array([value]), what="edge rows together")
    util.assert_close(feat.grad, d, what="edge rows together gradient")


def test_bernoulli_clamp_edges(dev):
    p, y = K.edge_bernoulli()
    value, d = K.bernoulli_ref(p, y)
    feat = _t(p, dev).requires_grad_(True)
    v = _run("bernoulli", feat, _t(y, dev), None, upstream=1.0)
    util.assert_close(v.reshape(1), np.array([value]), what="bernoulli edges value")
    g = _n(feat.grad)
    util.assert_close(g, d, what="bernoulli edges gradient")
    assert not g[:, :2].any() and g[:, 2:].all() and np.isfinite(g).all()     # p = 0, 1: clamped; eps, 1 - eps: inside


def test_a_nan_counts_only_inside_the_mask(dev):
    for kind, n, C_ in (("categorical", 300, 7), ("bernoulli", 300, 5)):
        p, y = (K.categorical_inputs if kind == "categorical" else K.bernoulli_inputs)(n, C_, 9)
        mask = K.mask_of("half", n, 9).copy()
        mask[100], mask[101] = True, False
        ref = (K.categorical_ref if kind == "categorical" else K.bernoulli_ref)(p, y, mask)[0]
        q = p.copy(); q[101, C_ - 1] = np.nan                                # outside the mask: changes nothing
        v = _run(kind, _t(q, dev), _t(y, dev), _t(mask, dev))
        util.assert_close(v.reshape(1), np.array([ref]), what=f"{kind} NaN outside the mask")
        q = p.copy(); q[100, C_ - 1] = np.nan                                # inside: the value is NaN
        assert np.isnan(_n(_run(kind, _t(q, dev), _t(y, dev), _t(mask, dev))))
        assert np.isnan(_n(_run(kind, _t(q, dev), _t(y, dev), None)))


def test_labels_outside_the_classes(dev):
    n, C_ = 300, 7
    p, y = K.categorical_inputs(n, C_, 11)
    mask = K.mask_of("half", n, 11).copy()
    mask[[70, 150, 200]] = True
    good = _t(p, dev).requires_grad_(True)
    _run("categorical", good, _t(y, dev), _t(mask, dev))
    bad_y = y.copy(); bad_y[70], bad_y[150] = -1, C_
    feat = _t(p, dev).requires_grad_(True)
    v = _run("categorical", feat, _t(bad_y, dev), _t(mask, dev))
    assert np.isnan(_n(v))
    g = feat.grad
    assert not g[70].any() and not g[150].any() and bool(torch.isfinite(g).all())
    keep = torch.ones(n, dtype=torch.bool, device=dev); keep[70] = keep[150] = False
    assert torch.equal(g[keep], good.grad[keep])                             # the other rows: untouched, bit for bit
    huge = y.copy(); huge[200] = 2 ** 40; huge[70] = -2 ** 40                # no address is formed from a label
    assert np.isnan(_n(_run("categorical", _t(p, dev), _t(huge, dev), _t(mask, dev))))
    mask[[70, 200]] = False                                                  # ... and outside the mask it is not read
    ref = K.categorical_ref(p, y, mask)[0]
    util.assert_close(_run("categorical", _t(p, dev), _t(huge, dev), _t(mask, dev)).reshape(1), np.array([ref]), what="bad label outside")


# ---- determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,C_", [("categorical", 4099, 40), ("categorical", 1000, 257), ("bernoulli", 4099, 121)])
def test_two_calls_give_the_same_bits_and_unmasked_rows_are_not_read(dev, kind, n, C_):
    case = K.categorical_case if kind == "categorical" else K.bernoulli_case
    p, y, mask, value, d = case(n, C_, "half")
    yt, mt = _t(y, dev), _t(mask, dev)
    runs = []
    for _ in range(2):
        feat = _t(p, dev).requires_grad_(True)
        runs.append((_run(kind, feat, yt, mt), feat.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    q = p.copy()
    q[~mask] = np.where(np.arange(C_) % 2 == 0, np.nan, np.float32(3e38))   # garbage where the mask is off
    feat = _t(q, dev).requires_grad_(True)
    yg = yt
    if kind == "bernoulli":
        yy = y.copy(); yy[~mask] = np.nan
        yg = _t(yy, dev)
    v = _run(kind, feat, yg, mt)
    assert torch.equal(v, runs[0][0]) and torch.equal(feat.grad, runs[0][1])


# ---- against torch on the device, through the models -------------------------------------------------------------------
def _loss_both_ways(model, g, x, y, mask, n_samples, monkeypatch, dev):
    import stag_amd
    from stag_amd import ops
    shipped, calls, got = ops.NLL_FUSED, [], {}
    real = ops.nll_mean
    monkeypatch.setattr(ops, "nll_mean", lambda *a, **k: calls.append(1) or real(*a, **k))
    try:
        for fused in (False, True):
            ops.NLL_FUSED = fused
            model.zero_grad(set_to_none=True)
            x.grad = None
            torch.manual_seed(17)
            stag_amd.manual_seed(18)
            before = len(calls)
            loss = model.loss(g, x, y, mask=mask, n_samples=n_samples)
            loss.backward()
            assert len(calls) - before == (n_samples if fused else 0)        # the route that was meant is the one that ran
            got[fused] = (loss.detach(), x.grad.clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    finally:
        ops.NLL_FUSED = shipped
    util.assert_close(got[True][0].reshape(1), _n(got[False][0]).reshape(1), what="loss")
    assert float(got[False][1].abs().max()) > 0
    util.assert_close(got[True][1], _n(got[False][1]), what="feat.grad")
    assert set(got[True][2]) == set(got[False][2]) and got[True][2]
    for k, ref in got[False][2].items():
        util.assert_close(got[True][2][k], _n(ref), what=f"d {k}")


def _gcn(in_f, hidden, out_f, act, dev, likelihood=None):
    import stag_amd
    SL, Z = stag_amd.layers.StagLayer, stag_amd.zoo
    q_a = torch.distributions.Normal(1.0, 0.3)
    layers = torch.nn.ModuleList([SL(Z.GCN(in_f, hidden, activation=torch.relu, allow_zero_in_degree=True), q_a=q_a),
                                  SL(Z.GCN(hidden, out_f, activation=act, allow_zero_in_degree=True), q_a=q_a)])
    return stag_amd.models.StagModel(layers=layers, likelihood=likelihood).to(dev)


def test_two_layer_gcn_loss_fused_against_composed(dev, monkeypatch):
    g = util.random_graph(300, 2400, seed=4, device=dev)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(300, 16, generator=gen).to(dev).requires_grad_(True)
    y = torch.randint(0, 5, (300,), generator=gen).to(dev)
    mask = (torch.rand(300, generator=gen) < 0.5).to(dev)
    torch.manual_seed(1)
    model = _gcn(16, 8, 5, lambda t: torch.softmax(t, -1), dev)
    _loss_both_ways(model, g, x, y, mask, 2, monkeypatch, dev)


def test_bernoulli_model_loss_fused_against_composed(dev, monkeypatch):
    from stag_amd import likelihoods
    g = util.random_graph(300, 2400, seed=5, device=dev)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(300, 16, generator=gen).to(dev).requires_grad_(True)
    y = (torch.rand(300, 11, generator=gen) < 0.5).float().to(dev)
    torch.manual_seed(2)
    model = _gcn(16, 8, 11, torch.sigmoid, dev, likelihood=likelihoods.BernoulliLikelihood())
    _loss_both_ways(model, g, x, y, None, 2, monkeypatch, dev)


def test_contrastive_model_loss_fused_against_composed(dev, monkeypatch):
    import stag_amd
    L, Z, Dist = stag_amd.layers, stag_amd.zoo, stag_amd.distributions
    g = util.random_graph(200, 1500, seed=6, device=dev)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(200, 16, generator=gen).to(dev).requires_grad_(True)
    y = torch.randint(0, 4, (200,), generator=gen).to(dev)
    mask = (torch.rand(200, generator=gen) < 0.5).to(dev)
    torch.manual_seed(3)
    layers = torch.nn.ModuleList([
        L.StagLayer(Z.GCN(16, 8, activation=torch.nn.functional.relu, allow_zero_in_degree=True),
                    q_a=Dist.AmortizedDistribution(16, 1), p_a=torch.distributions.Normal(0.5, 1.0), vi=True),
        L.StagLayer(Z.GCN(8, 4, activation=lambda t: torch.softmax(t, -1), allow_zero_in_degree=True),
                    q_a=Dist.AmortizedDistribution(8, 1), p_a=torch.distributions.Normal(0.5, 1.0), vi=True)])
    model = stag_amd.models.StagModelContrastive(layers=layers, kl_scaling=0.37).to(dev)
    _loss_both_ways(model, g, x, y, mask, 2, monkeypatch, dev)


def test_a_masked_training_step_does_not_synchronise_the_host(dev, monkeypatch):
    from stag_amd import ops
    monkeypatch.setattr(ops, "NLL_FUSED", True)
    calls = []
    real = ops.nll_mean
    monkeypatch.setattr(ops, "nll_mean", lambda *a, **k: calls.append(1) or real(*a, **k))
    g = util.random_graph(300, 2400, seed=4, device=dev)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(300, 16, generator=gen).to(dev)
    y = torch.randint(0, 5, (300,), generator=gen).to(dev)
    mask = (torch.rand(300, generator=gen) < 0.5).to(dev)
    torch.manual_seed(1)
    model = _gcn(16, 8, 5, lambda t: torch.softmax(t, -1), dev)
    opt = torch.optim.Adam(model.parameters(), 1e-3)

    def step():
        opt.zero_grad()
        loss = model.loss(g, x, y, mask=mask, n_samples=2)
        loss.backward()
        opt.step()
        return loss
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    before = len(calls)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            loss = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) - before == 6 and bool(torch.isfinite(loss))
