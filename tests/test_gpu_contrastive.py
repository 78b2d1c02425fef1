"""stag_contrastive_nll and its route through models.nll_contrastive on the GPU.

The checker is the reference's own formula (stag/models.py:7-25) in float64 torch on the CPU — torch.distributions.Normal's
log_prob and autograd — on the fp32 inputs the kernel saw, upcast.  The bar is tests/util.assert_close at TOL = 1e-5,
gradients relative to max(1, |ref|max) AFTER multiplying by E: they carry 1 / E, and unscaled they would sit far under the
1 + |ref| of the bar, where a wrong one could pass."""
import functools
import math

import numpy as np
import pytest
import torch

from util import TOL, assert_close, random_graph

pytestmark = pytest.mark.gpu

# (N, E, hidden): one thread | a second block with one lane in it | the grid-stride loop's second trip at 512 x 256
# threads, hidden padded inside HT = 4 | the widest head table
SHAPES = [(5, 1, 1), (64, 257, 2), (300, 131072 + 300, 3), (1000, 4000, 8)]
GRADS = ("d loc", "d log_scale", "d pre", "d wh", "d bh")


@pytest.fixture(autouse=True)
def _needs_device(dev):
    pass


def _dev():
    return torch.device("cuda:0")


def _inputs(N, E, hidden, seed, pad=0, hub=False):
    """fp32 CPU inputs: P ~ N(0, 1) (`pad` further columns on each side of the table), wh ~ 0.5 N(0, 1),
    bh = (0.3, -0.2), loc ~ N(0, 1), log_scale ~ U(-1, 1), ids uniform (hub: every fake edge on node 0)."""
    gen = torch.Generator().manual_seed(seed)
    Pw = torch.randn(N, 2 * hidden + 2 * pad, generator=gen)
    wh = 0.5 * torch.randn(hidden, 2, generator=gen)
    bh = torch.tensor([0.3, -0.2])
    loc = torch.randn(E, generator=gen)
    ls = torch.rand(E, generator=gen) * 2 - 1
    fs = torch.randint(0, N, (E,), generator=gen, dtype=torch.int32)
    fd = torch.randint(0, N, (E,), generator=gen, dtype=torch.int32)
    if hub:
        fs, fd = torch.zeros_like(fs), torch.zeros_like(fd)
    return Pw, wh, bh, loc, ls, fs, fd


@functools.lru_cache(maxsize=None)
def _case(N, E, hidden, bias=True, pad=0, hub=False):
    """(inputs, float64 reference: value, d loc, d log_scale, d pre, d wh, d bh, d P), computed once and shared."""
    Pw, wh, bh, loc, ls, fs, fd = _inputs(N, E, hidden, 1000 * hidden + E % 997, pad, hub)
    d = torch.float64
    P = Pw[:, pad:pad + 2 * hidden].to(d).requires_grad_(True)
    wh64, bh64 = wh.to(d).requires_grad_(True), bh.to(d).requires_grad_(True)
    loc64, ls64 = loc.to(d).requires_grad_(True), ls.to(d).requires_grad_(True)
    pre = P[fs.long(), :hidden] + P[fd.long(), hidden:]
    pre.retain_grad()
    h = torch.nn.functional.silu(pre)
    mf, lf = h @ wh64[:, 0], h @ wh64[:, 1]
    if bias:
        mf, lf = mf + bh64[0], lf + bh64[1]
    Normal = torch.distributions.Normal
    nll = (-Normal(loc64, ls64.exp()).log_prob(torch.tensor(1.0, dtype=d))
           - Normal(mf, lf.exp()).log_prob(torch.tensor(0.0, dtype=d))).mean()
    nll.backward()
    ref = [nll.detach(), loc64.grad, ls64.grad, pre.grad, wh64.grad, bh64.grad if bias else None, P.grad]
    return (Pw, wh, bh if bias else None, loc, ls, fs, fd), [None if r is None else r.numpy() for r in ref]


def _device_inputs(inp, hidden, pad):
    dev = _dev()
    Pw, wh, bh, loc, ls, fs, fd = (None if t is None else t.to(dev) for t in inp)
    return Pw[:, pad:pad + 2 * hidden], wh, bh, loc, ls, fs, fd       # pad > 0: a column slice, row stride > 2 hidden


def _raw(inp, hidden, pad, want):
    from stag_amd import ops
    P, wh, bh, loc, ls, fs, fd = _device_inputs(inp, hidden, pad)
    assert P.stride(0) == 2 * hidden + 2 * pad
    return ops._contrastive_raw(loc, ls, fs, fd, P, hidden, wh, bh, want)


def _assert_grad(got, ref, E, what):
    sc = max(1.0, float(np.abs(ref).max()) * E)
    print(f"{what}: |ref| E max {float(np.abs(ref).max()) * E:.3e}")
    assert_close(got.detach().cpu().numpy().astype(np.float64) * E / sc, ref * E / sc, what=what)


CASES = [(s, bias, 0) for s in SHAPES for bias in (True, False)] + [(SHAPES[1], True, 3)]


@pytest.mark.parametrize("shape,bias,pad", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_value_and_gradients_against_float64(shape, bias, pad):
    N, E, hidden = shape
    inp, ref = _case(N, E, hidden, bias, pad)
    want = (True, True, True, True, bias)
    out, *grads = _raw(inp, hidden, pad, want)
    assert_close(out, ref[0].reshape(1), what=f"{shape} value")
    for g, r, nm in zip(grads, ref[1:6], GRADS):
        if r is None:
            assert g is None
            continue
        _assert_grad(g, r.reshape(g.shape), E, f"{shape} bias={bias} pad={pad} {nm}")


@pytest.mark.parametrize("shape,bias,pad", [(SHAPES[0], True, 0), (SHAPES[2], True, 0), (SHAPES[3], False, 0), (SHAPES[1], True, 3)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_value_without_gradients_is_the_same_bits(shape, bias, pad):
    N, E, hidden = shape
    inp, _ = _case(N, E, hidden, bias, pad)
    plain = _raw(inp, hidden, pad, (False,) * 5)
    assert all(g is None for g in plain[1:])
    full = _raw(inp, hidden, pad, (True, True, True, True, bias))
    some = _raw(inp, hidden, pad, (False, False, True, False, False))
    assert torch.equal(plain[0], full[0]) and torch.equal(plain[0], some[0])
    assert torch.equal(some[3], full[3])


def _through_autograd(inp, hidden):
    from stag_amd import ops
    P, wh, bh, loc, ls, fs, fd = _device_inputs(inp, hidden, 0)
    leaves = [t.clone().requires_grad_(True) for t in (loc.reshape(-1, 1), ls.reshape(-1, 1), P, wh, bh)]
    out = ops._ContrastiveNll.apply(*leaves, fs, fd)
    out.backward()
    return out.detach(), [t.grad for t in leaves]


DP_CASES = {"random": (300, 5000, 2, False), "two-blocks": (64, 257, 3, False), "hub": (50, 1000, 2, True)}


@pytest.mark.parametrize("name", list(DP_CASES))
def test_dP_through_the_autograd_function(name):
    """hub: every fake edge on node 0 — one row of 1000 edges in both views of the fake graph, past the plan's segment
    length (64): the long-row path sums it."""
    N, E, hidden, hub = DP_CASES[name]
    inp, ref = _case(N, E, hidden, True, 0, hub)
    out, (dloc, dls, dP, dwh, dbh) = _through_autograd(inp, hidden)
    assert_close(out.reshape(1), ref[0].reshape(1), what=f"{name} value")
    assert dP.shape == (N, 2 * hidden) and dloc.shape == (E, 1) and dls.shape == (E, 1)
    _assert_grad(dP, ref[6], E, f"{name} d P")
    for g, r, nm in zip((dloc, dls, dwh, dbh), (ref[1], ref[2], ref[4], ref[5]), ("d loc", "d log_scale", "d wh", "d bh")):
        _assert_grad(g, r.reshape(g.shape), E, f"{name} {nm}")
    if hub:
        assert float(dP[1:].abs().max()) == 0.0


def test_incoming_gradient_scales_every_gradient():
    from stag_amd import ops
    N, E, hidden, _ = DP_CASES["random"]
    inp, ref = _case(N, E, hidden, True, 0, False)
    P, wh, bh, loc, ls, fs, fd = _device_inputs(inp, hidden, 0)
    leaves = [t.clone().requires_grad_(True) for t in (loc.reshape(-1, 1), ls.reshape(-1, 1), P, wh, bh)]
    (ops._ContrastiveNll.apply(*leaves, fs, fd) * -2.5).backward()
    for t, r, nm in zip(leaves, (ref[1], ref[2], ref[6], ref[4], ref[5]), ("d loc", "d log_scale", "d P", "d wh", "d bh")):
        _assert_grad(t.grad, -2.5 * r.reshape(t.shape), E, f"scaled {nm}")


@pytest.mark.parametrize("name", ["random", "hub"])
def test_two_runs_are_bit_identical(name):
    N, E, hidden, hub = DP_CASES[name]
    inp, _ = _case(N, E, hidden, True, 0, hub)
    a, ga = _through_autograd(inp, hidden)
    b, gb = _through_autograd(inp, hidden)
    assert torch.equal(a, b)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    big, _ = _case(*SHAPES[2], True, 0)
    a, ga = _through_autograd(big, SHAPES[2][2])
    b, gb = _through_autograd(big, SHAPES[2][2])
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(ga, gb))


# ---- the route through models.nll_contrastive ----------------------------------------------------------------------------
def _graph_and_features(N, E, in_features, seed, requires_grad=True):
    dev = _dev()
    g = random_graph(N, E, seed, device=dev)
    feat = torch.randn(N, in_features, generator=torch.Generator().manual_seed(seed)).to(dev).requires_grad_(requires_grad)
    return g, feat


def _nll_and_grads(q, g, feat, fused, seed, monkeypatch):
    from stag_amd import models, ops
    monkeypatch.setattr(ops, "CONTRASTIVE_FUSED", fused)
    entered = []
    real = ops.contrastive_nll
    monkeypatch.setattr(ops, "contrastive_nll", lambda *a: entered.append(1) or real(*a))
    for p in list(q.parameters()) + [feat]:
        p.grad = None
    q.condition(g, feat)
    torch.manual_seed(seed)
    val = models.nll_contrastive(q, g, feat)
    state = torch.cuda.get_rng_state()
    val.backward()
    assert bool(entered) == fused
    return val.detach(), [p.grad.clone() for p in q.parameters()], feat.grad.clone(), state


def _assert_rel(got, ref, what):
    ref = ref.detach().cpu().numpy().astype(np.float64)
    sc = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    assert_close(got.detach().cpu().numpy().astype(np.float64) / sc, ref / sc, what=what)


@pytest.mark.parametrize("hidden", [None, 3])
def test_nll_contrastive_switch_on_against_off(hidden, monkeypatch):
    import stag_amd
    g, feat = _graph_and_features(200, 1500, 16, 3)
    torch.manual_seed(0)
    q = stag_amd.distributions.AmortizedDistribution(16, 1, hidden_features=hidden).to(_dev())
    v0, p0, f0, s0 = _nll_and_grads(q, g, feat, False, 21, monkeypatch)
    v1, p1, f1, s1 = _nll_and_grads(q, g, feat, True, 21, monkeypatch)
    assert_close(v1.reshape(1), v0.reshape(1).cpu().numpy(), what="nll_contrastive")
    names = [n for n, _ in q.named_parameters()]
    assert len(p0) == len(p1) == len(names)
    for a, b, n in zip(p1, p0, names):
        assert float(b.abs().max()) > 0.0, n
        _assert_rel(a, b, f"d {n}")
    assert float(f0.abs().max()) > 0.0
    _assert_rel(f1, f0, "d feat")
    assert torch.equal(s0, s1)          # both routes consumed the torch generator identically


def _contrastive_model(in_features, hidden_features, out_features, dev):
    """The model of scripts/citation_rec_contrastive/gcn/run.py:54-104, without its dropout layers."""
    import stag_amd
    L, Z, Dist = stag_amd.layers, stag_amd.zoo, stag_amd.distributions
    layers = torch.nn.ModuleList([
        L.StagLayer(Z.GCN(in_features, hidden_features, activation=torch.nn.functional.relu, allow_zero_in_degree=True),
                    q_a=Dist.AmortizedDistribution(in_features, 1), p_a=torch.distributions.Normal(0.5, 1.0), vi=True),
        L.StagLayer(Z.GCN(hidden_features, out_features, activation=lambda x: torch.nn.functional.softmax(x, dim=-1),
                          allow_zero_in_degree=True),
                    q_a=Dist.AmortizedDistribution(hidden_features, 1), p_a=torch.distributions.Normal(0.5, 1.0), vi=True)])
    return stag_amd.models.StagModelContrastive(layers=layers, kl_scaling=0.37).to(dev)


def test_model_loss_terms_switch_on_against_off(monkeypatch):
    import stag_amd
    from stag_amd import ops
    dev = _dev()
    g, feat = _graph_and_features(200, 1500, 16, 5, requires_grad=False)
    gen = torch.Generator().manual_seed(6)
    y = torch.randint(0, 4, (200,), generator=gen).to(dev)
    mask = (torch.rand(200, generator=gen) < 0.5).to(dev)
    torch.manual_seed(1)
    model = _contrastive_model(16, 8, 4, dev)
    got = {}
    for fused in (False, True):
        monkeypatch.setattr(ops, "CONTRASTIVE_FUSED", fused)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(17)
        stag_amd.manual_seed(18)
        nll, reg = model.loss_terms(g, feat, y, mask=mask)
        (nll + reg).backward()
        got[fused] = (nll.detach(), reg.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert_close(got[True][0].reshape(1), got[False][0].reshape(1).cpu().numpy(), what="nll")
    assert_close(got[True][1].reshape(1), got[False][1].reshape(1).cpu().numpy(), what="reg")
    assert set(got[True][2]) == set(got[False][2]) and any("q_a" in n for n in got[True][2])
    for n, ref in got[False][2].items():
        _assert_rel(got[True][2][n], ref, f"d {n}")


def test_peak_memory(monkeypatch):
    """The fused route allocates O(E hidden + N in); the composed one holds the [E, 2 in] concatenation (and its two
    gathered halves).  Stated, not tuned: under a quarter of one such tensor against above one."""
    import stag_amd
    from stag_amd import models, ops
    dev = _dev()
    N, K, E = 2000, 512, 200_000
    g, feat = _graph_and_features(N, E, K, 9)
    torch.manual_seed(0)
    q = stag_amd.distributions.AmortizedDistribution(K, 1).to(dev)
    one = E * 2 * K * 4
    added = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "CONTRASTIVE_FUSED", fused)
        q.condition(g, feat)
        torch.manual_seed(2)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        models.nll_contrastive(q, g, feat).backward()
        torch.cuda.synchronize()
        added[fused] = torch.cuda.max_memory_allocated() - base
        q.zero_grad(set_to_none=True)
        feat.grad = None
    print(f"peak added: fused {added[True] / 2 ** 20:.1f} MiB, composed {added[False] / 2 ** 20:.1f} MiB, "
          f"one [E, 2 in] tensor {one / 2 ** 20:.1f} MiB")
    assert added[True] < one / 4
    assert added[False] > one


def _composed_lines(q_a, graph, feat):
    """stag/models.py:7-25 as written."""
    n, E = graph.number_of_nodes(), graph.number_of_edges()
    fake_src = torch.randint(high=n, size=[E], device=feat.device)
    fake_dst = torch.randint(high=n, size=[E], device=feat.device)
    h_fake = q_a.embedding_mlp(torch.cat([feat[fake_src], feat[fake_dst]], dim=-1))
    fake = {k: q_a.parameters_mlp[k](h_fake) for k in q_a.new_parameter_names}
    q_neg = q_a.base_distribution_class(
        **{k[4:] if k.startswith("log_") else k: (v.exp() if k.startswith("log_") else v) for k, v in fake.items()})
    nll = (-q_a.log_prob(torch.tensor(1.0, device=feat.device)) - q_neg.log_prob(torch.tensor(0.0, device=feat.device)))
    return nll.sum(dim=-1).mean()


class _Uniform(torch.distributions.Uniform):       # (torch's own keeps its constraints in a property)
    arg_constraints = {"low": torch.distributions.constraints.real, "high": torch.distributions.constraints.real}


@pytest.mark.parametrize("which", ["wide", "uniform"])
def test_other_distributions_keep_the_composed_route(which, monkeypatch):
    import stag_amd
    from stag_amd import models, ops

    def never(*a, **k):
        raise AssertionError("the fused route was entered")
    monkeypatch.setattr(ops, "CONTRASTIVE_FUSED", True)
    monkeypatch.setattr(ops, "contrastive_nll", never)
    g, feat = _graph_and_features(200, 1500, 16, 4, requires_grad=False)
    torch.manual_seed(0)
    if which == "wide":
        q = stag_amd.distributions.AmortizedDistribution(16, 4).to(_dev())
        assert ops.contrastive_why_not(q.condition(g, feat), g, feat) == "not narrow"
    else:
        q = stag_amd.distributions.AmortizedDistribution(16, 1, base_distribution_class=_Uniform).to(_dev())
        with torch.no_grad():       # 0 and 1 inside (low, high) for every edge
            for k, b in (("low", -8.0), ("high", 8.0)):
                q.parameters_mlp[k].weight.mul_(0.1)
                q.parameters_mlp[k].bias.fill_(b)
        assert ops.contrastive_why_not(q.condition(g, feat), g, feat) == "base distribution"
    torch.manual_seed(31)
    got = models.nll_contrastive(q, g, feat)
    torch.manual_seed(31)
    ref = _composed_lines(q, g, feat)
    assert math.isfinite(float(ref.detach()))
    assert_close(got.reshape(1), ref.detach().reshape(1).cpu().numpy(), what=which)
