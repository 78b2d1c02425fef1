"""reorder_graph on the device.

Identity: a graph relabelled with noise="original" returns the rows of the original graph BIT FOR BIT, in the new order,
with the same seeds — the forward of every aggregation entry, dx of the backward, the GAT forward.  Sums over ALL edges
whose partials are added in plan order (vi=True parameter gradients, the GAT's d el / d er / d ft, which ride through
other row orders) are compared with the suite's 1e-5 instead.  The graph is random_graph(600, 5000, hub=300): a
segmented hub row, rows past HEAVY_LEN, duplicate edges and a row without in-edges, under a random permutation.

"locality": on a planted-partition multigraph with scrambled ids the proposed order must lift the stripe locality from
a random graph's 1/8 past 0.5 — twice what switches the XCD-aware order on — deterministically, and the switch must
not change one bit."""
import importlib

import numpy as np
import pytest
import torch

from util import TOL, assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu

N, E, HUB = 600, 5000, 300
_CACHE = {}


def _pair(dev, noise="original"):
    import stag_amd
    if noise not in _CACHE:
        g = _CACHE.get("g")
        if g is None:
            g = _CACHE["g"] = random_graph(N, E, 11, hub=HUB, device=dev)
        perm = torch.from_numpy(np.random.default_rng(12).permutation(N)).to(dev)
        _CACHE[noise] = stag_amd.reorder_graph(g, "custom", {"nodes_perm": perm}, noise=noise)
    return _CACHE["g"], _CACHE[noise]


def _rand(dev, *shape, seed=0, lo=None):
    t = torch.from_numpy(np.random.default_rng(seed + 17 * len(shape) + sum(shape)).standard_normal(shape).astype(np.float32))
    if lo is not None:
        t = t.abs() + lo
    return t.to(dev)


def _weights(case, D, n_edges, dev):
    """case -> f(graph) building the edge weight of ops.aggregate for that graph: the same draws / tensors on both."""
    import stag_amd
    from stag_amd import _lib
    EN = stag_amd.EdgeNoise
    kw = dict(seed=91, offset=5)
    if case == "none":
        return lambda g: None
    if case == "normal":
        return lambda g: EN(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, **kw)
    if case == "normal_relu_innorm":
        return lambda g: EN(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, relu=True, in_norm=True, **kw)
    if case == "uniform_per_channel":
        lo, hi = _rand(dev, D, seed=1, lo=0.1), _rand(dev, D, seed=2, lo=1.5)
        return lambda g: EN(g, D, _lib.NOISE_UNIFORM, lo, hi, **kw)
    if case == "bernoulli":
        return lambda g: EN(g, D, _lib.NOISE_BERNOULLI, 0.7, None, **kw)
    if case == "explicit":
        w = _rand(dev, n_edges, D, seed=3)
        return lambda g: w
    if case == "per_edge1":
        loc, scale = _rand(dev, n_edges, 1, seed=4), _rand(dev, n_edges, 1, seed=5, lo=0.2)
        return lambda g: EN(g, D, _lib.NOISE_NORMAL, loc, scale, **kw)
    raise KeyError(case)


CASES = ["none", "normal", "normal_relu_innorm", "uniform_per_channel", "bernoulli", "explicit", "per_edge1"]
DRAWN = ["normal", "normal_relu_innorm", "uniform_per_channel", "bernoulli", "per_edge1"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("D", [8, 50, 128, 260])
def test_forward_identity(dev, D, case):
    from stag_amd import ops
    g, g2 = _pair(dev)
    perm = g2.node_perm
    x = _rand(dev, N, D)
    ss, ds = _rand(dev, N, seed=6, lo=0.5), _rand(dev, N, seed=7, lo=0.5)
    mk = _weights(case, D, g.number_of_edges(), dev)
    for reduce, scaled in (("sum", False), ("sum", True), ("mean", True)):
        a = dict(src_scale=ss, dst_scale=ds) if scaled else {}
        b = dict(src_scale=ss[perm], dst_scale=ds[perm]) if scaled else {}
        out1 = ops.aggregate(g, x, mk(g), reduce=reduce, **a)
        out2 = ops.aggregate(g2, g2.rows_from_original(x), mk(g2), reduce=reduce, **b)
        assert torch.equal(g2.rows_to_original(out2), out1), (case, D, reduce, scaled)
        assert torch.isfinite(out1).all()


def test_forward_identity_mc_half_max(dev):
    from stag_amd import ops
    g, g2 = _pair(dev)
    D = 128
    x = _rand(dev, N, D)
    x2 = g2.rows_from_original(x)
    mk = _weights("normal", D, g.number_of_edges(), dev)
    mc1, mc2 = ops.aggregate_mc(g, x, mk(g), 3), ops.aggregate_mc(g2, x2, mk(g2), 3)
    assert mc1.shape == (3, N, D) and torch.equal(mc2[:, g2.node_inv], mc1)
    for kind in ("none", "normal"):                                        # bf16 rows: stag_agg_fwd_half
        mk = _weights(kind, D, g.number_of_edges(), dev)
        assert ops.half_rows_ok(x.bfloat16(), None, mk(g2), False, g2)
        h1, h2 = ops.aggregate(g, x.bfloat16(), mk(g)), ops.aggregate(g2, x2.bfloat16(), mk(g2))
        assert torch.equal(g2.rows_to_original(h2), h1)
    for kind in ("none", "normal", "explicit"):
        mk = _weights(kind, D, g.number_of_edges(), dev)
        m1, m2 = ops.aggregate_max(g, x, mk(g)), ops.aggregate_max(g2, x2, mk(g2))
        assert torch.equal(g2.rows_to_original(m2), m1), kind


@pytest.mark.parametrize("case", DRAWN)
@pytest.mark.parametrize("D", [50, 128])
def test_backward_identity_dx(dev, D, case):
    from stag_amd import ops
    g, g2 = _pair(dev)
    x = _rand(dev, N, D)
    G = _rand(dev, N, D, seed=8)
    mk = _weights(case, D, g.number_of_edges(), dev)
    x1 = x.clone().requires_grad_(True)
    ops.aggregate(g, x1, mk(g)).backward(G)
    x2 = g2.rows_from_original(x).clone().requires_grad_(True)
    ops.aggregate(g2, x2, mk(g2)).backward(g2.rows_from_original(G))
    assert torch.equal(g2.rows_to_original(x2.grad), x1.grad), (case, D)
    assert float(x1.grad.abs().max()) > 0


@pytest.mark.parametrize("kind", ["none", "normal"])
def test_backward_identity_max(dev, kind):
    from stag_amd import ops
    g, g2 = _pair(dev)
    D = 128
    x, G = _rand(dev, N, D), _rand(dev, N, D, seed=8)
    mk = _weights(kind, D, g.number_of_edges(), dev)
    x1 = x.clone().requires_grad_(True)
    ops.aggregate_max(g, x1, mk(g)).backward(G)
    x2 = g2.rows_from_original(x).clone().requires_grad_(True)
    ops.aggregate_max(g2, x2, mk(g2)).backward(g2.rows_from_original(G))
    assert torch.equal(g2.rows_to_original(x2.grad), x1.grad)


@pytest.mark.parametrize("D", [50, 128])
def test_backward_vi_parameter_gradients(dev, D):
    """vi=True: dx is a row's own sum (bits); the parameter gradients are sums over ALL edges whose block partials are
    added in plan order, which a relabelling changes: the suite's 1e-5."""
    import stag_amd
    from stag_amd import _lib, ops
    g, g2 = _pair(dev)
    x, G = _rand(dev, N, D), _rand(dev, N, D, seed=8)
    res = []
    for gr, to in ((g, lambda t: t), (g2, g2.rows_from_original)):
        loc = torch.full((D,), 1.0, device=dev, requires_grad=True)
        scale = torch.full((D,), 0.5, device=dev, requires_grad=True)
        xi = to(x).clone().requires_grad_(True)
        noise = stag_amd.EdgeNoise(gr, D, _lib.NOISE_NORMAL, loc, scale, seed=91, offset=5, differentiable=True)
        ops.aggregate(gr, xi, noise).backward(to(G))
        res.append((xi.grad, loc.grad, scale.grad))
    assert torch.equal(g2.rows_to_original(res[1][0]), res[0][0])
    for i, name in ((1, "d loc"), (2, "d scale")):
        assert_close(res[1][i], res[0][i].cpu().numpy(), what=f"vi {name} D={D}")


@pytest.mark.parametrize("H,F", [(4, 8), (8, 32)])
def test_gat_identity(dev, H, F):
    import stag_amd
    from stag_amd import _lib, ops
    g, g2 = _pair(dev)
    el0, er0, ft0 = _rand(dev, N, H, seed=1), _rand(dev, N, H, seed=2), _rand(dev, N, H, F, seed=3)
    G = _rand(dev, N, H, F, seed=4)
    drop = (0.6, 77, 3)
    res = []
    for gr, to in ((g, lambda t: t), (g2, g2.rows_from_original)):
        el, er, ft = (to(t).clone().requires_grad_(True) for t in (el0, er0, ft0))
        noise = stag_amd.EdgeNoise(gr, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=91, offset=5)
        out = ops.gat_aggregate(gr, el, er, ft, 0.2, noise, attn_drop=drop)
        out.backward(to(G))
        res.append((out.detach(), el.grad, er.grad, ft.grad))
    back = g2.rows_to_original
    assert torch.equal(back(res[1][0]), res[0][0])
    for i, name in ((1, "d el"), (2, "d er"), (3, "d ft")):
        assert_close(back(res[1][i]), res[0][i].cpu().numpy(), what=f"GAT {H}x{F} {name}")
        assert float(res[0][i].abs().max()) > 0


def test_own_keying_against_the_oracle(dev, oracle):
    """noise="own": the graph draws by its own positions, like any graph built from its edge list."""
    import stag_amd
    from stag_amd import _lib, ops
    g, g2 = _pair(dev, noise="own")
    assert g2.csr.nidx is None
    D = 128
    x = _rand(dev, N, D)
    noise = stag_amd.EdgeNoise(g2, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=91, offset=5)
    got = ops.aggregate(g2, x, noise)
    spec = oracle.make_spec("normal", 1.0, 0.5, seed=91, offset=5, Dn=D, n_edges=g2.number_of_edges())
    with hw_normals(oracle, dev):
        ref = oracle.agg_fwd(oracle_graph(oracle, g2), x.cpu().numpy(), spec)
    assert_close(got, ref, tol=TOL, what="own keying vs oracle")
    moved = stag_amd.reorder_graph(g, "custom", {"nodes_perm": g2.node_perm.cpu()}, noise="original").to("cpu").to(dev)
    assert moved.noise_keying == "original" and torch.equal(moved.csr.nidx, _pair(dev)[1].csr.nidx)   # .to() carries the keying


def planted_graph(n, e, k, p_in, hub, seed, device=None):
    """Planted-partition multigraph: every node gets a community uniformly at random (so ids carry no structure), every
    edge a uniform destination and, with probability p_in, a source from the destination's community, else a uniform one;
    the first `hub` edges are redirected into one row."""
    import stag_amd
    rng = np.random.default_rng(seed)
    comm = rng.integers(0, k, n)
    dst = rng.integers(0, n, e)
    src = rng.integers(0, n, e)
    inside = rng.random(e) < p_in
    for c in range(k):
        members = np.nonzero(comm == c)[0]
        sel = inside & (comm[dst] == c)
        if len(members) and sel.any():
            src[sel] = rng.choice(members, int(sel.sum()))
    dst[:hub] = int(rng.integers(0, n))
    return stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=device)


def test_locality_order_lifts_stripe_locality(dev, monkeypatch):
    import stag_amd
    from stag_amd import _lib, ops
    gm = importlib.import_module("stag_amd.graph")
    n, D = 4096, 128
    g = planted_graph(n, 32768, 16, 0.9, 300, seed=1, device=dev)
    g2 = stag_amd.reorder_graph(g, "locality", seed=0)
    again = stag_amd.reorder_graph(g, "locality", seed=0)
    perm, inv = g2.node_perm, g2.node_inv
    assert torch.equal(torch.sort(perm).values, torch.arange(n, device=dev))
    assert torch.equal(inv[perm], torch.arange(n, device=dev))
    assert torch.equal(again.node_perm, perm)
    loc0, loc1, loc1t = g.csr.stripe_locality(), g2.csr.stripe_locality(), g2.csr_t.stripe_locality()
    print(f"stripe locality: scrambled {loc0:.3f}, reordered {loc1:.3f} (csr) {loc1t:.3f} (csr_t)")
    assert loc0 < 0.2
    assert loc1 >= 0.5 and loc1t >= 0.5
    # "auto": the reordered graph earns the XCD-aware order, the scrambled one does not; no bit changes
    monkeypatch.setattr(gm, "XCD_ORDER", "auto")
    x = _rand(dev, n, D)
    x2 = g2.rows_from_original(x)
    outs = {}
    for name, gr, xi in (("g", g, x), ("g2", g2, x2)):
        noise = stag_amd.EdgeNoise(gr, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=91, offset=5)
        first = ops.aggregate(gr, xi, noise)
        assert not gr.csr._plans[gm.DEFAULT_SEG_LEN].get("xcd_on")
        for _ in range(gm.XCD_AFTER_LAUNCHES):
            last = ops.aggregate(gr, xi, noise)
        outs[name] = (first, last)
    assert g2.csr._plans[gm.DEFAULT_SEG_LEN].get("xcd_on") and not g.csr._plans[gm.DEFAULT_SEG_LEN].get("xcd_on")
    assert torch.equal(outs["g2"][0], outs["g2"][1])
    assert torch.equal(g2.rows_to_original(outs["g2"][1]), outs["g"][1])


@pytest.mark.parametrize("shape", ["no_edges", "one_node", "isolated_and_loops"])
def test_edge_cases(dev, shape):
    import stag_amd
    from stag_amd import _lib, ops
    if shape == "no_edges":
        n, src, dst = 5, np.zeros(0, np.int64), np.zeros(0, np.int64)
    elif shape == "one_node":
        n, src, dst = 1, np.zeros(3, np.int64), np.zeros(3, np.int64)
    else:
        rng = np.random.default_rng(3)
        n = 50
        src = np.concatenate([rng.integers(0, 20, 80), np.arange(10, 30)])        # nodes 30 .. 49 are isolated
        dst = np.concatenate([rng.integers(0, 20, 80), np.arange(10, 30)])        # ... and 10 .. 29 carry a self-loop
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    D = 8
    x = _rand(dev, n, D)
    for algo, cfg in (("locality", None), ("custom", {"nodes_perm": torch.randperm(n)})):
        g2 = stag_amd.reorder_graph(g, algo, cfg)
        assert torch.equal(torch.sort(g2.node_perm).values, torch.arange(n, device=dev))
        assert torch.equal(g2.node_inv[g2.node_perm], torch.arange(n, device=dev))
        mk = _weights("normal", D, len(src), dev)
        out1 = ops.aggregate(g, x, mk(g))
        out2 = ops.aggregate(g2, g2.rows_from_original(x), mk(g2))
        assert torch.equal(g2.rows_to_original(out2), out1), (shape, algo)


def test_two_layer_gcn_end_to_end(dev):
    """A two-layer StagLayer(GCN) model, eval with n_samples = 4 and the same generator seeds, on g and on the reordered
    graph with permuted features: the aggregations are the same bits, the GEMMs between them are not promised bitwise."""
    import stag_amd
    L, Z = stag_amd.layers, stag_amd.zoo
    g, g2 = _pair(dev)
    D = 32
    torch.manual_seed(3)
    layers = torch.nn.ModuleList([
        L.StagLayer(Z.GCN(D, 16, activation=torch.relu), q_a=torch.distributions.Normal(1.0, 0.5)),
        L.StagLayer(Z.GCN(16, 5, activation=lambda t: torch.softmax(t, -1)), q_a=torch.distributions.Normal(1.0, 0.3))])
    model = stag_amd.models.StagModel(layers).to(dev).eval()
    x = _rand(dev, N, D)
    with torch.no_grad():
        stag_amd.manual_seed(1234)
        y1 = model(g, x, n_samples=4, return_parameters=True)
        stag_amd.manual_seed(1234)
        y2 = model(g2, g2.rows_from_original(x), n_samples=4, return_parameters=True)
    assert y1.shape == (N, 5)
    assert_close(g2.rows_to_original(y2), y1.cpu().numpy(), what="two-layer GCN on the reordered graph")
