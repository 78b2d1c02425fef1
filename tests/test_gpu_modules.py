"""The drop-in layer API on the GPU against fixtures computed by the reference's own
source (tests/golden/make_golden.py), plus the reference's shape contracts
(stag/tests/test_layers.py) and full-size, size-independent properties."""
import numpy as np
import pytest
import torch

from util import TOL, assert_close, oracle_graph, scaled_err

pytestmark = pytest.mark.gpu


def _graph(golden, name, dev):
    import stag_amd
    return stag_amd.Graph(torch.from_numpy(golden[f"{name}_src"]), torch.from_numpy(golden[f"{name}_dst"]),
                          int(golden[f"{name}_n"]), device=dev)


def _sd(golden, prefix, dev):
    return {k[len(prefix):]: torch.from_numpy(golden[k]).to(dev) for k in golden.files if k.startswith(prefix)}


# ---- reference shape contracts (stag/tests/test_layers.py:13-54) ------------------------------
@pytest.mark.parametrize("mode", ["r1", "rc", "re", "rec"])
def test_forward_shapes_like_reference_tests(dev, mode):
    import stag_amd
    q = {"r1": None,
         "rc": torch.distributions.Normal(torch.ones(16), torch.ones(16)),
         "re": stag_amd.distributions.AmortizedDistribution(16, 1),
         "rec": stag_amd.distributions.AmortizedDistribution(16, 16)}[mode]
    layer = stag_amd.zoo.GCN(16, 32)
    layer = stag_amd.layers.StagLayer(layer) if q is None else stag_amd.layers.StagLayer(layer, q_a=q)
    layer = layer.to(dev)
    g = stag_amd.rand_graph(3, 9, device=dev)
    h = layer(g, torch.randn(3, 16, device=dev))
    assert h.shape == torch.Size([3, 32])
    assert layer._edge_weight_sample.shape == (9, 16)


def test_layer_golden_with_injected_weights(dev, golden):
    """StagLayer over a sum aggregator: hand the reference's sampled w to the explicit-weight
    kernel and compare with the reference's layer output."""
    from stag_amd import ops
    for name in golden["layer_cases"]:
        name = str(name)
        g = _graph(golden, name.split("_")[1], dev)
        x = torch.from_numpy(golden[name + "_x"]).to(dev)
        w = torch.from_numpy(golden[name + "_w"]).to(dev)
        assert_close(ops.aggregate(g, x, w), golden[name + "_out"], what=name)
        # the DGL-style call the reference makes: update_all(u_mul_e, sum)
        import stag_amd.function as fn
        h = g.local_var()
        h.ndata["h"], h.edata["w"] = x, w
        h.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("m", "out"))
        assert_close(h.ndata["out"], golden[name + "_out"], what=name + " update_all")


def test_in_norm_tensor_path_golden(dev, golden):
    from stag_amd.layers import _in_norm
    for name in golden["layer_cases"]:
        name = str(name)
        if name.endswith("_bern"):
            g = _graph(golden, name.split("_")[1], dev)
            w_final = golden[name + "_w"]
            w_raw = torch.from_numpy((w_final != 0).astype(np.float32)).to(dev)
            assert_close(_in_norm(g, w_raw), w_final, what=name)


def test_gcn_sage_gat_modules_golden(dev, golden):
    import stag_amd
    g = _graph(golden, "hub40", dev)
    x = torch.from_numpy(golden["zoo_x"]).to(dev)
    w = torch.from_numpy(golden["zoo_w"]).to(dev)
    gcn = stag_amd.zoo.GCN(16, 8).to(dev)
    gcn.load_state_dict({"weight": torch.from_numpy(golden["gcn_weight"]), "bias": torch.from_numpy(golden["gcn_bias"])})
    assert_close(gcn(g, x, edge_weight=w), golden["gcn_out"], what="GCN")
    assert_close(gcn(g, x), golden["gcn_out_noweight"], what="GCN no weight")
    sage = stag_amd.zoo.GraphSAGE(16, 8, activation=torch.relu).to(dev)
    sage.load_state_dict(_sd(golden, "sage_sd_", dev))
    assert_close(sage(g, x, edge_weight=w), golden["sage_out"], what="GraphSAGE")
    for tag, last in (("gat", False), ("gat_last", True)):
        gat = stag_amd.zoo.GAT(16, 4, num_heads=3, last=last).to(dev)
        gat.load_state_dict(_sd(golden, tag + "_sd_", dev))
        out, attn = gat(g, x, get_attention=True, edge_weight=torch.from_numpy(golden[tag + "_w"]).to(dev))
        assert_close(out, golden[tag + "_out"], what=tag)
        assert_close(attn, golden[tag + "_attn"], what=tag + " attention")


def test_gcn_sage_gat_module_gradients_golden(dev, golden):
    """The reference's own autograd gradients (tests/golden/make_golden.py (e): loss = <gout, layer(g, x, edge_weight=w)>
    through stag/zoo/gcn.py:58-116, graph_sage.py:44-119, gat.py:74-149) against the HIP backward paths: d x, d w and
    every parameter gradient of zoo.GCN, zoo.GraphSAGE and zoo.GAT (both `last` modes)."""
    import stag_amd
    g = _graph(golden, "hub40", dev)

    def check(tag, layer, w_key):
        x = torch.from_numpy(golden["zoo_x"]).to(dev).requires_grad_(True)
        w = torch.from_numpy(golden[w_key]).to(dev).requires_grad_(True)
        out = layer(g, x, edge_weight=w)
        (out * torch.from_numpy(golden[f"{tag}_gout"]).to(dev)).sum().backward()
        for name, got in [("x", x.grad), ("w", w.grad)] + [(k, p.grad) for k, p in layer.named_parameters()]:
            ref = golden[f"{tag}_grad_{name}"]
            sc = max(1.0, float(np.abs(ref).max()))
            assert_close(got.reshape(ref.shape) / sc, ref / sc, what=f"{tag} d {name}")

    gcn = stag_amd.zoo.GCN(16, 8).to(dev)
    gcn.load_state_dict({"weight": torch.from_numpy(golden["gcn_weight"]), "bias": torch.from_numpy(golden["gcn_bias"])})
    check("gcn", gcn, "zoo_w")
    sage = stag_amd.zoo.GraphSAGE(16, 8, activation=torch.relu).to(dev)
    sage.load_state_dict(_sd(golden, "sage_sd_", dev))
    check("sage", sage, "zoo_w")
    for tag, last in (("gat", False), ("gat_last", True)):
        gat = stag_amd.zoo.GAT(16, 4, num_heads=3, last=last).to(dev)
        gat.load_state_dict(_sd(golden, tag + "_sd_", dev))
        check(tag, gat, tag + "_w")


def test_gated_gcn_module_golden(dev, golden):
    """zoo.GatedGCN against the reference's own forward (stag/zoo/gated_gcn.py:25-55)."""
    import stag_amd
    g = _graph(golden, "hub40", dev)
    x = torch.from_numpy(golden["zoo_x"]).to(dev)
    w = torch.from_numpy(golden["zoo_w"]).to(dev)
    for weighted, key in ((True, "gated_out"), (False, "gated_out_noweight")):
        layer = stag_amd.zoo.GatedGCN(16, 16, dropout=0.0, batch_norm=True, residual=True).to(dev)
        layer.load_state_dict(_sd(golden, "gated_sd_", dev))
        layer.train()
        assert_close(layer(g, x, edge_weight=w) if weighted else layer(g, x), golden[key], what=key)
    layer = stag_amd.zoo.GatedGCN(16, 8, batch_norm=False, residual=True).to(dev)
    layer.load_state_dict(_sd(golden, "gated3_sd_", dev))
    assert layer.residual is False
    assert_close(layer(g, x), golden["gated3_out_noweight"], what="gated 16->8")


def test_stag_model_loss_and_grads_golden(dev, golden, monkeypatch):
    """2-layer vi=True GCN stack: NLL, KL and gradients equal the reference's when the layers
    are fed the reference's sampled weights (stag/models.py:63-85)."""
    import stag_amd
    g = _graph(golden, "hub40", dev)
    x = torch.from_numpy(golden["zoo_x"]).to(dev)
    y = torch.from_numpy(golden["model_y"]).to(dev)
    N = torch.distributions.Normal
    l1 = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(16, 8, activation=torch.relu), q_a=N(1.0, 0.4), vi=True)
    l2 = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(8, 4, activation=lambda t: torch.softmax(t, dim=-1)),
                                   q_a=N(1.0, 0.4), vi=True)
    model = stag_amd.models.StagModel(layers=torch.nn.ModuleList([l1, l2]), kl_scaling=0.5).to(dev)
    for i, l in enumerate((l1, l2)):
        l.base_layer.load_state_dict({"weight": torch.from_numpy(golden[f"model_l{i}_weight"]),
                                      "bias": torch.from_numpy(golden[f"model_l{i}_bias"])})
    # replay the reference's draws: z = (w - loc) / scale, then w = loc + scale * z in-graph
    for l, key in ((l1, "model_w1"), (l2, "model_w2")):
        z = (torch.from_numpy(golden[key]).to(dev) - 1.0) / 0.4
        monkeypatch.setattr(l, "rsample_noise",
                            lambda graph, dn, l=l, z=z: l.q_a.loc + l.q_a.log_scale.exp() * z)
    nll, reg = model.loss_terms(g, x, y, n_samples=1)
    assert_close(torch.stack([nll, reg]), golden["model_nll_reg"], what="nll, reg")
    (nll + reg).backward()
    assert_close(l1.base_layer.weight.grad, golden["model_l0_weight_grad"], what="dL/dW0")
    assert_close(l1.q_a.loc.grad, golden["model_l0_qa_loc_grad"], what="dL/dloc")
    assert_close(l1.q_a.log_scale.grad, golden["model_l0_qa_log_scale_grad"], what="dL/dlog_scale")


def test_fused_layer_equals_materialised_layer(dev, oracle):
    """The fused path and `_edge_weight_sample` describe the same draw."""
    import stag_amd
    from stag_amd import ops
    from util import random_graph
    g = random_graph(300, 4000, seed=5, hub=700, device=dev)
    x = torch.randn(300, 32, device=dev)
    for kw in (dict(q_a=torch.distributions.Normal(1.0, 0.5)),
               dict(q_a=torch.distributions.Normal(0.2, 1.0), relu=True),
               dict(q_a=torch.distributions.Bernoulli(probs=0.7), norm=True),
               dict(q_a=torch.distributions.Uniform(0.5, 1.5))):
        for base in (stag_amd.zoo.GCN(32, 16), stag_amd.zoo.GraphSAGE(32, 16), stag_amd.zoo.GIN(32, 16)):
            layer = stag_amd.layers.StagLayer(base, **kw).to(dev)
            stag_amd.manual_seed(42)
            out = layer(g, x)
            w = layer._edge_weight_sample                    # materialised on demand
            assert w.shape == (g.number_of_edges(), 32)
            assert_close(base(g, x, edge_weight=w), out.detach().cpu().numpy(), what=f"{type(base).__name__} {kw}")
            stag_amd.manual_seed(42)
            assert torch.equal(layer(g, x), out), "same seed => same bits"
            assert not torch.equal(layer(g, x), out), "next forward draws fresh noise"


def test_fuzz_layers_equal_their_materialised_form(dev):
    """Seeded sweep of test_fused_layer_equals_materialised_layer over graphs x widths x base layers (GCN, GraphSAGE,
    GIN, GAT) x q_a (Normal, Normal + relu, Bernoulli + in-norm, Uniform) x vi: the layer's fused forward, d x and
    the base layer's parameter gradients equal the base layer called with the weights the layer reports in
    `_edge_weight_sample` (stag/layers.py:107-113) — the explicit-weight kernels, a different code path end to end."""
    import os
    import stag_amd
    from util import random_graph
    rng = np.random.default_rng(20261009)
    N, B, U = torch.distributions.Normal, torch.distributions.Bernoulli, torch.distributions.Uniform
    qs = [lambda: dict(q_a=N(1.0, 0.5)), lambda: dict(q_a=N(0.2, 1.0), relu=True),
          lambda: dict(q_a=B(probs=0.7), norm=True), lambda: dict(q_a=U(0.5, 1.5))]
    for it in range(16 * max(1, int(os.environ.get("STAG_FUZZ_SCALE", "1")))):
        n = int(rng.integers(20, 500))
        g = random_graph(n, int(rng.integers(1, 5000)), seed=12000 + it, hub=int(rng.choice([0, 0, 100, 800])), device=dev)
        din, dout = int(rng.choice([1, 3, 8, 32, 50, 128, 200])), int(rng.choice([1, 7, 16, 40]))
        which, qi = it % 4, int(rng.integers(0, 4))
        vi = bool(rng.random() < 0.4) and qi != 2                  # (Bernoulli has no rsample)
        torch.manual_seed(it)
        H = int(rng.choice([1, 2, 4, 8]))
        base = [lambda: stag_amd.zoo.GCN(din, dout, allow_zero_in_degree=True), lambda: stag_amd.zoo.GraphSAGE(din, dout),
                lambda: stag_amd.zoo.GIN(din, dout),
                lambda: stag_amd.zoo.GAT(din, dout, num_heads=H, allow_zero_in_degree=True)][which]()
        kw = qs[qi]()
        layer = stag_amd.layers.StagLayer(base, vi=vi, **kw).to(dev)
        what = f"layer fuzz {it}: n={n} E={g.number_of_edges()} {type(base).__name__} {din}->{dout} q={qi} vi={vi}" + (f" H={H}" if which == 3 else "")
        x = torch.tensor(rng.standard_normal((n, din)).astype(np.float32), device=dev, requires_grad=True)
        stag_amd.manual_seed(1000 + it)
        out = layer(g, x)
        gout = torch.tensor(rng.standard_normal(tuple(out.shape)).astype(np.float32), device=dev)
        out.backward(gout)
        w = layer._edge_weight_sample.detach()
        assert w.shape == (g.number_of_edges(), H if which == 3 else din), what
        grads = {k: p.grad.clone() for k, p in base.named_parameters() if p.grad is not None}
        base.zero_grad(set_to_none=True)
        x2 = x.detach().clone().requires_grad_(True)
        out2 = base(g, x2, edge_weight=w)
        out2.backward(gout)
        assert_close(out, out2.detach().cpu().numpy(), what=what + " out")
        sc = max(1.0, float(x2.grad.abs().max()))
        assert_close(x.grad / sc, (x2.grad / sc).cpu().numpy(), what=what + " dx")
        for k, p in base.named_parameters():
            if p.grad is None:
                continue
            sc = max(1.0, float(p.grad.abs().max()))
            assert_close(grads[k] / sc, (p.grad / sc).cpu().numpy(), what=what + f" d {k}")


def test_training_step_reduces_loss(dev):
    """End to end: 3-layer GCN stack of scripts/arxiv_mle/gcn/run.py shape, Adam steps."""
    import stag_amd
    from util import random_graph
    torch.manual_seed(0)
    g = random_graph(400, 4000, seed=9, device=dev)
    x = torch.randn(400, 32, device=dev)
    y = torch.randint(0, 5, (400,), device=dev)
    q = torch.distributions.Normal(1.0, 0.3)
    L, Z = stag_amd.layers, stag_amd.zoo
    layers = torch.nn.ModuleList([
        L.StagLayer(Z.GCN(32, 32), q_a=q),
        L.FeatOnlyLayer(torch.nn.Sequential(torch.nn.BatchNorm1d(32), torch.nn.ReLU())),
        L.StagLayer(Z.GCN(32, 32), q_a=q),
        L.FeatOnlyLayer(torch.nn.Sequential(torch.nn.BatchNorm1d(32), torch.nn.ReLU())),
        L.StagLayer(Z.GCN(32, 5, activation=lambda t: torch.softmax(t, dim=-1)), q_a=q)])
    model = stag_amd.models.StagModel(layers=layers).to(dev)
    opt = torch.optim.Adam(model.parameters(), 1e-2)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = model.loss(g, x, y, n_samples=2)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] - 0.05
    with torch.no_grad():
        p = model(g, x, n_samples=4, return_parameters=True)
    assert p.shape == (400, 5) and torch.allclose(p.sum(-1), torch.ones(400, device=dev), atol=1e-4)


def test_readout_layers(dev, oracle):
    import stag_amd
    gs = [stag_amd.rand_graph(n, 3 * n, device=dev) for n in (5, 1, 9)]
    b = stag_amd.batch(gs)
    x = torch.randn(15, 7, device=dev, requires_grad=True)
    for layer, red in ((stag_amd.layers.SumNodes(), oracle.REDUCE_SUM), (stag_amd.layers.MeanNodes(), oracle.REDUCE_MEAN)):
        out = layer(b, x)
        assert_close(out, oracle.segment_reduce(x.detach().cpu().numpy(), np.array([0, 5, 6, 15], np.int32), red))
        out.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape


def test_shard_equals_whole_graph(dev):
    """world=1 GraphShard == Graph, and a 2-way split computed on one GPU reproduces the
    whole-graph result bit for bit (global Philox positions)."""
    import stag_amd
    from stag_amd import _lib, ops
    from stag_amd.partition import GraphShard
    rng = np.random.default_rng(3)
    n, D = 500, 128
    dst = np.concatenate([rng.integers(0, n, 6000), np.full(900, 17)])
    src = rng.integers(0, n, len(dst))
    x = torch.randn(n, D, device=dev)
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    mk = lambda graph: stag_amd.EdgeNoise(graph, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=8, offset=3)
    whole = ops.aggregate(g, x, mk(g))
    sh = GraphShard(src, dst, n, 0, 1, device=dev)
    assert torch.equal(sh.aggregate(x, mk(sh)), whole)
    for world in (2, 3):
        parts, parts_halo = [], []
        for r in range(world):
            sh = GraphShard(src, dst, n, r, world, device=dev, exchange="allgather")
            buf = torch.zeros(world * sh.max_rows, D, device=dev)      # what the all-gather would deliver
            for q in range(world):
                lo, hi = int(sh.bounds[q]), int(sh.bounds[q + 1])
                buf[q * sh.max_rows:q * sh.max_rows + hi - lo] = x[lo:hi]
            noise = mk(sh)
            noise.pos_base = sh.pos_base
            parts.append(ops.aggregate(sh, buf, noise, _gathered=True))
            hs = GraphShard(src, dst, n, r, world, device=dev, exchange="halo")
            buf = torch.cat([x[hs.row_lo:hs.row_hi], x[torch.from_numpy(hs.recv_ids).to(dev)]], 0)   # all-to-all result
            assert buf.shape[0] == hs.n_buf
            noise = mk(hs)
            noise.pos_base = hs.pos_base
            parts_halo.append(ops.aggregate(hs, buf, noise, _gathered=True))
        assert torch.equal(torch.cat(parts, 0), whole)
        assert torch.equal(torch.cat(parts_halo, 0), whole)
    # channel shards: whole CSR on every rank, D/P channels each, no exchange; per-channel params follow
    from stag_amd.partition import ChannelShard
    loc, scale = torch.rand(D, device=dev) + 0.5, torch.rand(D, device=dev) * 0.5 + 0.1
    whole_pc = ops.aggregate(g, x, stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, loc, scale, seed=8, offset=3, relu=True))
    whole_bn = ops.aggregate(g, x, stag_amd.EdgeNoise(g, D, _lib.NOISE_BERNOULLI, 0.6, seed=8, offset=3, in_norm=True))
    for world in (2, 8, 3):
        cols, cols_pc, cols_bn = [], [], []
        for r in range(world):
            cs = ChannelShard(g, D, r, world)
            xc = cs.scatter_cols(x)
            cols.append(cs.aggregate(xc, stag_amd.EdgeNoise(g, cs.dn, _lib.NOISE_NORMAL, 1.0, 0.5, seed=8, offset=3)))
            cols_pc.append(cs.aggregate(xc, stag_amd.EdgeNoise(g, cs.dn, _lib.NOISE_NORMAL, loc[cs.c_lo:cs.c_hi],
                                                                 scale[cs.c_lo:cs.c_hi], seed=8, offset=3, relu=True)))
            cols_bn.append(cs.aggregate(xc, stag_amd.EdgeNoise(g, cs.dn, _lib.NOISE_BERNOULLI, 0.6, seed=8, offset=3,
                                                                 in_norm=True)))
        assert torch.equal(torch.cat(cols, 1), whole)
        assert torch.equal(torch.cat(cols_pc, 1), whole_pc)
        assert torch.equal(torch.cat(cols_bn, 1), whole_bn)
    # partitioned GAT (cfg5 shape of the exchange: ft and el, two tables of one step), 2 emulated ranks
    H, F = 8, 16
    el, er, ft = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev), torch.randn(n, H, F, device=dev)
    mkh = lambda graph: stag_amd.EdgeNoise(graph, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=9, offset=4)
    whole_gat = ops.gat_aggregate(g, el, er, ft, 0.2, mkh(g))
    parts = []
    for r in range(2):
        hs = GraphShard(src, dst, n, r, 2, device=dev, exchange="halo")
        ids = torch.cat([torch.arange(hs.row_lo, hs.row_hi, device=dev), torch.from_numpy(hs.recv_ids).to(dev)])
        hs.halo_gather_multi = lambda ts, ids=ids: [ft[ids], el[ids]]        # what the two-table exchange delivers
        parts.append(hs.gat_aggregate(el[hs.row_lo:hs.row_hi], er[hs.row_lo:hs.row_hi], ft[hs.row_lo:hs.row_hi],
                                      0.2, mkh(hs)))
    assert torch.equal(torch.cat(parts, 0), whole_gat)


def test_full_size_properties(dev):
    """BASELINE cfg2 size (N=169,343, E=1,166,243, D=128): properties that need no oracle run."""
    import stag_amd
    from stag_amd import _lib, ops, synthetic
    src, dst = synthetic.arxiv_like(seed=1)
    n = synthetic.ARXIV_NODES
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    D = 128
    gen = torch.Generator().manual_seed(123)           # seeded inputs: the same numbers on every run
    x = torch.randn(n, D, generator=gen).to(dev)
    y = torch.randn(n, D, generator=gen).to(dev)
    mk = lambda **kw: stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=0x5747A6, offset=0, **kw)
    a = ops.aggregate(g, x, mk())
    assert torch.equal(a, ops.aggregate(g, x, mk())), "deterministic"
    # linearity in x for a fixed noise field: three fp32 aggregations, one of them over inputs sqrt(5) times
    # larger, so the fp32 rounding of 13k-term sums shows up about 5 times (2 + 1 + sqrt 5) in the difference
    lin = ops.aggregate(g, 2.0 * x + y, mk())
    ref = 2.0 * a + ops.aggregate(g, y, mk())
    assert scaled_err(lin.cpu().numpy(), ref.cpu().numpy()) <= 5 * TOL
    # zero in-degree rows are exactly zero; noise-free aggregation of ones counts in-degrees
    deg = g.in_degrees()
    assert float(a[deg == 0].abs().max()) == 0.0
    ones = ops.aggregate(g, torch.ones(n, D, device=dev), None)
    assert torch.equal(ones[:, 0], deg.float()) and torch.equal(ones[:, 127], deg.float())
    # E[w] = 1: the noisy aggregate of ones is the in-degree up to sampling error
    noisy = ops.aggregate(g, torch.ones(n, D, device=dev), mk())
    hub = int(deg.argmax())
    assert abs(float(noisy[hub].mean()) / float(deg[hub]) - 1.0) < 5e-3
    # Bernoulli + in-norm: every destination's weights sum to its in-degree
    b = stag_amd.EdgeNoise(g, D, _lib.NOISE_BERNOULLI, 0.5, None, seed=1, offset=0, in_norm=True)
    s = ops.aggregate(g, torch.ones(n, D, device=dev), b)
    alive = s != 0
    assert scaled_err(s[alive].cpu().numpy(), deg.float().unsqueeze(1).expand(n, D)[alive].cpu().numpy()) <= TOL
    # backward = transpose: <A x, y> == <x, A^T y> with the same noise
    xr = x.clone().requires_grad_(True)
    out = ops.aggregate(g, xr, mk())
    out.backward(y)
    lhs, rhs = float((out.detach().double() * y.double()).sum()), float((x.double() * xr.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + abs(rhs))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pmode", ["scalar", "per_channel", "per_edge1", "per_edge"])
@pytest.mark.parametrize("kind", ["normal", "uniform"])
def test_fused_vi_gradients(dev, oracle, kind, pmode, relu):
    """vi=True on the fused path: gradients w.r.t. x and the distribution parameters equal those
    of the materialised reparameterisation w = p0 + p1 * z (the reference's rsample path), with
    nothing [E, D]-sized saved for the backward."""
    import stag_amd
    from stag_amd import _lib, ops
    from util import random_graph
    rng = np.random.default_rng(7)
    n, D = 150, 12
    g = random_graph(n, 1100, seed=31, hub=160, device=dev)
    E = g.number_of_edges()
    shape = {"scalar": (), "per_channel": (D,), "per_edge1": (E, 1), "per_edge": (E, D)}[pmode]
    a0 = torch.tensor(rng.uniform(0.5, 1.0, shape).astype(np.float32), device=dev)
    b0 = torch.tensor(rng.uniform(0.3, 0.8, shape).astype(np.float32), device=dev)
    if kind == "uniform":
        b0 = a0 + b0 + 0.5          # high > low
    x0 = torch.tensor(rng.standard_normal((n, D)).astype(np.float32), device=dev)
    gout = torch.tensor(rng.standard_normal((n, D)).astype(np.float32), device=dev)
    ss = torch.tensor(rng.uniform(0.5, 1.5, n).astype(np.float32), device=dev)
    ds = torch.tensor(rng.uniform(0.5, 1.5, n).astype(np.float32), device=dev)
    K = _lib.NOISE_NORMAL if kind == "normal" else _lib.NOISE_UNIFORM
    shift = -0.9 if relu else 0.0   # push a good share of the weights below zero under relu

    # fused
    x, a, b = (t.clone().requires_grad_(True) for t in (x0, a0, b0))
    noise = stag_amd.EdgeNoise(g, D, K, a + shift, b, relu=relu, seed=5, offset=2, differentiable=True)
    out = ops.aggregate(g, x, noise, reduce="mean", src_scale=ss, dst_scale=ds, seg_len=32)
    out.backward(gout)
    # materialised reparameterisation with the same standard draw
    std = stag_amd.EdgeNoise(g, D, K, 0.0, 1.0, seed=5, offset=2).materialize()
    x2, a2, b2 = (t.clone().requires_grad_(True) for t in (x0, a0, b0))
    w = (a2 + shift) + b2 * std if kind == "normal" else (a2 + shift) + (b2 - (a2 + shift)) * std
    if relu:
        w = w.relu()
    out2 = ops.aggregate(g, x2, w.expand(E, D), reduce="mean", src_scale=ss, dst_scale=ds, seg_len=32)
    out2.backward(gout)
    assert_close(out, out2.detach().cpu().numpy(), what="forward")
    assert_close(x.grad, x2.grad.cpu().numpy(), what="dx")
    assert_close(a.grad, a2.grad.cpu().numpy(), what=f"d p0 {pmode}")
    assert_close(b.grad, b2.grad.cpu().numpy(), what=f"d p1 {pmode}")
    # and against the oracle's statement of dw/dp (per-edge modes)
    if pmode == "per_edge":
        og = oracle_graph(oracle, g)
        gs = (gout * ds.unsqueeze(1) / g.in_degrees().clamp(min=1).unsqueeze(1)).cpu().numpy()
        spec = oracle.make_spec(kind, (a0 + shift).cpu().numpy(), b0.cpu().numpy(), relu=relu, seed=5, offset=2,
                                Dn=D, n_edges=E, deriv=2)
        ref = oracle.agg_bwd_w(og, x0.cpu().numpy(), gs, src_scale=ss.cpu().numpy(), spec=spec)
        assert_close(b.grad, ref, what="d p1 vs oracle")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pmode", ["scalar", "per_channel", "per_edge1", "per_edge"])
@pytest.mark.parametrize("kind", ["normal", "uniform"])
def test_fused_vi_gradients_with_in_norm(dev, kind, pmode, relu):
    """vi=True AND norm=True (stag/layers.py:102-105 on top of :123-124) on the fused path: the in-degree
    renormalisation s = indeg / sum_in(w) depends on the parameters through every weight of the row; its
    derivative comes from two [N, D] tensors (the factor and the output), not from an [E, D] graph.  Against
    autograd through the materialised statement: w = p0 + p1 z, relu, _in_norm, explicit-weight aggregation."""
    import stag_amd
    from stag_amd import _lib, ops
    from stag_amd.layers import _in_norm
    from util import random_graph
    rng = np.random.default_rng(17)
    n, D = 150, 12
    g = random_graph(n, 1100, seed=33, hub=160, device=dev)
    E = g.number_of_edges()
    shape = {"scalar": (), "per_channel": (D,), "per_edge1": (E, 1), "per_edge": (E, D)}[pmode]
    a0 = torch.tensor(rng.uniform(0.8, 1.2, shape).astype(np.float32), device=dev)
    b0 = torch.tensor(rng.uniform(0.2, 0.5, shape).astype(np.float32), device=dev)
    if kind == "uniform":
        b0 = a0 + b0 + 0.5
    x0 = torch.tensor(rng.standard_normal((n, D)).astype(np.float32), device=dev)
    gout = torch.tensor(rng.standard_normal((n, D)).astype(np.float32), device=dev)
    ss = torch.tensor(rng.uniform(0.5, 1.5, n).astype(np.float32), device=dev)
    ds = torch.tensor(rng.uniform(0.5, 1.5, n).astype(np.float32), device=dev)
    K = _lib.NOISE_NORMAL if kind == "normal" else _lib.NOISE_UNIFORM
    shift = -0.6 if relu else 0.0
    for reduce in ("sum", "mean"):
        x, a, b = (t.clone().requires_grad_(True) for t in (x0, a0, b0))
        noise = stag_amd.EdgeNoise(g, D, K, a + shift, b, relu=relu, in_norm=True, seed=5, offset=2, differentiable=True)
        out = ops.aggregate(g, x, noise, reduce=reduce, src_scale=ss, dst_scale=ds, seg_len=32)
        out.backward(gout)
        std = stag_amd.EdgeNoise(g, D, K, 0.0, 1.0, seed=5, offset=2).materialize()
        x2, a2, b2 = (t.clone().requires_grad_(True) for t in (x0, a0, b0))
        w = (a2 + shift) + b2 * std if kind == "normal" else (a2 + shift) + (b2 - (a2 + shift)) * std
        if relu:
            w = w.relu()
        w = _in_norm(g, w.expand(E, D))
        out2 = ops.aggregate(g, x2, w, reduce=reduce, src_scale=ss, dst_scale=ds, seg_len=32)
        out2.backward(gout)
        assert_close(out, out2.detach().cpu().numpy(), what=f"forward {reduce}")
        assert_close(x.grad, x2.grad.cpu().numpy(), what=f"dx {reduce}")
        for got, ref, nm in ((a.grad, a2.grad, "p0"), (b.grad, b2.grad, "p1")):
            sc = max(1.0, float(ref.abs().max()))
            assert_close(got / sc, (ref / sc).cpu().numpy(), what=f"d {nm} {pmode} {reduce}")
    # and the layer: vi + norm stays on the fused path, with gradients into loc / log_scale
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, 8), q_a=torch.distributions.Normal(1.0, 0.5), vi=True,
                                      norm=True, relu=relu).to(dev)
    y = layer(g, x0)
    assert isinstance(layer._edge_weight_handle, stag_amd.EdgeNoise) and layer._edge_weight_handle.in_norm
    y.square().mean().backward()
    assert layer.q_a.loc.grad is not None and float(layer.q_a.log_scale.grad.abs()) > 0


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pmode", ["scalar", "per_edge1", "per_edge"])
def test_log_scale_parameters(dev, oracle, pmode, relu):
    """stag_noise_spec.p1_log: the scale handed over as its logarithm (what AmortizedDistribution's `log_scale`
    head produces, stag/distributions.py:235-242) and exponentiated where the kernels load it.  Forward and the
    materialised field against the oracle, gradients w.r.t. x, loc and LOG-scale against autograd through
    w = loc + exp(log_scale) z."""
    import stag_amd
    from stag_amd import _lib, ops
    from util import random_graph
    rng = np.random.default_rng(23)
    n, D = 160, 12
    g = random_graph(n, 1200, seed=41, hub=170, device=dev)
    E = g.number_of_edges()
    shape = {"scalar": (), "per_edge1": (E, 1), "per_edge": (E, D)}[pmode]
    a0 = torch.tensor(rng.uniform(0.5, 1.0, shape).astype(np.float32), device=dev)
    l0 = torch.tensor(np.log(rng.uniform(0.3, 0.8, shape)).astype(np.float32), device=dev)
    x0 = torch.tensor(rng.standard_normal((n, D)).astype(np.float32), device=dev)
    gout = torch.tensor(rng.standard_normal((n, D)).astype(np.float32), device=dev)
    shift = -0.9 if relu else 0.0
    og = oracle_graph(oracle, g)
    p0n, p1n = (a0 + shift).cpu().numpy(), l0.cpu().numpy()
    if pmode == "scalar":
        p0n, p1n = float(p0n), float(p1n)
    spec = oracle.make_spec("normal", p0n, p1n, relu=relu, seed=5, offset=2, Dn=D, n_edges=E, p1_log=True)
    mk = lambda a, l, **kw: stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, (a + shift) if pmode != "scalar" else float(a + shift),
                                                l if pmode != "scalar" else float(l), relu=relu, seed=5, offset=2,
                                                p1_log=True, **kw)
    assert_close(ops.aggregate(g, x0, mk(a0, l0)), oracle.agg_fwd(og, x0.cpu().numpy(), spec), what=f"p1_log forward {pmode}")
    assert_close(mk(a0, l0).materialize(), oracle.noise_materialize(og, spec, D), what=f"p1_log materialised {pmode}")
    if pmode == "scalar":
        return
    x, a, l = (t.clone().requires_grad_(True) for t in (x0, a0, l0))
    out = ops.aggregate(g, x, stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, a + shift, l, relu=relu, seed=5, offset=2,
                                                 p1_log=True, differentiable=True), reduce="mean", seg_len=32)
    out.backward(gout)
    z = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 0.0, 1.0, seed=5, offset=2).materialize()
    x2, a2, l2 = (t.clone().requires_grad_(True) for t in (x0, a0, l0))
    w = (a2 + shift) + l2.exp() * z
    if relu:
        w = w.relu()
    out2 = ops.aggregate(g, x2, w.expand(E, D), reduce="mean", seg_len=32)
    out2.backward(gout)
    assert_close(out, out2.detach().cpu().numpy(), what="p1_log vi forward")
    assert_close(x.grad, x2.grad.cpu().numpy(), what="p1_log dx")
    assert_close(a.grad, a2.grad.cpu().numpy(), what=f"p1_log d loc {pmode}")
    assert_close(l.grad, l2.grad.cpu().numpy(), what=f"p1_log d log_scale {pmode}")


@pytest.mark.parametrize("of", [1, 16])
def test_amortized_layer_uses_log_scale_descriptor(dev, of):
    """StagLayer(GCN, q_a=AmortizedDistribution) hands the kernel loc / log_scale as the heads produce them: the
    descriptor carries p1_log, no [E, Dn] exp tensor is formed, and the MLP's gradients equal those of the
    reference's dataflow (exp, rsample, edge_weight=)."""
    import stag_amd
    from stag_amd import _lib
    from stag_amd.distributions import AmortizedDistribution
    from util import random_graph
    g = random_graph(120, 900, seed=6, hub=90, device=dev)
    x = torch.randn(120, 16, device=dev)
    torch.manual_seed(4)
    q = AmortizedDistribution(16, of, init_like=torch.distributions.Normal(1.0, 0.3))
    gcn = stag_amd.zoo.GCN(16, 8)
    layer = stag_amd.layers.StagLayer(gcn, q_a=q, vi=True).to(dev)
    stag_amd.manual_seed(9)
    out = layer(g, x)
    h = layer._edge_weight_handle
    assert isinstance(h, stag_amd.EdgeNoise) and h.p1_log and h.param_mode in (_lib.PARAM_PER_EDGE1, _lib.PARAM_PER_EDGE)
    gout = torch.randn_like(out)
    out.backward(gout)
    got = {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}
    layer.zero_grad()
    q.condition(g, x)
    z = stag_amd.EdgeNoise(g, 16, _lib.NOISE_NORMAL, 0.0, 1.0, seed=9, offset=h.offset).materialize()
    w = q.new_parameters["loc"] + q.new_parameters["log_scale"].exp() * z
    ref = gcn(g, x, edge_weight=w)
    assert_close(out, ref.detach().cpu().numpy(), what="amortised layer forward")
    ref.backward(gout)
    assert any("parameters_mlp.log_scale" in k for k in got)
    for k, p in layer.named_parameters():
        if p.grad is None:
            continue
        sc = max(1.0, float(p.grad.abs().max()))
        assert_close(got[k] / sc, (p.grad / sc).cpu().numpy(), what=f"amortised d {k}")


def test_sample_based_kl_reaches_q_a_on_the_fused_path(dev):
    """No closed-form KL (a MixtureSameFamily prior, which StagLayer accepts: stag/layers.py:66-67) => the
    regulariser is q.log_prob(w) - p.log_prob(w) on the LAST SAMPLE (stag/layers.py:141-143), and the
    reference differentiates through that sample (`rsample`).  On the fused vi=True path the sample is
    re-formed from the live parameters and the same counters, so loc / log_scale get the same gradient as
    on the materialised path."""
    import stag_amd
    from stag_amd import _lib
    from util import random_graph
    g = random_graph(120, 900, seed=12, hub=100, device=dev)
    E, D = g.number_of_edges(), 8
    x = torch.randn(120, D, device=dev)
    mix = torch.distributions.MixtureSameFamily(
        torch.distributions.Categorical(torch.tensor([0.3, 0.7], device=dev)),
        torch.distributions.Normal(torch.tensor([0.0, 1.0], device=dev), torch.tensor([0.5, 0.8], device=dev)))
    for relu in (False, True):
        layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, 4), q_a=torch.distributions.Normal(1.0, 0.5),
                                          p_a=mix, vi=True, relu=relu).to(dev)
        stag_amd.manual_seed(21)
        out = layer(g, x)
        assert isinstance(layer._edge_weight_handle, stag_amd.EdgeNoise), "vi=True GCN stays on the fused path"
        off = layer._edge_weight_handle.offset
        kl = layer.kl_divergence()
        assert kl.requires_grad
        (out.sum() * 0.0 + kl).backward()
        got = (layer.q_a.loc.grad.clone(), layer.q_a.log_scale.grad.clone())
        assert float(got[0].abs()) > 0 and float(got[1].abs()) > 0
        # the materialised statement: z from the same counters, the affine map and both log-probs in torch
        z = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 0.0, 1.0, seed=21, offset=off).materialize()
        loc = layer.q_a.loc.detach().clone().requires_grad_(True)
        ls = layer.q_a.log_scale.detach().clone().requires_grad_(True)
        w = loc + ls.exp() * z
        if relu:
            w = w.relu()
        ref = (torch.distributions.Normal(loc, ls.exp()).log_prob(w).sum(-1).mean() - mix.log_prob(w).sum(-1).mean())
        ref.backward()
        assert_close(kl, ref.detach().cpu().numpy(), what="sample-based KL")
        assert_close(got[0], loc.grad.cpu().numpy(), what="d KL / d loc")
        assert_close(got[1], ls.grad.cpu().numpy(), what="d KL / d log_scale")


@pytest.mark.parametrize("norm", [False, True])
def test_gat_vi_descriptor_gradients(dev, norm):
    """StagLayer(GAT, vi=True) hands the GAT layer a differentiable descriptor; the gradients into loc / log_scale
    equal those of the reference's dataflow (rsample -> [E, H] tensor -> relu -> _in_norm -> edge_weight=)."""
    import stag_amd
    from stag_amd import _lib
    from stag_amd.layers import _in_norm
    from util import random_graph
    g = random_graph(200, 1500, seed=8, hub=150, device=dev)
    x = torch.randn(200, 16, device=dev)
    torch.manual_seed(1)
    gat = stag_amd.zoo.GAT(16, 8, num_heads=4).to(dev)
    layer = stag_amd.layers.StagLayer(gat, q_a=torch.distributions.Normal(1.0, 0.5), vi=True, relu=True, norm=norm).to(dev)
    stag_amd.manual_seed(3)
    out = layer(g, x)
    h = layer._edge_weight_handle
    assert isinstance(h, stag_amd.EdgeNoise) and h.grad_params is not None and h.in_norm == norm
    gout = torch.randn_like(out)
    out.backward(gout)
    got = (layer.q_a.loc.grad.clone(), layer.q_a.log_scale.grad.clone(), gat.fc.weight.grad.clone())
    layer.zero_grad()
    z = stag_amd.EdgeNoise(g, 4, _lib.NOISE_NORMAL, 0.0, 1.0, seed=3, offset=h.offset).materialize()
    w = (layer.q_a.loc + layer.q_a.log_scale.exp() * z).relu()
    if norm:
        w = _in_norm(g, w)
    ref = gat(g, x, edge_weight=w)
    assert_close(out, ref.detach().cpu().numpy(), what="vi GAT forward")
    ref.backward(gout)
    for a_, b_, nm in zip(got, (layer.q_a.loc.grad, layer.q_a.log_scale.grad, gat.fc.weight.grad), ("loc", "log_scale", "fc.weight")):
        sc = max(1.0, float(b_.abs().max()))
        assert_close(a_ / sc, (b_ / sc).cpu().numpy(), what=f"vi GAT d {nm}")


def test_gat_attention_dropout(dev):
    """zoo.GAT(attn_drop=0.6) — what the reference's GAT scripts construct (scripts/citation_mle/gat/run.py:40)
    — builds, trains through the composed path (dropout between softmax and sum, stag/zoo/gat.py:122) and is
    the fused kernel again in eval mode."""
    import stag_amd
    from stag_amd import ops
    from util import random_graph
    g = random_graph(150, 1200, seed=3, hub=200, device=dev)
    x = torch.randn(150, 16, device=dev)
    torch.manual_seed(0)
    gat = stag_amd.zoo.GAT(16, 8, num_heads=4, feat_drop=0.0, attn_drop=0.6).to(dev)
    ref = stag_amd.zoo.GAT(16, 8, num_heads=4).to(dev)
    ref.load_state_dict(gat.state_dict())
    gat.eval()
    w = torch.rand(g.number_of_edges(), 4, device=dev) + 0.5
    out_eval, a_eval = gat(g, x, get_attention=True, edge_weight=w)
    assert torch.equal(out_eval, ref(g, x, edge_weight=w)), "eval mode: the fused kernel, dropout off"
    gat.train()
    torch.manual_seed(5)
    out_tr, a_tr = gat(g, x, get_attention=True, edge_weight=w)
    torch.manual_seed(5)
    a_drop = torch.nn.functional.dropout(a_eval.squeeze(-1), 0.6, training=True)
    assert_close(a_tr.squeeze(-1), a_drop.cpu().numpy(), what="dropped attention")
    ft = (x @ gat.fc.weight.t()).view(-1, 4, 8)
    want = ops.aggregate(g, ft.reshape(150, 32), a_drop.repeat_interleave(8, dim=1)) + gat.bias
    assert_close(out_tr, want.detach().cpu().numpy(), what="GAT output under attention dropout")
    kept = float((a_tr != 0).float().mean())
    assert 0.3 < kept < 0.5
    xg = x.clone().requires_grad_(True)
    gat(g, xg, edge_weight=w).square().mean().backward()
    assert torch.isfinite(xg.grad).all() and all(p.grad is not None for p in gat.parameters())
    # and under a StagLayer with drawn head weights
    layer = stag_amd.layers.StagLayer(gat, q_a=torch.distributions.Normal(1.0, 0.5)).to(dev)
    assert layer(g, x).shape == (150, 32)


def test_vi_layer_trains_fused(dev):
    """StagLayer(vi=True) on GCN keeps the EdgeNoise descriptor (no [E, D] tensor) and its
    q_a parameters receive gradients; KL uses the closed form."""
    import stag_amd
    from util import random_graph
    g = random_graph(200, 2000, seed=3, device=dev)
    x = torch.randn(200, 16, device=dev)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(16, 8), q_a=torch.distributions.Normal(1.0, 0.4), vi=True).to(dev)
    out = layer(g, x)
    assert isinstance(layer._edge_weight_handle, stag_amd.EdgeNoise)
    (out.square().mean() + layer.kl_divergence()).backward()
    assert layer.q_a.loc.grad is not None and layer.q_a.log_scale.grad is not None
    assert float(layer.q_a.log_scale.grad.abs()) > 0
    rc = stag_amd.layers.StagLayer(stag_amd.zoo.GraphSAGE(16, 8), relu=True, vi=True,
                                   q_a=torch.distributions.Normal(torch.ones(16), 0.5 * torch.ones(16))).to(dev)
    rc(g, x).sum().backward()
    assert rc.q_a.loc.grad.shape == (16,) and rc.q_a.log_scale.grad.shape == (16,)


def _gat_torch_reference(src, dst, n, el, er, ft, w, neg_slope):
    """Plain torch (autograd) statement of stag/zoo/gat.py:114-126 for the gradient check."""
    e = torch.nn.functional.leaky_relu(el[src] + er[dst], neg_slope)
    if w is not None:
        e = w * e
    H = e.shape[1]
    idx = dst.unsqueeze(1).expand_as(e)
    mx = torch.full((n, H), -float("inf"), device=e.device, dtype=e.dtype).scatter_reduce(0, idx, e, "amax")
    ex = torch.exp(e - mx[dst])
    den = torch.zeros((n, H), device=e.device, dtype=e.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    return torch.zeros_like(ft).index_add_(0, dst, a.unsqueeze(-1) * ft[src])


@pytest.mark.parametrize("H,F", [(8, 32), (3, 4), (2, 16), (8, 16)])      # (8, 16): 32 lanes per row, forward and backward
@pytest.mark.parametrize("mode", ["none", "explicit", "noise", "noise_norm"])
def test_gat_backward(dev, oracle, H, F, mode):
    """stag_gat_bwd against its CPU twin (oracle.gat_bwd = stag_gat_bwd_cpu, float64; pinned by the reference's own
    autograd gradients in tests/test_oracle_golden.py::test_gat_gradients_golden); the torch statement on the device
    stays as a second opinion."""
    import stag_amd
    from stag_amd import _lib, ops
    from util import random_graph
    rng = np.random.default_rng(H * 7 + F)
    n = 120
    g = random_graph(n, 900, seed=H + F, hub=200, device=dev)
    src, dst = g.edges()
    E = g.number_of_edges()
    mk = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32), device=dev)
    el0, er0, ft0, G = mk(n, H), mk(n, H), mk(n, H, F), mk(n, H, F)
    w0 = torch.tensor(rng.uniform(0.5, 1.5, (E, H)).astype(np.float32), device=dev)
    if mode == "noise":
        weight = stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.3, seed=3, offset=1)
        w_ref = weight.materialize()
    elif mode == "noise_norm":
        weight = stag_amd.EdgeNoise(g, H, _lib.NOISE_BERNOULLI, 0.7, None, seed=3, offset=1, in_norm=True)
        w_ref = weight.materialize()
    elif mode == "explicit":
        weight = w0.clone().requires_grad_(True)
        w_ref = w0.clone().requires_grad_(True)
    else:
        weight = w_ref = None
    el, er, ft = (t.clone().requires_grad_(True) for t in (el0, er0, ft0))
    out = ops.gat_aggregate(g, el, er, ft, 0.2, weight, seg_len=32)
    out.backward(G)
    el2, er2, ft2 = (t.clone().requires_grad_(True) for t in (el0, er0, ft0))
    ref = _gat_torch_reference(src, dst, n, el2, er2, ft2, w_ref, 0.2)
    ref.backward(G)
    from util import assert_gat_grads_vs_oracle
    og = oracle_graph(oracle, g)
    if mode == "noise":
        spec = oracle.make_spec("normal", 1.0, 0.3, seed=3, offset=1, Dn=H, n_edges=E)
    elif mode == "noise_norm":
        spec = oracle.make_spec("bernoulli", 0.7, None, in_norm=True, seed=3, offset=1, Dn=H, n_edges=E)
    elif mode == "explicit":
        spec = oracle.make_spec("explicit", w0.cpu().numpy())
    else:
        spec = oracle.make_spec("none")
    assert_gat_grads_vs_oracle(oracle, og, el0.cpu().numpy(), er0.cpu().numpy(), ft0.cpu().numpy(), G.cpu().numpy(), spec,
                               [el.grad, er.grad, ft.grad], got_dw=weight.grad if mode == "explicit" else None,
                               what=f"gat bwd {mode} H={H} F={F}", dev=dev)
    # the two-gather form of the same backward
    ops._GAT_BWD_ONE_GATHER = False
    try:
        t3 = [t.clone().requires_grad_(True) for t in (el0, er0, ft0)]
        w3 = w0.clone().requires_grad_(True) if mode == "explicit" else weight
        ops.gat_aggregate(g, *t3, 0.2, w3, seg_len=32).backward(G)
    finally:
        ops._GAT_BWD_ONE_GATHER = True
    assert_gat_grads_vs_oracle(oracle, og, el0.cpu().numpy(), er0.cpu().numpy(), ft0.cpu().numpy(), G.cpu().numpy(), spec,
                               [a_.grad for a_ in t3], got_dw=w3.grad if mode == "explicit" else None,
                               what=f"gat bwd two-pass {mode} H={H} F={F}", dev=dev)
    assert_close(out, ref.detach().cpu().numpy(), what="gat forward")
    assert_close(ft.grad, ft2.grad.cpu().numpy(), what="d ft")
    assert_close(el.grad, el2.grad.cpu().numpy(), what="d el")
    assert_close(er.grad, er2.grad.cpu().numpy(), what="d er")
    if mode == "explicit":
        assert_close(weight.grad, w_ref.grad.cpu().numpy(), what="d w")


def test_gat_layer_trains(dev):
    import stag_amd
    from util import random_graph
    torch.manual_seed(0)
    g = random_graph(300, 3000, seed=2, hub=400, device=dev)
    x = torch.randn(300, 16, device=dev)
    y = torch.randint(0, 4, (300,), device=dev)
    layers = torch.nn.ModuleList([
        stag_amd.layers.StagLayer(stag_amd.zoo.GAT(16, 8, num_heads=4, activation=torch.nn.functional.elu),
                                  q_a=torch.distributions.Normal(1.0, 0.2)),
        stag_amd.layers.StagLayer(stag_amd.zoo.GAT(32, 4, num_heads=2, last=True,
                                                   activation=lambda t: torch.softmax(t, -1)),
                                  q_a=torch.distributions.Normal(1.0, 0.2))])
    model = stag_amd.models.StagModel(layers=layers).to(dev)
    opt = torch.optim.Adam(model.parameters(), 1e-2)
    losses = []
    for _ in range(25):
        opt.zero_grad()
        loss = model.loss(g, x, y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] - 0.03


def test_full_size_against_oracle_and_repeatability(dev, oracle):
    """cfg2 at full size against the CPU oracle, then 200 back-to-back launches bit-compared with
    the first: the in-launch hand-off of long-row partials (write-through stores, ticket, acquire)
    must never read a stale partial, whatever the placement and load."""
    import stag_amd
    from stag_amd import _lib, ops, synthetic
    from util import oracle_graph
    src, dst = synthetic.arxiv_like(seed=1)
    n, D = synthetic.ARXIV_NODES, 128
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(0))
    xd = x.to(dev)
    mk = lambda off: stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=0x5747A6, offset=off)
    first = ops.aggregate(g, xd, mk(0))
    og = oracle_graph(oracle, g)
    from util import hw_normals
    spec2 = oracle.make_spec("normal", 1.0, 0.5, seed=0x5747A6, offset=0, Dn=D, n_edges=g.number_of_edges())
    deg = g.in_degrees().cpu().numpy()
    # the bar, flat over every row (the 13k-edge hub included): the oracle draws the device's own normals
    # (tables of the hardware functions, pinned exhaustively by test_normal_tables_exhaustive), so what is
    # compared is the arithmetic of 21.7 M sums — fp32 + Kahan here, fp64 there
    with hw_normals(oracle, dev):
        ref = oracle.agg_fwd(og, x.numpy(), spec2)
    assert_close(first, ref, what="cfg2 full size vs oracle, every row at 1e-5")
    # against the oracle's own (libm, fp64) normals the same bar holds on every row of up to 256 in-edges;
    # beyond, the hardware's ~4.5e-8 rms per-draw deviation accumulates over thousands of draws of one sum
    ref_libm = oracle.agg_fwd(og, x.numpy(), spec2)
    short = deg <= 256
    assert_close(first[torch.from_numpy(short).to(dev)], ref_libm[short], what="cfg2 vs libm normals, rows <= 256 edges")
    assert_close(first, ref_libm, tol=1.1e-5, what="cfg2 vs libm normals, every row (measured worst: 1.06e-5, on a 3k-edge row)")
    other = ops.aggregate(g, xd, mk(1))            # interleave a different noise field: L1/L2 stay warm
    bad = 0
    for i in range(200):
        out = ops.aggregate(g, xd, mk(i % 2))
        bad += int(not torch.equal(out, first if i % 2 == 0 else other))
    assert bad == 0, f"{bad} of 200 launches differed"
    # GAT at cfg5 shape: same protocol with per-segment softmax states
    H, F = 8, 32
    el, er = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev)
    ft = torch.randn(n, H, F, device=dev)
    mkh = lambda: stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=5, offset=0)
    g0 = ops.gat_aggregate(g, el, er, ft, 0.2, mkh())
    with hw_normals(oracle, dev):
        ref = oracle.gat_fwd(og, el.cpu().numpy(), er.cpu().numpy(), ft.cpu().numpy(), 0.2,
                             oracle.make_spec("normal", 1.0, 0.5, seed=5, offset=0, Dn=H, n_edges=g.number_of_edges()))
    assert_close(g0.reshape(n, -1), ref.reshape(n, -1), what="cfg5 full size vs oracle, every row at 1e-5")
    assert all(torch.equal(ops.gat_aggregate(g, el, er, ft, 0.2, mkh()), g0) for _ in range(30))


def test_device_epoch_and_graph_capture(dev):
    """spec.epoch: the kernels draw at offset + *epoch (a device counter), so a captured hipGraph
    gets fresh noise per replay.  (1) epoch e at offset o == offset o + e, bit for bit, on every
    entry point that draws; (2) a captured StagLayer step replays with new noise each time and each
    replay equals the eager result at the same effective offset; (3) no host sync in the step."""
    import stag_amd
    from stag_amd import _lib, ops
    from stag_amd.random import NoiseGenerator
    from util import random_graph
    n, D, H, F = 300, 32, 4, 8
    g = random_graph(n, 3000, seed=1, hub=200, device=dev)
    x = torch.randn(n, D, device=dev)
    epoch = torch.full((1,), 5, dtype=torch.int64, device=dev)
    mk = lambda off, ep, dn=D: stag_amd.EdgeNoise(g, dn, _lib.NOISE_NORMAL, 1.0, 0.5, seed=9, offset=off, epoch=ep)
    assert torch.equal(ops.aggregate(g, x, mk(3, epoch)), ops.aggregate(g, x, mk(8, None)))
    assert torch.equal(mk(3, epoch).materialize(), mk(8, None).materialize())
    el, er, ft = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev), torch.randn(n, H, F, device=dev)
    assert torch.equal(ops.gat_aggregate(g, el, er, ft, 0.2, mk(3, epoch, H)),
                       ops.gat_aggregate(g, el, er, ft, 0.2, mk(8, None, H)))
    xg = x.clone().requires_grad_(True)
    ops.aggregate(g, xg, mk(3, epoch)).square().sum().backward()
    xh = x.clone().requires_grad_(True)
    ops.aggregate(g, xh, mk(8, None)).square().sum().backward()
    assert torch.equal(xg.grad, xh.grad)

    # ---- capture one layer step; the generator's device epoch moves the noise between replays
    gen = NoiseGenerator(seed=77)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, 16), q_a=torch.distributions.Normal(1.0, 0.5),
                                      relu=True, generator=gen).to(dev)
    ref_layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, 16), q_a=torch.distributions.Normal(1.0, 0.5),
                                          relu=True, generator=NoiseGenerator(seed=77)).to(dev)
    ref_layer.load_state_dict(layer.state_dict())
    gen.enable_device_epoch(dev)
    with torch.no_grad():
        layer(g, x)                        # warm-up outside the capture: plans, counters, caches
        gen.manual_seed(77)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            mark = gen.offset
            y = layer(g, x)
            gen.advance_epoch(gen.offset - mark)
        outs = []
        for _ in range(3):
            graph.replay()
            outs.append(y.clone())
        torch.cuda.synchronize()
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
        for i in range(3):                 # eager twin: one draw per call, offsets 0, 1, 2
            assert torch.equal(ref_layer(g, x), outs[i])
        assert int(gen.device_epoch) == 3


def test_model_monte_carlo_first_layer_batched(dev):
    """StagModel(..., n_samples=S) at inference draws the first layer's S samples from one pass over
    the gathered rows; every sample sees the noise the sequential loop would give it, so the mean
    is unchanged bit for bit, and the generator ends where the loop would leave it."""
    import stag_amd
    from stag_amd.random import NoiseGenerator
    from util import random_graph
    n, D = 400, 24
    g = random_graph(n, 4000, seed=3, hub=300, device=dev)
    x = torch.randn(n, D, device=dev)
    N = torch.distributions.Normal
    for first_kw in (dict(q_a=N(1.0, 0.5)), dict(q_a=torch.distributions.Bernoulli(0.7)), dict(q_a=N(1.0, 0.5), relu=True, vi=True),
                     dict(q_a=torch.distributions.Bernoulli(0.7), norm=True)):     # scripts/arxiv_mle/gcn/run.py:70-74
        gen = NoiseGenerator(seed=5)
        layers = [stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, 16, activation=torch.relu), generator=gen, **first_kw),
                  stag_amd.layers.StagLayer(stag_amd.zoo.GraphSAGE(16, 16, activation=torch.relu), generator=gen,
                                            q_a=N(1.0, 0.3)),
                  stag_amd.layers.StagLayer(stag_amd.zoo.GCN(16, 5), generator=gen, q_a=N(1.0, 0.3))]
        for l in layers:
            l.to(dev)
        model = stag_amd.models.StagModel(layers)
        calls = []
        orig = layers[0].forward_mc
        layers[0].forward_mc = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        with torch.no_grad():
            gen.manual_seed(5)
            got = model(g, x, n_samples=5, return_parameters=True)
            end = gen.offset
            gen.manual_seed(5)
            ref = torch.stack([model._forward(g, x) for _ in range(5)], 0).mean(0)
            assert gen.offset == end == 15
        assert calls and all(calls), "the batched first layer was not used"
        assert torch.equal(got, ref)
    # an input that carries a gradient: the loop is the reference's
    gen.manual_seed(5)
    model(g, x.requires_grad_(True), n_samples=2, return_parameters=True).sum().backward()
    assert x.grad is not None


@pytest.mark.parametrize("first", ["gcn_normal", "gcn_bernoulli_norm", "sage_normal", "gin_uniform", "gcn_vi", "gcn_vi_rc",
                                   "gcn_vi_mixture", "gcn_normal_dx"])
def test_training_monte_carlo_loop_batched_on_the_first_layer(dev, first):
    """`model.loss(..., n_samples=4)` — the training loop of stag/models.py:67-68 as the sweeps run it
    (`--n_samples_training 4`, scripts/arxiv_mle/graph_sage/meta_run.sh:29) — draws the first layer's 4 samples from
    one pass over the gathered rows when its input is data and its noise fixed: loss, KL term and EVERY parameter
    gradient equal the sequential loop's, the generator ends where the loop leaves it.  The model has a vi=True
    layer further up (its KL is read per sample) and a GAT layer with in-kernel attention dropout (two offsets per
    forward)."""
    import stag_amd
    from stag_amd.random import NoiseGenerator
    from util import random_graph
    n, D = 400, 24
    g = random_graph(n, 4000, seed=3, hub=300, device=dev)
    x = torch.randn(n, D, device=dev)
    y = torch.randint(0, 5, (n,), device=dev)
    mask = torch.rand(n, device=dev) < 0.6
    N, B, U = torch.distributions.Normal, torch.distributions.Bernoulli, torch.distributions.Uniform
    L, Z = stag_amd.layers, stag_amd.zoo
    gen = NoiseGenerator(seed=5)
    torch.manual_seed(1)
    l0 = {"gcn_normal": lambda: L.StagLayer(Z.GCN(D, 16, activation=torch.relu), generator=gen, q_a=N(1.0, 0.5), relu=True),
          "gcn_bernoulli_norm": lambda: L.StagLayer(Z.GCN(D, 16, activation=torch.relu), generator=gen, q_a=B(0.7), norm=True),
          "sage_normal": lambda: L.StagLayer(Z.GraphSAGE(D, 16, activation=torch.relu), generator=gen, q_a=N(1.0, 0.5)),
          "gin_uniform": lambda: L.StagLayer(Z.GIN(D, 16, activation=torch.relu), generator=gen, q_a=U(0.5, 1.5)),
          # a LEARNED first layer (scripts/citation_r1, citation_rc with --n_samples_training): the forward is batched,
          # the backward is the loop's per-sample passes; its KL term is read per sample
          "gcn_vi": lambda: L.StagLayer(Z.GCN(D, 16, activation=torch.relu), generator=gen, q_a=N(1.0, 0.5), relu=True, vi=True),
          "gcn_vi_rc": lambda: L.StagLayer(Z.GCN(D, 16, activation=torch.relu), generator=gen,
                                           q_a=N(torch.ones(D), 0.5 * torch.ones(D)), vi=True),
          # a prior without a closed-form KL: the sample-based estimate reads the layer's CURRENT sample (mc_select)
          "gcn_vi_mixture": lambda: L.StagLayer(
              Z.GCN(D, 16, activation=torch.relu), generator=gen, q_a=N(1.0, 0.5), vi=True,
              p_a=torch.distributions.MixtureSameFamily(torch.distributions.Categorical(torch.tensor([0.5, 0.5], device=dev)),
                                                        N(torch.tensor([0.0, 1.0], device=dev), torch.tensor([0.5, 0.5], device=dev)))),
          "gcn_normal_dx": lambda: L.StagLayer(Z.GCN(D, 16, activation=torch.relu), generator=gen, q_a=N(1.0, 0.5))}[first]()
    if first == "gcn_normal_dx":          # an input that carries a gradient
        x = x.requires_grad_(True)
    layers = torch.nn.ModuleList([
        l0,
        L.StagLayer(Z.GAT(16, 4, num_heads=4, attn_drop=0.5, activation=torch.nn.functional.elu), generator=gen, q_a=N(1.0, 0.3)),
        L.StagLayer(Z.GCN(16, 5, activation=lambda t: torch.softmax(t, -1)), generator=gen, q_a=N(1.0, 0.3), vi=True)])
    model = stag_amd.models.StagModel(layers, kl_scaling=0.3).to(dev)
    model.train()
    assert [l.offsets_per_forward() for l in layers] == [1, 2, 1]
    calls = []
    orig = l0.forward_mc
    def counted(*a, **k):
        out = orig(*a, **k)
        calls.append(out is not None)
        return out
    l0.forward_mc = counted

    def run(batched):
        model.zero_grad(set_to_none=True)
        model._mc_batching_off = not batched
        gen.manual_seed(5)
        if x.requires_grad:
            x.grad = None
        nll, reg = model.loss_terms(g, x, y, mask=mask, n_samples=4)
        (nll + reg).backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        if x.requires_grad:
            grads["x"] = x.grad.clone()
        return nll.detach(), reg.detach(), gen.offset, grads

    nll_b, reg_b, end_b, gr_b = run(True)
    assert calls and all(calls), "the batched first layer was not used"
    nll_s, reg_s, end_s, gr_s = run(False)
    assert end_b == end_s == 16
    assert_close(torch.stack([nll_b, reg_b]), torch.stack([nll_s, reg_s]).cpu().numpy(), what=f"{first}: nll, kl")
    assert gr_b.keys() == gr_s.keys() and len(gr_b) >= 8
    for k in gr_s:
        sc = max(1.0, float(gr_s[k].abs().max()))
        assert_close(gr_b[k] / sc, (gr_s[k] / sc).cpu().numpy(), what=f"{first}: d {k}")
    # a layer that consumes offsets it does not report: the first sample notices, the loop falls back for good
    layers[1].offsets_per_forward = lambda: 1
    model._mc_batching_off = False
    gen.manual_seed(5)
    nll_f, reg_f = model.loss_terms(g, x.detach(), y, mask=mask, n_samples=4)
    assert model._mc_batching_off and gen.offset == 16
    assert_close(torch.stack([nll_f, reg_f]), torch.stack([nll_s, reg_s]).cpu().numpy(), what="fallback loop")


def test_bench_contract_and_smoke(dev):
    """The driver's entry points, run the way the driver runs them: `python bench.py` prints ONE JSON
    line with the contract's keys (plus `roofline` and, with --full, `cpu_baseline`), and smoke() passes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "30", "--warmup", "5",
                        "--cpu-budget-s", "3", "--full"], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["steps"] == 30 and line["warmup"] == 5 and line["unit"] == "edges/s"
    assert line["dtype"] == "f32" and line["data"] == "synthetic" and line["vs_baseline"] is None
    assert "workload" in line["config"] and "model" not in line["config"]
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0.05 < rf["frac"] < 1.0
    # value = edges per step / wall time per step; device time agrees with wall time within 10 %
    assert abs(line["value"] - 1166243 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-6
    assert abs(rf["device_ms_per_step"] - line["ms_per_step"]) / line["ms_per_step"] < 0.10
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "edges/s" and cb["cores"] >= 1 and cb["value"] > 0
    import __graft_entry__
    __graft_entry__.smoke()


def test_no_memory_growth_across_training_steps(dev):
    """Every layer mode, forward + backward repeated: device memory in use must not grow from step
    to step.  (Autograd contexts once kept a `local_var()` graph whose frames held the step's
    [E, D] tensors — a cycle through the autograd graph, 650 MB per step at cfg2 size.)"""
    import gc
    import stag_amd
    from util import random_graph
    n, D = 3000, 32
    g = random_graph(n, 40000, seed=1, hub=500, device=dev)
    x = torch.randn(n, D, device=dev, requires_grad=True)
    gout = torch.randn(n, D, device=dev)
    N = torch.distributions.Normal
    modes = [dict(q_a=N(1.0, 0.5)), dict(q_a=N(1.0, 0.5), vi=True, relu=True), dict(q_a=N(1.0, 0.5), vi=True, norm=True),
             dict(q_a=torch.distributions.Bernoulli(0.5), norm=True),
             dict(q_a=stag_amd.distributions.AmortizedDistribution(D, 1, init_like=N(1.0, 0.3)), vi=True),
             dict(q_a=stag_amd.distributions.AmortizedDistribution(D, D, init_like=N(1.0, 0.3)), vi=True)]
    for kw in modes:
        layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, D), **kw).to(dev)
        mem = []
        for i in range(5):
            for p in layer.parameters():
                p.grad = None
            layer(g, x).backward(gout)
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated())
        assert mem[4] <= mem[2], (kw, mem)
        del layer
        gc.collect()


@pytest.mark.parametrize("H,F", [(4, 128), (8, 64), (16, 64), (3, 256), (8, 96), (2, 6), (3, 12), (20, 16)])
def test_gat_outside_the_fused_kernel_limits(dev, oracle, H, F):
    """Beyond 256 channels per row.  Up to H*F = 1024 (H <= 16, F % 4 == 0) the workgroup-cooperative kernels
    give every lane 2 or 4 chunks of 4 channels ((4,128), (8,64), (16,64), (3,256)); F/4 not a power of two
    under autograd ((8,96), (2,6), (3,12)) or H > 16 with more than 256 channels ((20,16)) is composed from
    the aggregation kernel and [E, H] torch ops.  Forward against the oracle, gradients against a float64
    torch restatement — the same bar either way."""
    import stag_amd
    from stag_amd import _lib, ops
    from util import random_graph
    n = 60
    g = random_graph(n, 500, seed=5, hub=80, device=dev)
    src, dst = (t.long() for t in g.edges())
    torch.manual_seed(H * 100 + F)
    el, er, ft = (torch.randn(n, H, device=dev, requires_grad=True), torch.randn(n, H, device=dev, requires_grad=True),
                  torch.randn(n, H, F, device=dev, requires_grad=True))
    noise = stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=3, offset=2)
    out, attn = ops.gat_aggregate(g, el, er, ft, 0.2, noise, want_attn=True)
    og = oracle_graph(oracle, g)
    sp = oracle.make_spec("normal", 1.0, 0.5, seed=3, offset=2, Dn=H, n_edges=g.number_of_edges())
    ref, ref_attn = oracle.gat_fwd(og, el.detach().cpu().numpy(), er.detach().cpu().numpy(), ft.detach().cpu().numpy(),
                                   0.2, sp, want_attn=True)
    assert_close(out, ref, what="composed GAT out")
    assert_close(attn, ref_attn, what="composed GAT attention")
    G = torch.randn_like(out)
    out.backward(G)
    # float64 restatement with the same (materialised) weights
    w = noise.materialize().double()
    el2, er2, ft2 = (t.detach().double().requires_grad_(True) for t in (el, er, ft))
    e = torch.nn.functional.leaky_relu(el2[src] + er2[dst], 0.2) * w
    m = torch.full((n, H), -1e300, dtype=torch.float64, device=dev).scatter_reduce(0, dst.unsqueeze(1).expand(-1, H), e.detach(), "amax")
    p = torch.exp(e - m[dst])
    l = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add(0, dst, p)
    a = p / l[dst]
    o2 = torch.zeros(n, H, F, dtype=torch.float64, device=dev).index_add(0, dst, a.unsqueeze(-1) * ft2[src])
    o2.backward(G.double())
    for got, want, name in ((el.grad, el2.grad, "d el"), (er.grad, er2.grad, "d er"), (ft.grad, ft2.grad, "d ft")):
        assert_close(got, want.float().cpu().numpy(), what=name)


def test_sage_pool_and_max_reducer(dev):
    """GraphSAGE 'pool' (max reducer; stag/zoo/graph_sage.py:90-93) is composed from the row gather
    and a scatter-amax: values and gradients against a float64 dense restatement; rows without
    in-edges read 0 as in DGL."""
    import stag_amd
    from util import random_graph
    n, D = 80, 12
    g = random_graph(n, 400, seed=9, hub=60, device=dev)
    src, dst = (t.long() for t in g.edges())
    x = torch.randn(n, D, device=dev, requires_grad=True)
    w = (torch.rand(g.number_of_edges(), D, device=dev) + 0.5).requires_grad_(True)
    layer = stag_amd.zoo.GraphSAGE(D, 7, aggregator_type="pool").to(dev)
    out = layer(g, x, edge_weight=w)
    out.sum().backward()
    x2, w2 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    lin = lambda m, t: t @ m.weight.double().t() + (m.bias.double() if m.bias is not None else 0)
    h = torch.relu(lin(layer.fc_pool, x2))
    msg = h[src] * w2
    neigh = torch.zeros(n, D, dtype=torch.float64, device=dev).scatter_reduce(
        0, dst.unsqueeze(1).expand(-1, D), msg, "amax", include_self=False)
    ref = lin(layer.fc_self, x2) + lin(layer.fc_neigh, neigh) + layer.bias.double()
    ref.sum().backward()
    assert_close(out, ref.detach().float().cpu().numpy(), what="pool")
    assert_close(x.grad, x2.grad.float().cpu().numpy(), what="pool dx")
    assert_close(w.grad, w2.grad.float().cpu().numpy(), what="pool dw")
    # through the graph surface, with fused-noise weights materialised on the way
    import stag_amd.function as fn
    from stag_amd import _lib
    gl = g.local_var()
    gl.srcdata["h"] = x.detach()
    gl.edata["w"] = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.3, seed=1, offset=1)
    gl.update_all(fn.u_mul_e("h", "w", "m"), fn.max("m", "o"))
    wm = gl.edata["w"].materialize()
    want = torch.zeros(n, D, device=dev).scatter_reduce(0, dst.unsqueeze(1).expand(-1, D), x.detach()[src] * wm, "amax",
                                                         include_self=False)
    assert torch.equal(gl.dstdata["o"], want)
    assert (gl.dstdata["o"][g.in_degrees() == 0] == 0).all()


# ---- amortised per-edge parameters with narrow heads (csrc/amort.hip) ----------------------------------------

@pytest.mark.parametrize("n,K,C", [(0, 8, 2), (1, 1, 1), (1000, 9, 2), (5000, 128, 2), (3000, 50, 4), (2000, 256, 8),
                                   (700, 1433, 16), (40000, 128, 3),
                                   # the other (lanes per row, column tile) pairs: K <= 32, 64, 128, more; C <= 2, 4, 8, 16
                                   (500, 20, 4), (500, 32, 8), (500, 40, 2), (500, 64, 8), (500, 50, 16), (500, 100, 8),
                                   (500, 128, 16), (500, 300, 2), (500, 300, 4)])
def test_node_project(dev, n, K, C):
    """stag_node_project_fwd / _bwd: y = x w + b, and (dx, dw, db) from one pass, against float64 torch."""
    from stag_amd import ops
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.standard_normal((n, K)).astype(np.float32), device=dev, requires_grad=True)
    w = torch.tensor((rng.standard_normal((K, C)) / np.sqrt(K)).astype(np.float32), device=dev, requires_grad=True)
    b = torch.tensor(rng.standard_normal(C).astype(np.float32), device=dev, requires_grad=True)
    gy = torch.tensor(rng.standard_normal((n, C)).astype(np.float32), device=dev)
    y = ops._NodeProject.apply(x, w, b)      # (ops.node_project hands more than 8 columns to the library GEMM)
    y.backward(gy)
    xd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    ref = xd @ wd + bd
    ref.backward(gy.double())
    assert_close(y, ref.detach().cpu().numpy(), what="y")
    assert_close(x.grad, xd.grad.cpu().numpy(), what="dx")
    for got, r, nm in ((w.grad, wd.grad, "dw"), (b.grad, bd.grad, "db")):
        sc = max(1.0, float(r.abs().max()))
        assert_close(got / sc, (r / sc).cpu().numpy(), what=nm)
    if n:
        # no bias, no dx; and twice the same bits
        w2 = w.detach().clone().requires_grad_(True)
        y2 = ops._NodeProject.apply(x.detach(), w2, None)
        y2.backward(gy)
        assert_close(y2, (xd.detach() @ wd.detach()).cpu().numpy(), what="y, no bias")
        assert torch.equal(w2.grad, w.grad)


@pytest.mark.parametrize("hidden,n_par", [(1, 2), (1, 1), (2, 2), (3, 4), (8, 2)])
def test_edge_mlp(dev, hidden, n_par):
    """stag_edge_mlp_fwd / _bwd against the reference's dataflow in float64: SiLU(P_src[src] + P_dst[dst]) then
    one Linear(hidden -> 1) per parameter (stag/distributions.py:178-191, 225-231), with gradients to the
    projected tables and to the heads; hub rows on both sides."""
    from stag_amd import ops
    from util import random_graph
    rng = np.random.default_rng(8)
    n = 300
    g = random_graph(n, 4000, seed=12, hub=500, device=dev)
    src, dst = g.edges()
    E = g.number_of_edges()
    P = torch.tensor(rng.standard_normal((n, 2 * hidden)).astype(np.float32), device=dev, requires_grad=True)
    wh = torch.tensor(rng.standard_normal((hidden, n_par)).astype(np.float32), device=dev, requires_grad=True)
    bh = torch.tensor(rng.standard_normal(n_par).astype(np.float32), device=dev, requires_grad=True)
    gs = [torch.tensor(rng.standard_normal((E, 1)).astype(np.float32), device=dev) for _ in range(n_par)]
    outs = ops.edge_mlp(g, P, wh, bh)
    assert len(outs) == n_par and all(o.shape == (E, 1) for o in outs)
    torch.autograd.backward(outs, gs)
    Pd, whd, bhd = (t.detach().double().requires_grad_(True) for t in (P, wh, bh))
    h = torch.nn.functional.silu(Pd[src, :hidden] + Pd[dst, hidden:])
    ref = h @ whd + bhd
    ref.backward(torch.cat(gs, 1).double())
    for c in range(n_par):
        assert_close(outs[c], ref[:, c:c + 1].detach().cpu().numpy(), what=f"head {c}")
    for got, r, nm in ((P.grad, Pd.grad, "dP"), (wh.grad, whd.grad, "dwh"), (bh.grad, bhd.grad, "dbh")):
        sc = max(1.0, float(r.abs().max()))
        assert_close(got / sc, (r / sc).cpu().numpy(), what=nm)


@pytest.mark.parametrize("shape", [(5000, 1), (700, 16)])
@pytest.mark.parametrize("learn_prior", [False, True])
def test_normal_kl_mean(dev, shape, learn_prior):
    """stag_normal_kl_fwd / _bwd against torch.distributions.kl_divergence(...).mean() in float64
    (stag/layers.py:132-145), gradients to the heads and — when it is learned — to the prior."""
    from stag_amd import ops
    rng = np.random.default_rng(4)
    loc = torch.tensor(rng.normal(1.0, 0.4, shape).astype(np.float32), device=dev, requires_grad=True)
    ls = torch.tensor(rng.normal(-1.0, 0.5, shape).astype(np.float32), device=dev, requires_grad=True)
    pl = torch.tensor(0.8, device=dev, requires_grad=learn_prior)
    pls = torch.tensor(-0.4, device=dev, requires_grad=learn_prior)
    kl = ops.normal_kl_mean(loc, ls, pl, pls.exp())
    (kl * 1.7).backward()
    N = torch.distributions.Normal
    locd, lsd, pld, plsd = (t.detach().double().requires_grad_(t.requires_grad) for t in (loc, ls, pl, pls))
    ref = torch.distributions.kl_divergence(N(locd, lsd.exp()), N(pld, plsd.exp())).mean()
    (ref * 1.7).backward()
    assert_close(kl, ref.detach().cpu().numpy(), what="kl")
    n = loc.numel()
    assert_close(loc.grad * n, (locd.grad * n).cpu().numpy(), what="d loc")
    assert_close(ls.grad * n, (lsd.grad * n).cpu().numpy(), what="d log_scale")
    if learn_prior:
        assert_close(pl.grad, pld.grad.cpu().numpy(), what="d prior loc")
        assert_close(pls.grad, plsd.grad.cpu().numpy(), what="d prior log_scale")


@pytest.mark.parametrize("hidden", [None, 4])
def test_narrow_amortized_distribution_equals_dense_dataflow(dev, hidden):
    """AmortizedDistribution(in, 1) on a HIP device takes the three-kernel form (ops.node_project, ops.edge_mlp);
    its parameters and every gradient equal the reference's dataflow — cat([feat[src], feat[dst]]), Linear, SiLU,
    one Linear per head (stag/distributions.py:221-233) — evaluated in float64; and StagLayer.kl_divergence of the
    pair equals torch's closed form."""
    import copy
    import stag_amd
    from stag_amd.distributions import AmortizedDistribution
    from util import random_graph
    n, D = 200, 24
    g = random_graph(n, 2500, seed=3, hub=300, device=dev)
    src, dst = g.edges()
    torch.manual_seed(2)
    q = AmortizedDistribution(D, 1, hidden_features=hidden, init_like=torch.distributions.Normal(1.0, 0.3)).to(dev)
    for p in q.parameters():       # the default heads are near-constant: make every weight matter
        torch.nn.init.normal_(p, 0.0, 0.5)
    qd = copy.deepcopy(q).double()
    x = torch.randn(n, D, device=dev, requires_grad=True)
    xd = x.detach().double().requires_grad_(True)
    q.condition(g, x)
    assert q.new_parameters["loc"].grad_fn is not None and "EdgeMlp" in type(q.new_parameters["loc"].grad_fn).__name__
    h = qd.embedding_mlp(torch.cat([xd[src], xd[dst]], -1))
    ref = {k: qd.parameters_mlp[k](h) for k in qd.new_parameter_names}
    gl, gs = torch.randn(g.number_of_edges(), 1, device=dev), torch.randn(g.number_of_edges(), 1, device=dev)
    (q.new_parameters["loc"] * gl + q.new_parameters["log_scale"] * gs).sum().backward()
    (ref["loc"] * gl.double() + ref["log_scale"] * gs.double()).sum().backward()
    for k in ("loc", "log_scale"):
        assert_close(q.new_parameters[k], ref[k].detach().cpu().numpy(), what=k)
    sc = max(1.0, float(xd.grad.abs().max()))
    assert_close(x.grad / sc, (xd.grad / sc).cpu().numpy(), what="d feat")
    for (k, p), (_, pd) in zip(q.named_parameters(), qd.named_parameters()):
        sc = max(1.0, float(pd.grad.abs().max()))
        assert_close(p.grad / sc, (pd.grad / sc).cpu().numpy(), what=f"d {k}")
    # the layer's KL term
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, 8), q_a=q, vi=True).to(dev)
    layer(g, x.detach())
    kl = layer.kl_divergence()
    assert "NormalKlMean" in type(kl.grad_fn).__name__
    ref_kl = torch.distributions.kl_divergence(layer.q_a.base_distribution, layer.p_a.base_distribution).mean()
    assert_close(kl, ref_kl.detach().cpu().numpy(), what="layer KL")
    kl.backward()
    assert layer.p_a.loc.grad is not None and layer.q_a.parameters_mlp["log_scale"].weight.grad is not None


@pytest.mark.parametrize("n,H,F", [(1, 1, 4), (1000, 8, 32), (777, 3, 32), (500, 4, 64), (300, 2, 256), (2000, 16, 8),
                                   (900, 1, 128), (1200, 8, 40), (640, 5, 12), (333, 3, 124), (50, 1, 252),
                                   (400, 2, 32)])                # (2, 32): 16 lanes per row
def test_head_dot(dev, n, H, F):
    """stag_head_dot_fwd / _bwd: GAT's el / er = (ft * attn).sum(-1) (stag/zoo/gat.py:109-110) and the gradients
    to ft, attn_l, attn_r against float64 torch."""
    from stag_amd import ops
    rng = np.random.default_rng(11)
    ft = torch.tensor(rng.standard_normal((n, H, F)).astype(np.float32), device=dev, requires_grad=True)
    al = torch.tensor(rng.standard_normal((1, H, F)).astype(np.float32), device=dev, requires_grad=True)
    ar = torch.tensor(rng.standard_normal((1, H, F)).astype(np.float32), device=dev, requires_grad=True)
    gl, gr = (torch.tensor(rng.standard_normal((n, H)).astype(np.float32), device=dev) for _ in range(2))
    el, er = ops.head_dot(ft, al, ar)
    torch.autograd.backward([el, er], [gl, gr])
    ftd, ald, ard = (t.detach().double().requires_grad_(True) for t in (ft, al, ar))
    rl, rr = (ftd * ald).sum(-1), (ftd * ard).sum(-1)
    torch.autograd.backward([rl, rr], [gl.double(), gr.double()])
    assert_close(el, rl.detach().cpu().numpy(), what="el")
    assert_close(er, rr.detach().cpu().numpy(), what="er")
    assert_close(ft.grad, ftd.grad.cpu().numpy(), what="d ft")
    for got, r, nm in ((al.grad, ald.grad, "d attn_l"), (ar.grad, ard.grad, "d attn_r")):
        sc = max(1.0, float(r.abs().max()))
        assert_close(got / sc, (r / sc).cpu().numpy(), what=nm)
    assert ops.head_dot(torch.zeros(4, 2, 10, device=dev), al, ar) is None      # F % 4 != 0: the GEMM form


def test_fuzz_amortized_head_kernels(dev):
    """Seeded sweep over shapes for the narrow-head kernels of csrc/amort.hip — stag_node_project, stag_edge_mlp,
    stag_head_dot, stag_normal_kl, forward and backward — against float64 torch: row counts around the kernels' row
    and block granularities, odd widths, hub rows on both sides of the edge MLP.  STAG_FUZZ_SCALE multiplies the
    number of cases (profiles/r02/fuzz_soak.txt)."""
    import os
    from stag_amd import ops
    from util import random_graph
    rng = np.random.default_rng(20261007)
    scale = max(1, int(os.environ.get("STAG_FUZZ_SCALE", "1")))
    T = lambda a, grad=True: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=grad)

    def rel(got, ref, what):
        sc = max(1.0, float(ref.abs().max()))
        assert_close(got / sc, (ref / sc).cpu().numpy(), what=what)

    for it in range(16 * scale):
        # ---- node_project: y = x w + b ---------------------------------------------------------------------
        n = int(rng.choice([1, 3, 4, 5, 63, 64, 255, 257, 1000, 2049, int(rng.integers(1, 6000))]))
        K = int(rng.choice([1, 3, 4, 8, 9, 50, 127, 128, 200, 256, 515, 1433]))
        C = int(rng.integers(1, 9))
        what = f"amort fuzz {it}: n={n} K={K} C={C}"
        x, w, b = T(rng.standard_normal((n, K))), T(rng.standard_normal((K, C)) / np.sqrt(K)), T(rng.standard_normal(C))
        gy = T(rng.standard_normal((n, C)), False)
        y = ops._NodeProject.apply(x, w, b)
        y.backward(gy)
        xd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, w, b))
        ref = xd @ wd + bd
        ref.backward(gy.double())
        assert_close(y, ref.detach().cpu().numpy(), what=what + " node_project y")
        assert_close(x.grad, xd.grad.cpu().numpy(), what=what + " node_project dx")
        rel(w.grad, wd.grad, what + " node_project dw")
        rel(b.grad, bd.grad, what + " node_project db")
        # ---- edge_mlp: SiLU(P_src[src] + P_dst[dst]) -> heads ---------------------------------------------------
        hidden, n_par = int(rng.choice([1, 1, 2, 3, 4, 8])), int(rng.integers(1, 5))
        nn = int(rng.integers(2, 500))
        g = random_graph(nn, int(rng.integers(1, 5000)), seed=9500 + it, hub=int(rng.choice([0, 0, 300, 900])) if nn > 4 else 0,
                         device=dev)
        src, dst = g.edges()
        E = g.number_of_edges()
        what = f"amort fuzz {it}: n={nn} E={E} hidden={hidden} n_par={n_par}"
        P, wh, bh = T(rng.standard_normal((nn, 2 * hidden))), T(rng.standard_normal((hidden, n_par))), T(rng.standard_normal(n_par))
        gs = [T(rng.standard_normal((E, 1)), False) for _ in range(n_par)]
        outs = ops.edge_mlp(g, P, wh, bh)
        torch.autograd.backward(outs, gs)
        Pd, whd, bhd = (t.detach().double().requires_grad_(True) for t in (P, wh, bh))
        ref = torch.nn.functional.silu(Pd[src, :hidden] + Pd[dst, hidden:]) @ whd + bhd
        ref.backward(torch.cat(gs, 1).double())
        for c in range(n_par):
            assert_close(outs[c], ref[:, c:c + 1].detach().cpu().numpy(), what=what + f" edge_mlp head {c}")
        rel(P.grad, Pd.grad, what + " edge_mlp dP")
        rel(wh.grad, whd.grad, what + " edge_mlp dwh")
        rel(bh.grad, bhd.grad, what + " edge_mlp dbh")
        # ---- head_dot: el / er = (ft * attn).sum(-1) -----------------------------------------------------------
        H = int(rng.choice([1, 2, 3, 4, 5, 8, 16]))
        F = int(rng.choice([f for f in (4, 8, 12, 16, 32, 40, 64, 124, 128, 252, 256) if H * f <= 2048]))
        what = f"amort fuzz {it}: n={n} H={H} F={F}"
        ft, al, ar = T(rng.standard_normal((n, H, F))), T(rng.standard_normal((1, H, F))), T(rng.standard_normal((1, H, F)))
        gl, gr = T(rng.standard_normal((n, H)), False), T(rng.standard_normal((n, H)), False)
        lr = ops.head_dot(ft, al, ar)
        if lr is not None:
            torch.autograd.backward(list(lr), [gl, gr])
            ftd, ald, ard = (t.detach().double().requires_grad_(True) for t in (ft, al, ar))
            rl, rr = (ftd * ald).sum(-1), (ftd * ard).sum(-1)
            torch.autograd.backward([rl, rr], [gl.double(), gr.double()])
            assert_close(lr[0], rl.detach().cpu().numpy(), what=what + " head_dot el")
            assert_close(lr[1], rr.detach().cpu().numpy(), what=what + " head_dot er")
            assert_close(ft.grad, ftd.grad.cpu().numpy(), what=what + " head_dot d ft")
            rel(al.grad, ald.grad, what + " head_dot d attn_l")
            rel(ar.grad, ard.grad, what + " head_dot d attn_r")
        # ---- normal_kl_mean ------------------------------------------------------------------------------------
        shape = (int(rng.choice([1, 7, 256, 513, 5000, 70000])), int(rng.choice([1, 1, 3, 16])))
        what = f"amort fuzz {it}: kl {shape}"
        loc, ls = T(rng.normal(1.0, 0.4, shape)), T(rng.normal(-1.0, 0.5, shape))
        pl, pls = T(rng.normal(0.8, 0.2)), T(rng.normal(-0.4, 0.2))
        kl = ops.normal_kl_mean(loc, ls, pl, pls.exp())
        kl.backward()
        Nm = torch.distributions.Normal
        locd, lsd, pld, plsd = (t.detach().double().requires_grad_(True) for t in (loc, ls, pl, pls))
        ref = torch.distributions.kl_divergence(Nm(locd, lsd.exp()), Nm(pld, plsd.exp())).mean()
        ref.backward()
        m = loc.numel()
        assert_close(kl, ref.detach().cpu().numpy(), what=what + " kl")
        assert_close(loc.grad * m, (locd.grad * m).cpu().numpy(), what=what + " d loc")
        assert_close(ls.grad * m, (lsd.grad * m).cpu().numpy(), what=what + " d log_scale")
        assert_close(pl.grad, pld.grad.cpu().numpy(), what=what + " d prior loc")
        assert_close(pls.grad, plsd.grad.cpu().numpy(), what=what + " d prior log_scale")


@pytest.mark.parametrize("front", ["ctypes", "dispatcher"])
@pytest.mark.parametrize("n,E", [(5, 0), (1, 0), (3, 1)])
def test_layers_on_edgeless_and_one_edge_graphs(dev, n, E, front, monkeypatch):
    """Degenerate graphs through whole layers, forward and backward: no edges at all (per-edge arrays without an
    address; every gradient that flows through an edge is zero; the KL mean over zero edges is NaN as in the
    reference, stag/layers.py:136-139) and a single edge (an [E, 1] head of one element is still per edge)."""
    import stag_amd
    from stag_amd import ops
    from stag_amd.distributions import AmortizedDistribution
    N = torch.distributions.Normal
    if front == "dispatcher":       # (round 4) the same through torch.ops.stag.* — gat_fwd / gat_bwd / agg_fwd_mc / agg_bwd_dp too
        monkeypatch.setenv("STAG_TORCH_OPS", "1")
    g = stag_amd.Graph(torch.zeros(E, dtype=torch.int64), torch.full((E,), min(1, n - 1), dtype=torch.int64), n, device=dev)
    x = torch.randn(n, 8, device=dev, requires_grad=True)
    # a vi layer whose parameter gradients are finished in the dx pass, and a Monte-Carlo batch, on the same graphs
    vi = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(8, 4, allow_zero_in_degree=True), q_a=N(1.0, 0.5), vi=True, relu=True).to(dev)
    xv = torch.randn(n, 8, device=dev, requires_grad=True)
    (vi(g, xv).sum() + vi.kl_divergence()).backward()
    assert torch.isfinite(xv.grad).all() and all(torch.isfinite(p.grad).all() for p in vi.parameters() if p.grad is not None)
    with torch.no_grad():
        mc = ops.aggregate_mc(g, xv.detach(), stag_amd.EdgeNoise(g, 8, stag_amd._lib.NOISE_NORMAL, 1.0, 0.5, seed=1, offset=0), 3)
    assert mc.shape == (3, n, 8) and torch.isfinite(mc).all() and (E > 0 or float(mc.abs().sum()) == 0.0)
    q = AmortizedDistribution(8, 1, init_like=N(1.0, 0.3)).to(dev)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(8, 4, allow_zero_in_degree=True), q_a=q, vi=True).to(dev)
    y = layer(g, x)
    kl = layer.kl_divergence()
    assert y.shape == (n, 4) and torch.isfinite(y).all()
    assert torch.isnan(kl) if E == 0 else torch.isfinite(kl)
    (y.sum() + (kl if E else 0.0)).backward()
    assert torch.isfinite(x.grad).all()
    if E == 0:
        assert float(x.grad.abs().sum()) == 0.0 and float(layer.base_layer.weight.grad.abs().sum()) == 0.0
    else:
        assert float(q.embedding_mlp[0].weight.grad.abs().sum()) > 0.0
    for base in (stag_amd.zoo.GAT(8, 4, num_heads=2, allow_zero_in_degree=True),
                 stag_amd.zoo.GraphSAGE(8, 4, aggregator_type="mean"), stag_amd.zoo.GIN(8, 4)):
        lay = stag_amd.layers.StagLayer(base, q_a=N(1.0, 0.5)).to(dev)
        x2 = torch.randn(n, 8, device=dev, requires_grad=True)
        o = lay(g, x2)
        o.sum().backward()
        assert torch.isfinite(o).all() and torch.isfinite(x2.grad).all()


def test_new_backward_paths_are_bit_reproducible(dev):
    """Fixed-order reductions everywhere: the one-pass [E,1] backward, the narrow amortised heads, the KL, GAT's
    per-head dots and its one-gather backward, the parameter gradients finished in the dx pass (stag_agg_bwd_dp,
    with in-norm) give the same bits on every run (hub rows, segments, block partials included) — nothing is
    accumulated with atomics."""
    import stag_amd
    from stag_amd.distributions import AmortizedDistribution
    from util import random_graph
    N = torch.distributions.Normal
    n, D = 3000, 64
    g = random_graph(n, 40000, seed=5, hub=2500, device=dev)
    torch.manual_seed(3)
    x0 = torch.randn(n, D, device=dev)
    gout = torch.randn(n, D, device=dev)
    q = AmortizedDistribution(D, 1, init_like=N(1.0, 0.3)).to(dev)
    for p in q.parameters():
        torch.nn.init.normal_(p, 0.0, 0.3)
    re_layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, D), q_a=q, vi=True).to(dev)
    gat_layer = stag_amd.layers.StagLayer(stag_amd.zoo.GAT(D, 16, num_heads=4), q_a=N(1.0, 0.5)).to(dev)
    r1_layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, D), q_a=N(1.0, 0.5), vi=True, relu=True, norm=True).to(dev)

    def run(layer, with_kl):
        stag_amd.manual_seed(11)
        layer.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = layer(g, x)
        outs, grads = [y], [gout[:, :y.shape[1]]]
        if with_kl:
            outs.append(layer.kl_divergence())
            grads.append(torch.ones((), device=dev))
        torch.autograd.backward(outs, grads)
        return [y.detach().clone(), x.grad.clone()] + [o.detach().clone() for o in outs[1:]] + \
               [p.grad.clone() for p in layer.parameters() if p.grad is not None]

    for layer, with_kl in ((re_layer, True), (gat_layer, False), (r1_layer, True)):
        first = run(layer, with_kl)
        for _ in range(3):
            again = run(layer, with_kl)
            assert len(again) == len(first) and all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("H,F,last", [(3, 7, False), (8, 40, True), (2, 121, False), (4, 6, True), (1, 3, False)])
def test_gat_odd_head_widths_stay_fused(dev, H, F, last):
    """Head widths off the kernels' natural grid — the class counts on the last layer of the reference's GAT scripts,
    scripts/arxiv_mle/gat/run.py:50-58 — stay fused: F % 4 == 0 with F / 4 not a power of two (40) runs as it is, a
    head taking the next power of two lanes; F % 4 != 0 (7, 121, 6, 3) runs zero-padded to the next multiple of 4
    inside zoo.GAT.  Output, d/dx and every parameter gradient equal the layer's own statement on the composed
    path (torch ops over [E, H] + the aggregation kernel, unpadded), and the autograd graph holds the fused node."""
    import stag_amd
    from stag_amd import _lib, ops
    from util import random_graph
    n, D = 250, 24
    g = random_graph(n, 3000, seed=14, hub=400, device=dev)
    torch.manual_seed(5)
    gat = stag_amd.zoo.GAT(D, F, num_heads=H, last=last).to(dev)
    with torch.no_grad():
        gat.bias.copy_(torch.randn_like(gat.bias) * 0.1)
    x = torch.randn(n, D, device=dev, requires_grad=True)
    noise = stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=6, offset=1)
    y = gat(g, x, edge_weight=noise)
    assert y.shape == ((n, F) if last else (n, H * F))
    names = []
    node = y.grad_fn
    stack = [node]
    while stack and len(names) < 200:
        nd = stack.pop()
        if nd is None:
            continue
        names.append(type(nd).__name__)
        stack.extend(f for f, _ in nd.next_functions)
    assert any("GatAggregate" in nm for nm in names), "the fused GAT node is in the graph"
    gout = torch.randn_like(y)
    y.backward(gout)
    got = {"x": x.grad.clone(), **{k: p.grad.clone() for k, p in gat.named_parameters()}}
    # the same layer, unpadded, on the composed path
    x2 = x.detach().clone().requires_grad_(True)
    gat.zero_grad()
    ft = (x2 @ gat.fc.weight.t()).view(n, H, F)
    el, er = (ft * gat.attn_l).sum(-1), (ft * gat.attn_r).sum(-1)
    rst = ops._gat_composed(g, el, er, ft, 0.2, noise, None, False, 64) + gat.bias.view(1, H, F)
    ref = rst.mean(-2) if last else rst.flatten(-2, -1)
    assert_close(y, ref.detach().cpu().numpy(), what="output")
    ref.backward(gout)
    want = {"x": x2.grad, **{k: p.grad for k, p in gat.named_parameters()}}
    for k in got:
        sc = max(1.0, float(want[k].abs().max()))
        assert_close(got[k] / sc, (want[k] / sc).cpu().numpy(), what=f"d {k}")


def test_short_row_graphs_run_without_a_plan_until_they_are_reused(dev):
    """A batch of molecules (no row longer than HEAVY_LEN edges) is launched plan-less — building a plan costs a
    host round trip per minibatch graph — with the same bits as the planned launch; a view that keeps being
    launched gets its plan after PLAN_AFTER_LAUNCHES launches; the GAT kernels get one at once (need=True)."""
    import stag_amd
    import importlib
    from stag_amd import _lib, ops, synthetic
    G = importlib.import_module("stag_amd.graph")
    s, d, sizes = synthetic.molecules_like(256)
    n = int(sizes.sum())
    g = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), n, device=dev)
    assert g.csr._short_rows()
    x = torch.randn(n, 32, device=dev)
    mk = lambda: stag_amd.EdgeNoise(g, 32, _lib.NOISE_NORMAL, 1.0, 0.5, seed=2, offset=7)
    assert g.csr.plan(64) is None
    first = ops.aggregate(g, x, mk())
    for _ in range(G.PLAN_AFTER_LAUNCHES):
        ops.aggregate(g, x, mk())
    assert g.csr.plan(64) is not None                       # the view earned its plan
    assert torch.equal(ops.aggregate(g, x, mk()), first)    # and the planned launch gives the same bits
    g2 = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), n, device=dev)
    assert g2.csr.plan(64, need=True) is not None and g2.csr.plan(64, need=True)["n_blocks"] > 0
    hub = stag_amd.Graph(torch.zeros(40, dtype=torch.int64), torch.arange(40) % 2, 3, device=dev)   # a 20-edge row
    assert not hub.csr._short_rows() and hub.csr.plan(64) is not None


@pytest.mark.parametrize("n,D", [(20000, 121), (9000, 7), (100, 121), (30000, 128)])
def test_column_sum_and_bias_gradient(dev, n, D):
    """ops.column_sum / ops.add_bias: the bias gradient of odd widths (121 classes on PPI) by the readout kernel over
    row chunks — torch's reduction takes 575 us for [56,944, 121]."""
    from stag_amd import ops
    g = torch.randn(n, D, device=dev)
    ref = g.double().sum(0)
    sc = max(1.0, float(ref.abs().max()))
    assert_close(ops.column_sum(g) / sc, (ref / sc).cpu().numpy(), what="column_sum")
    x = torch.randn(n, D, device=dev, requires_grad=True)
    b = torch.randn(D, device=dev, requires_grad=True)
    y = ops.add_bias(x, b)
    y.backward(g)
    assert torch.equal(y.detach(), x.detach() + b.detach()) and torch.equal(x.grad, g)
    assert_close(b.grad / sc, (ref / sc).cpu().numpy(), what="d bias")


def test_masked_loss_equals_boolean_indexing(dev):
    """StagModel.loss with a boolean train mask (stag/models.py:73-76: `nll[mask].mean()`) applies the mask as a
    where(): the same value and gradients as the boolean index, no nonzero / size read-back on the step —
    Categorical ([N] log-probabilities) and Bernoulli ([N, C]) likelihoods, an infinite value outside the mask."""
    from stag_amd.models import _masked_mean
    torch.manual_seed(0)
    for shape in ((500,), (500, 7)):
        nll = torch.randn(*shape, device=dev, requires_grad=True)
        mask = torch.rand(500, device=dev) < 0.4
        got = _masked_mean(nll, mask)
        ref_in = nll.detach().clone().requires_grad_(True)
        ref = ref_in[mask].mean()
        got.backward(); ref.backward()
        assert torch.allclose(got, ref, rtol=1e-6, atol=1e-7) and torch.allclose(nll.grad, ref_in.grad, rtol=1e-6, atol=1e-8)
        poisoned = nll.detach().clone()
        poisoned[~mask] = float("inf")
        assert torch.isfinite(_masked_mean(poisoned, mask))
    idx = torch.tensor([1, 5, 9], device=dev)
    v = torch.randn(20, device=dev)
    assert torch.equal(_masked_mean(v, idx), v[idx].mean()) and torch.equal(_masked_mean(v, None), v.mean())


def test_steady_state_training_steps_do_not_synchronise_the_host(dev):
    """After the first steps (plans, cached degree vectors), a masked training step of every model family — fixed
    Bernoulli + in-norm GCN, vi GCN with the KL term, amortised GCN, GAT with feature and attention dropout,
    GraphSAGE — issues no synchronising torch call (torch's sync debug mode raises on .item(), nonzero, boolean
    indexing, device->host copies): the stream never waits for the host, and the step is capturable."""
    import stag_amd
    from util import random_graph
    n = 600
    g = random_graph(n, 9000, seed=5, hub=900, device=dev)
    x = torch.randn(n, 32, device=dev)
    y = torch.randint(0, 5, (n,), device=dev)
    mask = torch.rand(n, device=dev) < 0.5
    N = torch.distributions.Normal
    SL, Z = stag_amd.layers.StagLayer, stag_amd.zoo
    sm = lambda t: torch.softmax(t, -1)
    families = {
        "gcn bernoulli norm": [SL(Z.GCN(32, 16), q_a=torch.distributions.Bernoulli(0.9), norm=True),
                               SL(Z.GCN(16, 5, activation=sm), q_a=torch.distributions.Bernoulli(0.9), norm=True)],
        "gcn vi": [SL(Z.GCN(32, 16), q_a=N(1.0, 0.3), vi=True, relu=True), SL(Z.GCN(16, 5, activation=sm), q_a=N(1.0, 0.3), vi=True)],
        "gcn amortised": [SL(Z.GCN(32, 16), q_a=stag_amd.distributions.AmortizedDistribution(32, 1, init_like=N(1.0, 0.3)), vi=True),
                          SL(Z.GCN(16, 5, activation=sm), q_a=stag_amd.distributions.AmortizedDistribution(16, 1, init_like=N(1.0, 0.3)), vi=True)],
        "gat dropout": [SL(Z.GAT(32, 8, num_heads=4, feat_drop=0.5, attn_drop=0.5), q_a=N(1.0, 0.3)),
                        SL(Z.GAT(32, 5, num_heads=4, last=True, attn_drop=0.5, activation=sm), q_a=N(1.0, 0.3))],
        "sage": [SL(Z.GraphSAGE(32, 16, aggregator_type="mean"), q_a=N(1.0, 0.3)),
                 SL(Z.GraphSAGE(16, 5, aggregator_type="mean", activation=sm), q_a=N(1.0, 0.3))],
    }
    for name, layers in families.items():
        model = stag_amd.models.StagModel(layers=torch.nn.ModuleList(layers)).to(dev)
        opt = torch.optim.Adam(model.parameters(), 1e-3)

        def step():
            opt.zero_grad()
            loss = model.loss(g, x, y, mask=mask)
            loss.backward()
            opt.step()
            return loss
        for _ in range(12):
            step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                loss = step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.isfinite(loss), name


def test_cached_parameter_rows_follow_their_tensors(dev):
    """A non-learned distribution's device scalars travel to the kernel as per-channel rows that are kept per
    buffer tensor (launch-bound graphs: two small launches less per layer call).  The rows must follow the buffers:
    an in-place update, load_state_dict and .to() all show in the next forward."""
    import stag_amd
    from util import random_graph
    g = random_graph(200, 1500, seed=2, device=dev)
    x = torch.ones(200, 8, device=dev)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(8, 8, weight=False, bias=False, norm="none"),
                                      q_a=torch.distributions.Normal(2.0, 1e-6)).to(dev)

    def mean_out():
        stag_amd.manual_seed(3)
        with torch.no_grad():
            y = layer(g, x)
        deg = g.in_degrees().clamp(min=1).float().unsqueeze(1)
        return float((y / deg)[g.in_degrees() > 0].mean())
    assert abs(mean_out() - 2.0) < 1e-3 and abs(mean_out() - 2.0) < 1e-3          # second call: from the kept rows
    d1 = layer.q_a.base_distribution
    assert layer.q_a.base_distribution is d1                                        # kept while the buffers stand
    with torch.no_grad():
        layer.q_a.loc.fill_(5.0)                                                    # in-place: version bump
    assert layer.q_a.base_distribution is not d1 and abs(mean_out() - 5.0) < 1e-3
    sd = layer.state_dict()
    sd["q_a.loc"] = torch.tensor(7.0)
    layer.load_state_dict(sd)
    assert abs(mean_out() - 7.0) < 1e-3
    layer.q_a.loc = layer.q_a.loc.clone() * 0 + 9.0                                 # a new buffer tensor
    assert abs(mean_out() - 9.0) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(4, 64), (8, 32), (2, 16), (4, 256)])
def test_gat_with_xcd_aware_batches_equals_plan_order(dev, oracle, monkeypatch, H, F):
    """stag_plan_blocks_xcd only changes WHICH workgroup takes a batch of units (batch b belongs to stripe b mod 8 of the
    destination rows; empty batches where a stripe has run out): the cooperative GAT forward (noise, in-norm, attention
    dropout, get_attention), the one-gather and the two-pass backward and the in-kernel parameter gradients give what
    they give in plan order — forward and input gradients bit for bit — on a block-diagonal batch (the case it is for),
    on hubs cut into segments and on a graph with fewer units than stripes; forward also against the oracle."""
    import importlib
    import stag_amd
    from stag_amd import _lib, ops, synthetic
    from util import random_graph
    G = importlib.import_module("stag_amd.graph")
    s3, d3, sizes = synthetic.ppi_like(n_graphs=6, n_nodes=3000, n_edges=40000, seed=5)
    # "batch_graphs": the union knows its graphs (batch_num_nodes): batches of whole graphs per stripe, bin-packed
    # (stag_plan_blocks_xcd_ranges; the budget lowered so that these small graphs make several fine ranges)
    monkeypatch.setattr(G, "XCD_RANGE_BYTES", 150_000)
    graphs = [("batch", lambda: stag_amd.Graph(torch.from_numpy(s3), torch.from_numpy(d3), int(sizes.sum()), device=dev)),
              ("batch_graphs", lambda: stag_amd.Graph(torch.from_numpy(s3), torch.from_numpy(d3), int(sizes.sum()),
                                                      batch_num_nodes=torch.from_numpy(sizes).to(dev), device=dev)),
              ("hubs", lambda: random_graph(1500, 12000, seed=3, hub=2500, device=dev)),
              ("tiny", lambda: random_graph(5, 12, seed=9, device=dev))]
    if H * F > 256:
        graphs = graphs[:2]
    rng = np.random.default_rng(H * 100 + F)
    for name, mk in graphs:
        monkeypatch.setattr(G, "XCD_ORDER", "1")
        monkeypatch.setattr(G, "XCD_FINE", 3)
        ga = mk()
        pa = ga.csr.plan(64, need=True)                # (the policy is read when a plan is asked for)
        ga.csr_t.plan(64, need=True)
        monkeypatch.setattr(G, "XCD_ORDER", "0")
        gb = mk()
        pb = gb.csr.plan(64, need=True)
        gb.csr_t.plan(64, need=True)
        assert pa["xcd_on"] and not pb.get("xcd_on")
        if name == "batch_graphs":
            want = 1000 + min(H * F, 256) if H * F > 128 else 3       # rows of 1 KB and up (graph.GRAPHS_ABOVE); else XCD_FINE
            assert ga.csr.gat_blocks(pa, H * F)[3] == want, "the range-table batches are the ones launched"
        n, E = ga.number_of_nodes(), ga.number_of_edges()
        t = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32), device=dev)
        el0, er0, ft0, gout = t(n, H), t(n, H), t(n, H, F), t(n, H, F)
        og = oracle_graph(oracle, ga)
        cases = [("none", lambda g: None, oracle.make_spec("none"), None),
                 ("normal", lambda g: stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.3, seed=3, offset=1),
                  oracle.make_spec("normal", 1.0, 0.3, seed=3, offset=1, Dn=H, n_edges=E), None),
                 ("bernoulli+norm", lambda g: stag_amd.EdgeNoise(g, H, _lib.NOISE_BERNOULLI, 0.7, None, seed=3, offset=1, in_norm=True),
                  oracle.make_spec("bernoulli", 0.7, None, in_norm=True, seed=3, offset=1, Dn=H, n_edges=E), None),
                 ("normal+drop", lambda g: stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.3, seed=3, offset=1), None, (0.4, 11, 5))]
        for what, noise, spec, drop in cases:
            res = []
            for g in (ga, gb):
                el, er, ft = (v.clone().requires_grad_(True) for v in (el0, er0, ft0))
                out = ops.gat_aggregate(g, el, er, ft, 0.2, noise(g), attn_drop=drop)
                out.backward(gout)
                res.append((out.detach(), el.grad, er.grad, ft.grad))
            for a, b, nm in zip(res[0], res[1], ("out", "d el", "d er", "d ft")):
                assert torch.equal(a, b), f"{name} {what} H={H} F={F}: {nm}"
            if spec is not None:
                ref = oracle.gat_fwd(og, el0.cpu().numpy(), er0.cpu().numpy(), ft0.cpu().numpy(), 0.2, spec)
                ref = ref[0] if isinstance(ref, tuple) else ref
                assert_close(res[0][0], ref, what=f"{name} {what} forward vs oracle")
        if H * F <= 256:
            # get_attention and the two-pass backward
            with torch.no_grad():
                oa, aa = ops.gat_aggregate(ga, el0, er0, ft0, 0.2, cases[1][1](ga), want_attn=True)
                ob, ab = ops.gat_aggregate(gb, el0, er0, ft0, 0.2, cases[1][1](gb), want_attn=True)
            assert torch.equal(oa, ob) and torch.equal(aa, ab)
            monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", False)
            res = []
            for g in (ga, gb):
                el, er, ft = (v.clone().requires_grad_(True) for v in (el0, er0, ft0))
                ops.gat_aggregate(g, el, er, ft, 0.2, cases[1][1](g)).backward(gout)
                res.append((el.grad, er.grad, ft.grad))
            monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", True)
            for a, b, nm in zip(res[0], res[1], ("d el", "d er", "d ft")):
                assert torch.equal(a, b), f"{name} two-pass H={H} F={F}: {nm}"
            # vi=True: the parameter gradients finished in the kernels (block partials added in the new batch order)
            res = []
            for g in (ga, gb):
                loc = torch.full((H,), 1.0, device=dev, requires_grad=True)
                scale = torch.full((H,), 0.3, device=dev, requires_grad=True)
                el, er, ft = (v.clone().requires_grad_(True) for v in (el0, er0, ft0))
                noise = stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, loc, scale, seed=3, offset=1, differentiable=True)
                ops.gat_aggregate(g, el, er, ft, 0.2, noise).backward(gout)
                res.append((ft.grad, loc.grad, scale.grad))
            assert torch.equal(res[0][0], res[1][0])
            for a, b, nm in zip(res[0][1:], res[1][1:], ("d loc", "d scale")):
                sc = max(1.0, float(b.abs().max()))
                assert_close(a / sc, (b / sc).cpu().numpy(), what=f"{name} vi H={H} F={F}: {nm}")


@pytest.mark.gpu
def test_constant_inputs_of_odd_width_are_padded_once(dev):
    """PPI's 50 input features (BASELINE configs[2], layer 1): a tensor that carries no gradient and comes back unchanged
    is zero-padded to 52 columns ONCE, on its second sighting, and the launch runs its vector forms at the padded width —
    the result is a [:, :50] view of the padded output with the SAME bits as the unpadded launch (a Philox block covers 4
    channels either way); a tensor that changed is padded again; the dense transform behind it reads the view through its
    row stride (split-K weight gradient included)."""
    import stag_amd
    from stag_amd import _lib, ops
    from util import random_graph
    g = random_graph(3000, 40000, seed=4, hub=900, device=dev)
    n, D = g.number_of_nodes(), 50
    x = torch.randn(n, D, device=dev)
    mk = lambda: stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=8, offset=2)
    ops._const_pads.clear()
    first = ops.aggregate(g, x, mk(), reduce="mean")
    assert first.is_contiguous() and id(x) in ops._const_pads and ops._const_pads[id(x)][4] is None
    second = ops.aggregate(g, x, mk(), reduce="mean")
    third = ops.aggregate(g, x, mk(), reduce="mean")
    assert second.stride() == (52, 1) and second.shape == (n, D) and ops._const_pads[id(x)][4].shape == (n, 52)
    assert torch.equal(first, second) and torch.equal(first, third)
    assert torch.equal(ops.aggregate(g, x, None), ops.aggregate(g, x.clone(), None))           # (no noise; a fresh tensor: unpadded)
    x.mul_(2.0)                                                     # the constant changed: its padded copy must not be used
    again = ops.aggregate(g, x, mk(), reduce="mean")
    assert again.is_contiguous() and torch.equal(again, 2.0 * first)
    assert torch.equal(ops.aggregate(g, x, mk(), reduce="mean"), again)
    # per-channel parameters (what a layer hands over for a distribution whose parameters are module buffers): their rows
    # are extended to the padded width, the same bits; per-edge parameters and an input that carries a gradient: the plain path
    loc_r, sc_r = torch.rand(D, device=dev) + 0.5, torch.rand(D, device=dev) * 0.5 + 0.1
    pc = lambda: stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, loc_r, sc_r, seed=8, offset=2)
    plain = ops.aggregate(g, x.clone(), pc(), reduce="mean")
    for _ in range(3):
        got = ops.aggregate(g, x, pc(), reduce="mean")
        assert got.stride() == (52, 1) and torch.equal(got, plain)
    pe = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, torch.rand(g.number_of_edges(), 1, device=dev) + 0.5,
                            torch.rand(g.number_of_edges(), 1, device=dev) * 0.5 + 0.1, seed=8, offset=2)
    assert ops.aggregate(g, x, pe, reduce="mean").is_contiguous()
    xg = x.clone().requires_grad_(True)
    for _ in range(3):
        assert ops.aggregate(g, xg, mk()).is_contiguous()
    # the layer: GraphSAGE 50 -> 16 on a constant input, three steps; outputs and weight gradients do not depend on
    # whether the padded form ran
    torch.manual_seed(3)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GraphSAGE(D, 16, aggregator_type="mean"), q_a=torch.distributions.Normal(1.0, 0.5)).to(dev)
    feat = torch.randn(n, D, device=dev)
    outs, grads = [], []
    for step in range(3):
        stag_amd.manual_seed(5)
        layer.zero_grad()
        out = layer(g, feat)
        out.square().sum().backward()
        outs.append(out.detach().clone())
        grads.append(layer.base_layer.fc_neigh.weight.grad.clone())
    assert ops._const_pads[id(feat)][4] is not None, "the layer's constant input took the padded form from its second step"
    for o, gr in zip(outs[1:], grads[1:]):
        assert_close(o, outs[0].cpu().numpy(), what="SAGE on a padded constant input: output")
        sc = max(1.0, float(grads[0].abs().max()))
        assert_close(gr / sc, (grads[0] / sc).cpu().numpy(), what="SAGE on a padded constant input: d fc_neigh.weight")
