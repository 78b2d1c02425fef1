"""Monte-Carlo GAT forward on the GPU: stag_gat_fwd_mc / ops.gat_aggregate_mc against S separate stag_gat_fwd launches
(bit for bit, output and softmax statistics), against the oracle, across the counter space; the batched first GAT
layer of a StagModel against the sequential Monte-Carlo loop (values, generator offsets, gradients); the fallbacks."""
import copy

import pytest
import torch

from util import assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


@pytest.fixture(params=["ctypes", "torch_ops"])
def front(request, monkeypatch):
    """The ctypes binding or the dispatcher op (stag::gat_fwd_mc) under ops.*: the same library, two argument paths."""
    if request.param == "torch_ops":
        monkeypatch.setenv("STAG_TORCH_OPS", "1")
        from stag_amd import _torch_ext
        assert _torch_ext.available()
    else:
        monkeypatch.delenv("STAG_TORCH_OPS", raising=False)
    return request.param


def _noise(g, H, kind, pmode, relu, dev, **kw):
    import stag_amd
    from stag_amd import _lib
    k = {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM, "bernoulli": _lib.NOISE_BERNOULLI}[kind]
    gen = torch.Generator().manual_seed(H * 7 + len(kind))
    if kind == "bernoulli":
        p0, p1 = (0.7 if pmode == "scalar" else (0.3 + 0.6 * torch.rand(H, generator=gen)).to(dev)), None
    elif kind == "uniform":
        p0, p1 = ((0.5, 1.5) if pmode == "scalar" else ((0.2 + 0.5 * torch.rand(H, generator=gen)).to(dev),
                                                        (1.0 + torch.rand(H, generator=gen)).to(dev)))
    else:
        p0, p1 = ((1.0, 0.5) if pmode == "scalar" else ((0.5 + torch.rand(H, generator=gen)).to(dev),
                                                        (0.1 + 0.5 * torch.rand(H, generator=gen)).to(dev)))
    nz = stag_amd.EdgeNoise(g, H, k, p0, p1, relu=relu, **kw)
    assert nz.param_mode == (_lib.PARAM_SCALAR if pmode == "scalar" else _lib.PARAM_PER_CHANNEL)
    return nz


def _inputs(g, H, F, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    n = g.number_of_nodes()
    el = torch.randn(n, H, generator=gen).to(dev)
    er = torch.randn(n, H, generator=gen).to(dev)
    ft = torch.randn(n, H, F, generator=gen).to(dev)
    return el, er, ft


def _separate(g, el, er, ft, noise, S, stride, seg_len, dev):
    """S separate stag_gat_fwd launches at offset + s * stride: (out [S, N, H, F], stats [S, N, 2H])."""
    from stag_amd import ops
    H, F = ft.shape[1], ft.shape[2]
    n = g.csr.n_dst
    out = torch.full((S, n, H, F), float("nan"), device=dev)
    stats = torch.full((S, n, 2 * H), float("nan"), device=dev)
    for s in range(S):
        nz = copy.copy(noise)
        nz.offset = (noise.offset + s * stride) & M64
        ops._gat_fwd_into(g.csr, g.csr.plan(seg_len, need=True), el, er, ft, H, F, 0.2, nz.spec(), None, None,
                          out[s], stats[s], dev)
    return out, stats


# (H, F, kind, parameters, relu, S, seg_len): every row / lane shape class of the cooperative kernels — one chunk per
# lane (LPE 4..64, idle lanes for F / 4 not a power of two), two chunks, four chunks (2 samples per pass) — and
# S across whole and partial passes
CASES = [
    (8, 32, "normal", "scalar", False, 4, 64),         # cfg5's row
    (8, 32, "uniform", "head", True, 5, 64),
    (8, 32, "bernoulli", "scalar", False, 8, 16),
    (1, 8, "normal", "head", True, 3, 64),
    (4, 8, "bernoulli", "head", False, 2, 256),
    (16, 8, "uniform", "scalar", False, 4, 64),
    (4, 40, "normal", "head", False, 3, 32),
    (8, 40, "normal", "scalar", True, 4, 64),          # 2 chunks per lane
    (16, 32, "uniform", "head", False, 8, 64),         # 2 chunks per lane, 512 channels
    (4, 256, "normal", "scalar", False, 5, 64),        # 4 chunks per lane: 2 samples per pass, 3 passes
    (4, 256, "bernoulli", "head", True, 2, 16),
    (1, 256, "bernoulli", "scalar", True, 1, 64),
    (16, 64, "normal", "head", False, 3, 64),          # 1024 channels
]


@pytest.mark.parametrize("order", ["plain", "xcd"])
def test_gat_mc_bit_equal_to_separate_launches(dev, front, order, monkeypatch):
    import importlib
    from stag_amd import ops
    monkeypatch.setattr(importlib.import_module("stag_amd.graph"), "XCD_ORDER", "1" if order == "xcd" else "0")
    g = random_graph(700, 7000, seed=11, hub=1500, device=dev)      # the hub row is split into segments
    local = 0
    for i, (H, F, kind, pmode, relu, S, seg_len) in enumerate(CASES):
        assert ops.gat_cooperative_shape(H, F, seg_len)
        el, er, ft = _inputs(g, H, F, dev, seed=i)
        noise = _noise(g, H, kind, pmode, relu, dev, seed=0x5EED + i, offset=1000 * i + 3)
        stride = 1 + i % 3
        got, gstats = ops._gat_fwd_mc_raw(g.csr, el, er, ft, noise, S, stride, 0.2, seg_len, want_stats=True)
        ref, rstats = _separate(g, el, er, ft, noise, S, stride, seg_len, dev)
        assert got.shape == (S, g.number_of_nodes(), H, F) and gstats.shape == (S, g.number_of_nodes(), 2 * H)
        assert torch.equal(got, ref), (H, F, kind, pmode, S, seg_len)
        assert torch.equal(gstats, rstats), (H, F, kind, pmode, S, seg_len)
        # the public op: the same samples, and the stack of ordinary calls agrees
        assert torch.equal(ops.gat_aggregate_mc(g, el, er, ft, 0.2, noise, S, stride, seg_len=seg_len), ref)
        plan_t = g.csr.plan(seg_len, need=True)
        local += ops._gat_plan_args(g.csr, plan_t, dev, H * F)[4] is not None
    assert (local > 0) == (order == "xcd")


def test_gat_mc_against_the_oracle(dev, oracle):
    """Per sample against oracle.gat_fwd at offset + s * stride (hardware normals), on a hub graph and on cfg5 at full
    size (the arxiv-shaped graph, H = 8, F = 32) with S = 4."""
    import stag_amd
    from stag_amd import ops, synthetic
    src, dst = synthetic.arxiv_like(seed=1)
    big = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), synthetic.ARXIV_NODES, device=dev)
    for g, H, F, kind, S in ((random_graph(500, 5000, seed=3, hub=900, device=dev), 4, 40, "uniform", 3),
                             (big, 8, 32, "normal", 4)):
        el, er, ft = _inputs(g, H, F, dev, seed=7)
        noise = _noise(g, H, kind, "scalar", False, dev, seed=21, offset=77)
        got = ops.gat_aggregate_mc(g, el, er, ft, 0.2, noise, S, 3)
        og = oracle_graph(oracle, g)
        p = (0.5, 1.5) if kind == "uniform" else (1.0, 0.5)
        with hw_normals(oracle, dev):
            for s in range(S):
                spec = oracle.make_spec(kind, p[0], p[1], seed=21, offset=77 + 3 * s, Dn=H, n_edges=g.number_of_edges())
                ref = oracle.gat_fwd(og, el.cpu().numpy(), er.cpu().numpy(), ft.cpu().numpy(), 0.2, spec)
                assert_close(got[s], ref, what=f"H={H} F={F} sample {s}")


@pytest.mark.parametrize("regime", ["offset_wrap", "epoch", "pos_hi"])
def test_gat_mc_counter_regimes(dev, front, regime):
    """An offset and stride that wrap past 2^64 between samples, a device epoch, a pos_base with a nonzero high word:
    each sample stays the separate launch's, bit for bit."""
    from stag_amd import ops
    g = random_graph(600, 6000, seed=5, hub=700, device=dev)
    H, F, S = 8, 32, 5
    kw = {"offset_wrap": dict(seed=9, offset=M64 - 5),
          "epoch": dict(seed=9, offset=2**32 - 3, epoch=torch.tensor([7], dtype=torch.int64, device=dev)),
          "pos_hi": dict(seed=9, offset=11, pos_base=3 * 2**32 + 17)}[regime]
    stride = 3 if regime == "offset_wrap" else 2**40 + 1
    el, er, ft = _inputs(g, H, F, dev, seed=2)
    noise = _noise(g, H, "normal", "head", False, dev, **kw)
    got, gstats = ops._gat_fwd_mc_raw(g.csr, el, er, ft, noise, S, stride, 0.2, 64, want_stats=True)
    ref, rstats = _separate(g, el, er, ft, noise, S, stride, 64, dev)
    assert torch.equal(got, ref) and torch.equal(gstats, rstats)
    assert not torch.equal(got[0], got[1])


def _gat_model(dev, D, first_kw, second, gen):
    import stag_amd
    L, Z = stag_amd.layers, stag_amd.zoo
    N = torch.distributions.Normal
    layers = torch.nn.ModuleList([L.StagLayer(Z.GAT(D, **first_kw), generator=gen, q_a=N(1.0, 0.3)), second])
    return stag_amd.models.StagModel(layers).to(dev)


def _count_mc(layer):
    calls = []
    orig = layer.forward_mc

    def counted(*a, **k):
        out = orig(*a, **k)
        calls.append(out is not None)
        return out
    layer.forward_mc = counted
    return calls


@pytest.mark.parametrize("shape", ["arxiv", "ppi"])
def test_model_eval_batches_the_first_gat_layer(dev, shape):
    """model.eval() under no_grad with n_samples = 8 (the evaluation of scripts/arxiv_mle/gat/run.py and
    scripts/ppi_mle/gat/run.py): the first GAT layer's samples come from one gather per pass; forward and loss equal
    the sequential loop's bit for bit and the generator ends where the loop leaves it.  In train() with feature or
    attention dropout the loop runs and the results are unchanged."""
    import stag_amd
    from stag_amd.random import NoiseGenerator
    L, Z = stag_amd.layers, stag_amd.zoo
    N = torch.distributions.Normal
    n = 500
    g = stag_amd.add_self_loop(stag_amd.remove_self_loop(random_graph(n, 5000, seed=4, hub=600, device=dev)))
    gen = NoiseGenerator(seed=5)
    torch.manual_seed(3)
    if shape == "arxiv":      # GAT(128, 8, heads 8, elu) -> GAT(64, 40, heads 8, last, softmax)
        D, C = 32, 40
        first = dict(out_feats=8, num_heads=8, feat_drop=0.6, attn_drop=0.6, activation=torch.nn.functional.elu)
        second = L.StagLayer(Z.GAT(64, C, num_heads=8, last=True, feat_drop=0.6, attn_drop=0.6,
                                   activation=lambda t: torch.softmax(t, -1)), generator=gen, q_a=N(1.0, 0.3))
    else:                     # GAT(50, 256, heads 4, elu, no dropout) -> GAT(1024, 121, heads 6, last)
        D, C = 50, 12
        first = dict(out_feats=256, num_heads=4, activation=torch.nn.functional.elu, residual=True)
        second = L.StagLayer(Z.GAT(1024, C, num_heads=6, last=True, residual=True), generator=gen, q_a=N(1.0, 0.3))
    model = _gat_model(dev, D, first, second, gen)
    x = torch.randn(n, D, device=dev)
    y = torch.randint(0, C, (n,), device=dev)
    calls = _count_mc(model.layers[0])
    model.eval()

    def run(batched, fn):
        model._mc_batching_off = not batched
        gen.manual_seed(5)
        with torch.no_grad():
            r = fn()
        return r, gen.offset

    fwd = lambda: model(g, x, n_samples=8, return_parameters=True)
    loss = lambda: model.loss(g, x, y, n_samples=8)
    for fn in (fwd, loss):
        calls.clear()
        got, end_b = run(True, fn)
        assert calls and all(calls), "the batched first layer was not used"
        ref, end_s = run(False, fn)
        assert end_b == end_s == 16
        assert torch.equal(got, ref)
    # training with dropout: the loop (the layer does not batch), results unchanged
    model.train()
    if shape == "arxiv":
        assert not model.layers[0].base_layer.supports_edge_noise_mc
        calls.clear()
        torch.manual_seed(8)
        got, end_b = run(True, lambda: model.loss(g, x, y, n_samples=2))
        assert not any(calls)
        torch.manual_seed(8)
        ref, end_s = run(False, lambda: model.loss(g, x, y, n_samples=2))
        assert end_b == end_s and torch.equal(got, ref)
    else:
        assert model.layers[0].base_layer.supports_edge_noise_mc      # (no dropout: training batches too)
        model.layers[0].base_layer.attn_drop.p = 0.5
        assert not model.layers[0].base_layer.supports_edge_noise_mc
        model.layers[0].base_layer.attn_drop.p = 0.0


def test_training_batched_gat_first_layer_gradients(dev):
    """A GAT first layer without dropout trained with loss_terms(n_samples=4): the forward is batched
    (_GatAggregateMC), the backward the loop's per-sample one-gather passes; loss and every parameter gradient
    match the sequential loop."""
    import stag_amd
    from stag_amd.random import NoiseGenerator
    L, Z = stag_amd.layers, stag_amd.zoo
    N = torch.distributions.Normal
    n, D = 400, 24
    g = random_graph(n, 4000, seed=3, hub=300, device=dev)
    x = torch.randn(n, D, device=dev)
    y = torch.randint(0, 5, (n,), device=dev)
    mask = torch.rand(n, device=dev) < 0.6
    gen = NoiseGenerator(seed=5)
    torch.manual_seed(1)
    second = L.StagLayer(Z.GCN(32, 5, activation=lambda t: torch.softmax(t, -1)), generator=gen, q_a=N(1.0, 0.3), vi=True)
    model = _gat_model(dev, D, dict(out_feats=8, num_heads=4, activation=torch.nn.functional.elu, residual=True),
                       second, gen)
    model.train()
    calls = _count_mc(model.layers[0])

    def run(batched):
        model.zero_grad(set_to_none=True)
        model._mc_batching_off = not batched
        gen.manual_seed(5)
        nll, reg = model.loss_terms(g, x, y, mask=mask, n_samples=4)
        (nll + reg).backward()
        return nll.detach(), reg.detach(), gen.offset, {k: p.grad.clone() for k, p in model.named_parameters()
                                                        if p.grad is not None}

    nll_b, reg_b, end_b, gr_b = run(True)
    assert calls and all(calls), "the batched first layer was not used"
    nll_s, reg_s, end_s, gr_s = run(False)
    assert end_b == end_s == 8
    assert_close(torch.stack([nll_b, reg_b]), torch.stack([nll_s, reg_s]).cpu().numpy(), what="nll, kl")
    assert gr_b.keys() == gr_s.keys() and {"layers.0.base_layer.fc.weight", "layers.0.base_layer.attn_l"} <= gr_b.keys()
    for k in gr_s:
        sc = max(1.0, float(gr_s[k].abs().max()))
        assert_close(gr_b[k] / sc, (gr_s[k] / sc).cpu().numpy(), what=f"d {k}")


def test_gat_mc_fallbacks_are_the_stack(dev):
    """In-norm, vi=True parameters under autograd, a shape outside the cooperative kernels (H = 32) and CPU tensors
    take the stack of ordinary calls: the result is that stack's."""
    import stag_amd
    from stag_amd import _lib, ops

    def stack(g, el, er, ft, noise, S, stride):
        out = []
        for s in range(S):
            nz = copy.copy(noise)
            nz.offset = (noise.offset + s * stride) & M64
            out.append(ops.gat_aggregate(g, el, er, ft, 0.2, nz))
        return torch.stack(out, 0)

    g = random_graph(300, 3000, seed=8, hub=400, device=dev)
    el, er, ft = _inputs(g, 4, 8, dev, seed=1)
    nz = stag_amd.EdgeNoise(g, 4, _lib.NOISE_NORMAL, 1.0, 0.5, in_norm=True, seed=3, offset=5)
    assert torch.equal(ops.gat_aggregate_mc(g, el, er, ft, 0.2, nz, 3, 2), stack(g, el, er, ft, nz, 3, 2))
    el32, er32, ft32 = _inputs(g, 32, 4, dev, seed=2)
    nz = stag_amd.EdgeNoise(g, 32, _lib.NOISE_UNIFORM, 0.5, 1.5, seed=3, offset=5)
    assert not ops.gat_cooperative_shape(32, 4, 64)
    assert torch.equal(ops.gat_aggregate_mc(g, el32, er32, ft32, 0.2, nz, 3, 1), stack(g, el32, er32, ft32, nz, 3, 1))
    # vi=True: live parameters under autograd
    loc = torch.full((4,), 1.0, device=dev, requires_grad=True)
    scale = torch.full((4,), 0.5, device=dev, requires_grad=True)
    nz = stag_amd.EdgeNoise(g, 4, _lib.NOISE_NORMAL, loc, scale, seed=3, offset=5, differentiable=True)
    got = ops.gat_aggregate_mc(g, el, er, ft, 0.2, nz, 2, 1)
    ref = stack(g, el, er, ft, nz, 2, 1)
    assert torch.equal(got, ref) and got.grad_fn is not None
    got.sum().backward()
    assert loc.grad is not None and scale.grad is not None
    # CPU tensors: the stack (which refuses what has no device kernel, as gat_aggregate does)
    gc = random_graph(50, 300, seed=2)
    elc, erc, ftc = _inputs(gc, 4, 8, "cpu", seed=3)
    nzc = stag_amd.EdgeNoise(gc, 4, _lib.NOISE_NORMAL, 1.0, 0.5, seed=3, offset=5)
    try:
        ref = stack(gc, elc, erc, ftc, nzc, 2, 1)
    except Exception as exc:           # no CPU path in gat_aggregate: the MC call fails the same way
        with pytest.raises(type(exc)):
            ops.gat_aggregate_mc(gc, elc, erc, ftc, 0.2, nzc, 2, 1)
    else:
        assert torch.equal(ops.gat_aggregate_mc(gc, elc, erc, ftc, 0.2, nzc, 2, 1), ref)
