"""stag_sample_kl on the GPU: the sample-based KL estimate against a mixture-of-Normals prior and its parameter
gradients, from one pass that redraws the forward's sample from the counters (stag/layers.py:141-143).

Reference for every case, on the CPU in float64: z from EdgeNoise(g, Dn, NOISE_NORMAL, 0.0, 1.0, seed, offset[, pos_base])
.materialize() (the same counters), w = loc + s z (relu as configured), Normal(loc, s).log_prob(w) and mix.log_prob(w),
.sum(-1).mean(), autograd.  Bar: assert_close at TOL = 1e-5, gradients relative to max(1, |ref|max); the gradients of
[E, 1] parameters carry 1 / E and are compared times E, element by element."""
import numpy as np
import pytest
import torch

from util import TOL, assert_close, random_graph

pytestmark = pytest.mark.gpu

D = torch.distributions
SEED, OFFSET = 21, 5


def make_mix(K, dev):
    """K components with unequal weights, locs and scales (scales >= 0.3)."""
    j = torch.arange(K, dtype=torch.float32)
    probs = (1.0 + j) / (1.0 + j).sum()
    loc = -0.5 + 2.0 * j / max(K - 1, 1) if K > 1 else torch.tensor([0.4])
    scale = 0.3 + 0.2 * j
    return D.MixtureSameFamily(D.Categorical(probs.to(dev)), D.Normal(loc.to(dev), scale.to(dev)))


def mix64(mix):
    c = mix.component_distribution
    return D.MixtureSameFamily(D.Categorical(logits=mix.mixture_distribution.logits.cpu().double()),
                               D.Normal(c.loc.cpu().double(), c.scale.cpu().double()))


def std_draw(g, dn, seed=SEED, offset=OFFSET, pos_base=0):
    import stag_amd
    from stag_amd import _lib
    return stag_amd.EdgeNoise(g, dn, _lib.NOISE_NORMAL, 0.0, 1.0, seed=seed, offset=offset,
                              pos_base=pos_base).materialize().cpu().double()


def reference(z, p0, p1, p1_log, relu, mix):
    """(kl, d kl / d p0, d kl / d p1) in float64 from the fp32 parameter values p0, p1 (numbers or tensors)."""
    a = torch.as_tensor(p0, dtype=torch.float32).detach().cpu().double().requires_grad_(True)
    b = torch.as_tensor(p1, dtype=torch.float32).detach().cpu().double().requires_grad_(True)
    s = b.exp() if p1_log else b
    w = a + s * z
    if relu:
        w = w.relu()
    kl = D.Normal(a, s).log_prob(w).sum(-1).mean() - mix64(mix).log_prob(w).sum(-1).mean()
    kl.backward()
    return kl.detach().numpy(), a.grad.numpy(), b.grad.numpy()


def assert_grad_close(got, ref, what):
    sc = max(1.0, float(np.abs(ref).max()))
    assert_close(got.detach().cpu().numpy().reshape(ref.shape) / sc, ref / sc, what=what)


def assert_edge_grad_close(got, ref, what):
    """One edge's gradient is 1 / E of an O(1) number: times E, at the plain bar (no division by the largest)."""
    E = ref.shape[0]
    assert_close(got.detach().cpu().numpy().reshape(ref.shape).astype(np.float64) * E, ref * E, what=what)


def params(mode, relu, E, dn, dev):
    """(p0, p1, p1_log) of the sweep.  The relu cases draw around loc = 0.2, scale = 0.8: a good share is clipped."""
    if mode == "scalar":
        return (0.2, 0.8, False) if relu else (1.0, 0.5, False)
    if mode == "per_channel":
        k = torch.arange(dn, dtype=torch.float32)
        p0, p1 = (torch.full((dn,), 0.2), torch.full((dn,), 0.8)) if relu else (1.0 + 0.1 * k, 0.5 + 0.05 * k)
        return p0.to(dev).requires_grad_(True), p1.to(dev).requires_grad_(True), False
    gen = torch.Generator().manual_seed(3)
    p0 = (0.2 if relu else 1.0) + 0.2 * torch.randn(E, 1, generator=gen) * (0.0 if relu else 1.0)
    p1 = float(np.log(0.8 if relu else 0.5)) + 0.1 * torch.randn(E, 1, generator=gen) * (0.0 if relu else 1.0)
    return p0.to(dev).requires_grad_(True), p1.to(dev).requires_grad_(True), True


@pytest.fixture(scope="module")
def graphs(dev):
    import stag_amd
    hub = random_graph(120, 900, seed=12, hub=100, device=dev)       # a non-identity eid, a 100-edge row, an empty row
    one = stag_amd.Graph(torch.tensor([0]), torch.tensor([1]), 2, device=dev)
    return {"hub": hub, "one": one}


_DRAWS = {}


def shared_draw(graphs, name, dn):
    """The standard draw of (graph, Dn) at (SEED, OFFSET), computed once and left unchanged."""
    if (name, dn) not in _DRAWS:
        _DRAWS[name, dn] = std_draw(graphs[name], dn)
    return _DRAWS[name, dn]


@pytest.mark.parametrize("gname", ["hub", "one"])
@pytest.mark.parametrize("dn", [1, 4, 6, 8, 16, 32, 64, 128])      # 16 ... 128: 4, 8, 16 and 32 lanes per position
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("mode", ["scalar", "per_channel", "per_edge1"])
def test_value_and_gradients_over_the_sweep(dev, graphs, mode, relu, dn, gname):
    import stag_amd
    from stag_amd import _lib, ops
    g = graphs[gname]
    E = g.number_of_edges()
    z = shared_draw(graphs, gname, dn)
    for K in (1, 2, 5):
        mix = make_mix(K, dev)
        p0, p1, p1_log = params(mode, relu, E, dn, dev)
        noise = stag_amd.EdgeNoise(g, dn, _lib.NOISE_NORMAL, p0, p1, relu=relu, seed=SEED, offset=OFFSET,
                                   differentiable=True, p1_log=p1_log)
        assert noise.param_mode == {"scalar": _lib.PARAM_SCALAR, "per_channel": _lib.PARAM_PER_CHANNEL,
                                    "per_edge1": _lib.PARAM_PER_EDGE1}[mode]
        assert ops.sampled_kl_why_not(noise, mix) is None
        ref, r0, r1 = reference(z, p0, p1, p1_log, relu, mix)
        what = f"{gname} {mode} relu={relu} Dn={dn} K={K}"
        kl = ops.sampled_kl_mean(noise, mix)
        assert kl.shape == torch.Size([])
        assert_close(kl, ref, what=what + " kl")
        if mode == "scalar":
            # numbers carry no gradient: the plain value; the entry point's [1] gradients are the reference's sums
            assert not kl.requires_grad
            _, d0, d1 = ops._sample_kl_raw(noise, mix, True)
            assert_grad_close(d0, r0.reshape(1), what + " d p0")
            assert_grad_close(d1, r1.reshape(1), what + " d p1")
            continue
        assert kl.requires_grad
        kl.backward()
        close = assert_edge_grad_close if mode == "per_edge1" else assert_grad_close
        close(p0.grad, r0, what + " d p0")
        close(p1.grad, r1, what + " d p1")
        with torch.no_grad():
            assert_close(ops.sampled_kl_mean(noise, mix), ref, what=what + " kl (no grad)")


def test_wide_rows_loop_over_chunk_tiles(dev):
    """Dn = 260: 65 chunks, so a team of 64 lanes walks two tiles per edge; [E, 1] parameters."""
    import stag_amd
    from stag_amd import _lib, ops
    g = random_graph(40, 300, seed=5, device=dev)
    E, dn = g.number_of_edges(), 260
    mix = make_mix(2, dev)
    for relu in (False, True):
        p0, p1, p1_log = params("per_edge1", relu, E, dn, dev)
        noise = stag_amd.EdgeNoise(g, dn, _lib.NOISE_NORMAL, p0, p1, relu=relu, seed=SEED, offset=OFFSET,
                                   differentiable=True, p1_log=True)
        ref, r0, r1 = reference(std_draw(g, dn), p0, p1, True, relu, mix)
        kl = ops.sampled_kl_mean(noise, mix)
        kl.backward()
        assert_close(kl, ref, what=f"Dn=260 relu={relu} kl")
        assert_edge_grad_close(p0.grad, r0, f"Dn=260 relu={relu} d loc")
        assert_edge_grad_close(p1.grad, r1, f"Dn=260 relu={relu} d log_scale")
    # per-channel rows of that width: the channel tiles are blocks of their own
    k = torch.arange(dn, dtype=torch.float32)
    p0 = (1.0 + 0.001 * k).to(dev).requires_grad_(True)
    p1 = (0.5 + 0.001 * k).to(dev).requires_grad_(True)
    noise = stag_amd.EdgeNoise(g, dn, _lib.NOISE_NORMAL, p0, p1, seed=SEED, offset=OFFSET, differentiable=True)
    ref, r0, r1 = reference(std_draw(g, dn), p0, p1, False, False, mix)
    kl = ops.sampled_kl_mean(noise, mix)
    kl.backward()
    assert_close(kl, ref, what="Dn=260 per-channel kl")
    assert_grad_close(p0.grad, r0, "Dn=260 per-channel d loc")
    assert_grad_close(p1.grad, r1, "Dn=260 per-channel d scale")


@pytest.mark.parametrize("mode", ["scalar", "per_channel", "per_edge1"])
def test_two_calls_are_bit_identical(dev, graphs, mode):
    import stag_amd
    from stag_amd import _lib, ops
    g = graphs["hub"]
    mix = make_mix(5, dev)
    p0, p1, p1_log = params(mode, True, g.number_of_edges(), 6, dev)
    noise = stag_amd.EdgeNoise(g, 6, _lib.NOISE_NORMAL, p0, p1, relu=True, seed=SEED, offset=OFFSET, p1_log=p1_log)
    first = ops._sample_kl_raw(noise, mix, True)
    second = ops._sample_kl_raw(noise, mix, True)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.equal(ops._sample_kl_raw(noise, mix, False)[0], first[0])       # the value does not depend on the gradients


@pytest.mark.parametrize("pos_base", [(1 << 32) - 450, (1 << 32) - 1550])
def test_position_base_next_to_the_2_32_boundary(dev, graphs, pos_base):
    """The 1000 positions from 2^32 - 450 on (they pass the boundary after 450) and from 2^32 - 1550 on (they end 550
    short of it) draw what the materialised noise draws at the same pos_base."""
    import stag_amd
    from stag_amd import _lib, ops
    g = graphs["hub"]
    assert g.number_of_edges() == 1000
    mix = make_mix(2, dev)
    p0, p1, _ = params("per_channel", True, 1000, 6, dev)
    noise = stag_amd.EdgeNoise(g, 6, _lib.NOISE_NORMAL, p0, p1, relu=True, seed=SEED, offset=OFFSET, pos_base=pos_base,
                               differentiable=True)
    z = std_draw(g, 6, pos_base=pos_base)
    assert not torch.equal(z, shared_draw(graphs, "hub", 6))
    ref, r0, r1 = reference(z, p0, p1, False, True, mix)
    kl = ops.sampled_kl_mean(noise, mix)
    kl.backward()
    assert_close(kl, ref, what="pos_base kl")
    assert_grad_close(p0.grad, r0, "pos_base d loc")
    assert_grad_close(p1.grad, r1, "pos_base d scale")


def test_device_epoch_is_added_to_the_offset(dev, graphs):
    import stag_amd
    from stag_amd import _lib, ops
    g = graphs["hub"]
    mix = make_mix(2, dev)
    epoch = torch.full((1,), 3, dtype=torch.int64, device=dev)
    with_epoch = stag_amd.EdgeNoise(g, 8, _lib.NOISE_NORMAL, 1.0, 0.5, seed=SEED, offset=OFFSET, epoch=epoch)
    plain = stag_amd.EdgeNoise(g, 8, _lib.NOISE_NORMAL, 1.0, 0.5, seed=SEED, offset=OFFSET + 3)
    other = stag_amd.EdgeNoise(g, 8, _lib.NOISE_NORMAL, 1.0, 0.5, seed=SEED, offset=OFFSET)
    got, want, base = (ops._sample_kl_raw(n, mix, True) for n in (with_epoch, plain, other))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], base[0])


# ---- layer level -----------------------------------------------------------------------------------------------------
def _layer_reference(layer, g, dn, relu, mix):
    """From the layer's descriptor after a forward: the float64 statement on the same counters."""
    h = layer._edge_weight_handle
    z = std_draw(g, dn, seed=h.seed, offset=h.offset)
    return h, z


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("base", ["gcn", "gat"])
def test_layer_keeps_the_descriptor_and_learned_scalars_get_the_gradients(dev, graphs, base, relu):
    import stag_amd
    g = graphs["hub"]
    Dw = 8
    mix = make_mix(2, dev)
    net = stag_amd.zoo.GCN(Dw, 4) if base == "gcn" else stag_amd.zoo.GAT(Dw, 4, num_heads=3)
    dn = Dw if base == "gcn" else 3
    layer = stag_amd.layers.StagLayer(net, q_a=D.Normal(1.0, 0.5), p_a=mix, vi=True, relu=relu).to(dev)
    x = torch.randn(120, Dw, device=dev)
    stag_amd.manual_seed(33)
    layer(g, x)
    assert isinstance(layer._edge_weight_handle, stag_amd.EdgeNoise)
    kl = layer.kl_divergence()
    assert isinstance(layer._edge_weight_handle, stag_amd.EdgeNoise), "the handle stays a descriptor"
    assert layer._kl_sampled and kl.requires_grad
    kl.backward()
    h, z = _layer_reference(layer, g, dn, relu, mix)
    assert h.dn == dn
    ref, r0, r1 = reference(z, layer.q_a.loc, layer.q_a.log_scale, True, relu, mix)
    assert_close(kl, ref, what=f"{base} layer kl")
    assert_grad_close(layer.q_a.loc.grad, r0, f"{base} layer d loc")
    assert_grad_close(layer.q_a.log_scale.grad, r1, f"{base} layer d log_scale")


def test_layer_with_amortized_heads(dev, graphs):
    import stag_amd
    from stag_amd.distributions import AmortizedDistribution
    g = graphs["hub"]
    Dw = 8
    mix = make_mix(2, dev)
    torch.manual_seed(4)
    q = AmortizedDistribution(Dw, 1, init_like=D.Normal(1.0, 0.3))
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(Dw, 4), q_a=q, p_a=mix, vi=True).to(dev)
    x = torch.randn(120, Dw, device=dev)
    stag_amd.manual_seed(34)
    layer(g, x)
    kl = layer.kl_divergence()
    h = layer._edge_weight_handle
    assert isinstance(h, stag_amd.EdgeNoise) and h.p1_log and kl.requires_grad
    loc, ls = layer.q_a.new_parameters["loc"], layer.q_a.new_parameters["log_scale"]
    assert loc.shape == (1000, 1)
    ref, r0, r1 = reference(std_draw(g, Dw, seed=h.seed, offset=h.offset), loc, ls, True, False, mix)
    assert_close(kl, ref, what="amortized layer kl")
    heads = [p for p in layer.q_a.parameters() if p.requires_grad]
    # the reference's gradients of the heads' parameters: its [E, 1] gradients sent through the same heads
    want = torch.autograd.grad([loc, ls], heads, [torch.from_numpy(r0).float().to(dev), torch.from_numpy(r1).float().to(dev)],
                               retain_graph=True, allow_unused=True)
    kl.backward()
    assert any(w is not None and float(w.abs().max()) > 0 for w in want)
    for p, w in zip(heads, want):
        if w is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
            continue
        assert_grad_close(p.grad, w.cpu().double().numpy(), "amortized head gradient")


def test_no_edge_by_channel_tensor_is_allocated(dev):
    """E = 20,000, Dn = 64: from just before kl_divergence() to after backward() the peak allocation stays below a
    quarter of ONE [E, Dn] fp32 tensor (5.1 MB); the composed route holds several."""
    import stag_amd
    E, dn = 20000, 64
    g = random_graph(2000, E, seed=8, device=dev)
    assert g.number_of_edges() == E
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(dn, 4), q_a=D.Normal(1.0, 0.5), p_a=make_mix(2, dev), vi=True).to(dev)
    x = torch.randn(2000, dn, device=dev)
    for _ in range(2):                       # the second pass measures: plans and workspaces of the forward exist
        for p in layer.parameters():
            p.grad = None
        stag_amd.manual_seed(35)
        layer(g, x)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        kl = layer.kl_divergence()
        kl.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    print(f"peak allocation over kl_divergence() + backward(): {peak} bytes; one [E, Dn] tensor: {E * dn * 4}")
    assert peak < E * dn * 4 / 4, peak
    assert float(layer.q_a.loc.grad.abs()) > 0


def test_composed_route_is_intact(dev, graphs, monkeypatch):
    """ops.SAMPLED_KL_FUSED = False, or norm=True: the old lines run, on the materialised sample, and return what they
    returned; the fused and composed values agree."""
    import stag_amd
    from stag_amd import ops
    g = graphs["hub"]
    mix = make_mix(2, dev)
    x = torch.randn(120, 8, device=dev)

    def run(norm, fused):
        monkeypatch.setattr(ops, "SAMPLED_KL_FUSED", fused)
        layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(8, 4), q_a=D.Normal(1.0, 0.5), p_a=mix, vi=True, relu=True,
                                          norm=norm).to(dev)
        stag_amd.manual_seed(36)
        layer(g, x)
        kl = layer.kl_divergence()
        kl.backward()
        return layer, kl.detach(), layer.q_a.loc.grad.clone(), layer.q_a.log_scale.grad.clone()

    fused = run(False, True)
    assert isinstance(fused[0]._edge_weight_handle, stag_amd.EdgeNoise)
    for norm, switch in ((False, False), (True, True), (True, False)):
        layer, kl, d0, d1 = run(norm, switch)
        w = layer._edge_weight_handle
        assert torch.is_tensor(w) and w.shape == (1000, 8), "the composed route materialises the sample"
        old = (layer.q_a.log_prob(w).sum(dim=-1).mean() - layer.p_a.log_prob(w).sum(dim=-1).mean()).detach()
        assert torch.equal(kl, old)
        if not norm:
            assert_close(fused[1], kl.cpu().numpy(), what="fused against composed kl")
            assert_grad_close(fused[2], d0.cpu().double().numpy(), "fused against composed d loc")
            assert_grad_close(fused[3], d1.cpu().double().numpy(), "fused against composed d log_scale")
