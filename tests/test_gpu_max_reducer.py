"""The fused max reducer (stag_agg_max_fwd / stag_agg_max_bwd; ops.aggregate_max on the GPU) against restatements:
the forward bit for bit against scatter-amax of the fp32 messages x[src] * w (w from EdgeNoise.materialize(), which the
suite pins against the oracle), the backward against a float64 restatement of the equal-share rule."""
import pytest
import torch

from util import assert_close, random_graph

pytestmark = pytest.mark.gpu
N_, U_, B_ = 2, 3, 4     # NOISE_NORMAL, NOISE_UNIFORM, NOISE_BERNOULLI


def _edges(g):
    src, dst = g.edges()
    return src.long(), dst.long()


def _restate(g, x, w):
    """(out, cnt) of the fp32 messages m = x[src] * w: zeros.scatter_reduce(amax), and the tie counts; on the CPU."""
    src, dst = (t.cpu() for t in _edges(g))
    xc = x.detach().float().cpu()
    D = xc.shape[1]
    m = xc[src] if w is None else xc[src] * w.detach().float().cpu()
    n = g.number_of_nodes()
    idx = dst.unsqueeze(1).expand(-1, D)
    out = torch.zeros(n, D).scatter_reduce(0, idx, m, "amax", include_self=False)
    cnt = torch.zeros(n, D, dtype=torch.int32).scatter_add(0, idx, (m == out[dst]).int())
    return out, cnt, m


def _noise(g, D, kind, mode, relu, dev, seed=7, offset=3, **kw):
    import stag_amd
    E = g.number_of_edges()
    gen = torch.Generator().manual_seed(1234 + D + 10 * kind + mode)

    def par(lo, hi):
        shape = {0: (), 1: (D,), 2: (E, 1), 3: (E, D)}[mode]
        t = lo + (hi - lo) * torch.rand(shape, generator=gen)
        return float(t) if mode == 0 else t.to(dev)
    if kind == N_:
        p0, p1 = par(-0.5, 1.0), par(0.3, 1.2)
    elif kind == U_:
        p0, p1 = par(-0.5, 0.2), par(0.5, 1.5)
    else:
        p0, p1 = par(0.2, 0.8), None
    return stag_amd.EdgeNoise(g, D, kind, p0, p1, relu=relu, seed=seed, offset=offset, **kw)


def _fused(g, x, weight, seg_len=64):
    from stag_amd import ops
    with torch.no_grad():
        return ops.aggregate_max(g, x, weight, seg_len=seg_len)


def _raw_fwd(g, x, weight, seg_len=64):
    """(out, cnt) straight from the ctypes binding."""
    from stag_amd import ops
    if weight is None:
        spec = ops._none_spec()
    elif torch.is_tensor(weight):
        spec = ops._explicit_spec(weight.contiguous())
    else:
        spec = ops._noise_spec(weight)
    return ops._max_fwd_raw(g.csr, x, x.shape[1], ops._targs_or_c(spec), seg_len, True)


GRAPHS = {
    "hub": lambda dev: random_graph(300, 2500, seed=5, hub=700, device=dev),     # zero-in-degree rows, many segments
    "one_edge": lambda dev: random_graph(4, 1, seed=2, device=dev),
    "no_edges": lambda dev: random_graph(5, 0, seed=2, device=dev),
}


@pytest.mark.parametrize("D", [1, 3, 4, 8, 12, 32, 50, 128, 256, 300, 1433])     # 8, 32: 2 and 8 lanes per row
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_forward_exact_across_widths(dev, D, gname):
    g = GRAPHS[gname](dev)
    torch.manual_seed(D)
    x = torch.randn(g.number_of_nodes(), D, device=dev)
    noise = _noise(g, D, N_, 1, False, dev)
    out, cnt = _raw_fwd(g, x, noise)
    ref, rcnt, _ = _restate(g, x, noise.materialize() if g.number_of_edges() else None)
    assert torch.equal(out.cpu(), ref) and torch.equal(cnt.cpu(), rcnt)
    assert torch.equal(_fused(g, x, noise).cpu(), ref)
    out0, cnt0 = _raw_fwd(g, x, None)                       # no weight
    ref0, rcnt0, _ = _restate(g, x, None)
    assert torch.equal(out0.cpu(), ref0) and torch.equal(cnt0.cpu(), rcnt0)


KIND_CASES = [(k, 0) for k in ("none", "explicit")] + [(k, m) for k in (N_, U_, B_) for m in (0, 1, 3)]


@pytest.mark.parametrize("kind,mode", KIND_CASES)
@pytest.mark.parametrize("relu", [False, True])
def test_forward_exact_kinds_and_parameters(dev, kind, relu, mode):
    import stag_amd
    from stag_amd import ops
    g = GRAPHS["hub"](dev)
    D = 50
    torch.manual_seed(3)
    x = torch.randn(g.number_of_nodes(), D, device=dev)
    if kind == "none":
        w, wm = None, None
    elif kind == "explicit":
        w = torch.randn(g.number_of_edges(), D, device=dev)
        wm = w.relu() if relu else w
        spec = ops._explicit_spec(w, relu=relu)
        out, cnt = ops._max_fwd_raw(g.csr, x, D, ops._targs_or_c(spec), 64, True)
        ref, rcnt, _ = _restate(g, x, wm)
        assert torch.equal(out.cpu(), ref) and torch.equal(cnt.cpu(), rcnt)
        w = wm
    else:
        w = _noise(g, D, kind, mode, relu, dev)
        wm = w.materialize()
    out, cnt = _raw_fwd(g, x, w)
    ref, rcnt, _ = _restate(g, x, wm)
    assert torch.equal(out.cpu(), ref) and torch.equal(cnt.cpu(), rcnt)
    if kind == N_ and mode == 0:                                  # [E, 1] parameters and log-scales too
        E = g.number_of_edges()
        for p1_log in (False, True):
            nz = stag_amd.EdgeNoise(g, D, N_, torch.rand(E, 1, device=dev), torch.rand(E, 1, device=dev) - 0.5,
                                    relu=relu, seed=11, offset=2, p1_log=p1_log)
            out, cnt = _raw_fwd(g, x, nz)
            ref, rcnt, _ = _restate(g, x, nz.materialize())
            assert torch.equal(out.cpu(), ref) and torch.equal(cnt.cpu(), rcnt)


def test_ties_zeros_and_nan(dev):
    """-0.0 vs +0.0: the first maximal message in CSR order keeps its bits, both count; all-negative rows are their
    maximum, not 0; a NaN message makes the row NaN; a row without in-edges is +0.0."""
    import stag_amd
    # dst 0 <- sources 0 (-0.0), 1 (+0.0); dst 1 <- 1 (+0.0), 0 (-0.0); dst 2 <- 2 (-1), 3 (-2); dst 3 <- 2, 4 (NaN)
    src = torch.tensor([0, 1, 1, 0, 2, 3, 2, 4])
    dst = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3])
    g = stag_amd.Graph(src, dst, 6, device=dev)
    x = torch.tensor([[-0.0], [0.0], [-1.0], [-2.0], [float("nan")], [5.0]], device=dev).expand(6, 4).contiguous()
    out, cnt = _raw_fwd(g, x, None)
    bits = out.cpu().view(torch.int32)[:, 0]
    assert bits[0] == torch.tensor(-0.0).view(torch.int32) and bits[1] == 0          # first in CSR (= edge id) order
    assert cnt[0, 0] == 2 and cnt[1, 0] == 2
    assert out[2, 0] == -1.0 and cnt[2, 0] == 1
    assert torch.isnan(out[3]).all() and (cnt[3] == 0).all()
    assert bits[4] == 0 and bits[5] == 0 and (cnt[4:] == 0).all()
    # the same through segments: a hub row whose maximum is tied across segments
    n = 200
    src = torch.arange(n)
    g = stag_amd.Graph(src, torch.zeros(n, dtype=torch.long), n, device=dev)
    xs = torch.full((n, 4), -3.0)
    xs[17], xs[150] = -0.0, 0.0
    xs[90] = 0.0
    out, cnt = _raw_fwd(g, xs.to(dev), None, seg_len=16)
    assert out.cpu().view(torch.int32)[0, 0] == torch.tensor(-0.0).view(torch.int32) and cnt[0, 0] == 3
    xs[120] = float("nan")
    out, cnt = _raw_fwd(g, xs.to(dev), None, seg_len=16)
    assert torch.isnan(out[0]).all() and (cnt[0] == 0).all()


@pytest.mark.parametrize("D", [12, 128, 300])
def test_launch_shape_independence(dev, D):
    """out and cnt are bit-identical across seg_len and with the XCD-aware unit order forced on."""
    g = random_graph(3000, 40000, seed=8, hub=5000, device=dev)
    torch.manual_seed(1)
    x = torch.randn(3000, D, device=dev)
    noise = _noise(g, D, U_, 0, True, dev)
    base = _raw_fwd(g, x, noise, seg_len=16)
    for seg_len in (64, 256):
        out, cnt = _raw_fwd(g, x, noise, seg_len=seg_len)
        assert torch.equal(out.view(torch.int32), base[0].view(torch.int32)) and torch.equal(cnt, base[1])
    for seg_len in (16, 64):
        plan = g.csr.plan(seg_len, need=True)
        g.csr._add_xcd_order(plan)
        assert plan["xcd_on"] and g.csr.xcd_order(plan, D, True)[0] is not None
        out, cnt = _raw_fwd(g, x, noise, seg_len=seg_len)
        assert torch.equal(out.view(torch.int32), base[0].view(torch.int32)) and torch.equal(cnt, base[1])


REGIMES = {
    "pos_hi": dict(seed=9, offset=3, pos_base=3 * 2**32 + 17),
    "off_hi": dict(seed=9, offset=2**32 + 7, pos_base=0),
    "off_top": dict(seed=0xFEDCBA9876543210, offset=2**63 + 11, pos_base=0),
    "chunk_top": dict(seed=9, offset=3, pos_base=0, chunk_base=(1 << 20) - 13),
}


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("front", ["ctypes", "torch_ops"])
def test_counter_regimes(dev, regime, front, monkeypatch):
    if front == "torch_ops":
        monkeypatch.setenv("STAG_TORCH_OPS", "1")
        from stag_amd import _torch_ext
        assert _torch_ext.available()
    else:
        monkeypatch.delenv("STAG_TORCH_OPS", raising=False)
    g = random_graph(400, 3000, seed=4, hub=300, device=dev)
    D = 48
    torch.manual_seed(2)
    x = torch.randn(400, D, device=dev)
    noise = _noise(g, D, N_, 1, False, dev, **REGIMES[regime])
    ref, _, _ = _restate(g, x, noise.materialize())
    assert torch.equal(_fused(g, x, noise).cpu(), ref)
    epoch = torch.tensor([5], dtype=torch.int64, device=dev)
    kw = dict(REGIMES[regime])
    kw["offset"] = (kw["offset"] - 5) % 2**64
    ne = _noise(g, D, N_, 1, False, dev, epoch=epoch, **kw)        # the same counters through the device epoch
    assert torch.equal(_fused(g, x, ne).cpu(), ref)


def _ref_backward(g, x, w, out, gout, derivs=()):
    """float64 restatement of the equal-share rule: (dx, dw, [sum_e d_i * x[src] * share for each derivative])."""
    src, dst = (t.cpu() for t in _edges(g))
    xc = x.detach().float().cpu()
    wc = w.detach().float().cpu()
    m = xc[src] * wc
    oc = out.detach().float().cpu()
    tie = (m == oc[dst])
    D = xc.shape[1]
    idx = dst.unsqueeze(1).expand(-1, D)
    cnt = torch.zeros(oc.shape, dtype=torch.float64).scatter_add(0, idx, tie.double())
    gq = torch.where(cnt > 0, gout.detach().double().cpu() / cnt.clamp(min=1), torch.zeros_like(cnt))
    share = gq[dst] * tie.double()
    dx = torch.zeros(xc.shape, dtype=torch.float64).index_add(0, src, wc.double() * share)
    dw = xc.double()[src] * share
    dps = [(d.double().cpu() * xc.double()[src] * share) for d in derivs]
    return dx, dw, dps


@pytest.mark.parametrize("kind,mode,relu", [(N_, 1, False), (N_, 0, True), (U_, 1, True), (U_, 0, False)])
@pytest.mark.parametrize("D", [12, 128, 300])
def test_backward_vi_parameters(dev, kind, mode, relu, D):
    import stag_amd
    from stag_amd import ops
    g = random_graph(500, 6000, seed=6, hub=900, device=dev)
    torch.manual_seed(5)
    x = torch.randn(500, D, device=dev, requires_grad=True)
    shape = () if mode == 0 else (D,)
    if kind == N_:
        p0 = (0.5 + 0.3 * torch.randn(shape, device=dev)).requires_grad_(True)
        p1 = (0.8 + 0.1 * torch.rand(shape, device=dev)).requires_grad_(True)
    else:
        p0 = (-0.3 + 0.1 * torch.rand(shape, device=dev)).requires_grad_(True)
        p1 = (1.2 + 0.1 * torch.rand(shape, device=dev)).requires_grad_(True)
    noise = stag_amd.EdgeNoise(g, D, kind, p0, p1, relu=relu, seed=21, offset=4, differentiable=True)
    out = ops.aggregate_max(g, x, noise, seg_len=32)
    gout = torch.randn_like(out)
    out.backward(gout)
    with torch.no_grad():
        w = ops.materialize_noise(g, noise)
        std = stag_amd.EdgeNoise(g, D, kind, 0.0, 1.0, seed=21, offset=4)
        t = ops.materialize_noise(g, std)                 # z (Normal) | u (Uniform) of the same counters
    mask = (w > 0).double() if relu else torch.ones_like(w, dtype=torch.float64)
    d0 = (torch.ones_like(t) if kind == N_ else 1 - t).double() * mask
    d1 = t.double() * mask
    ref, rcnt, _ = _restate(g, x, w)
    assert torch.equal(out.detach().cpu(), ref)
    dx, _, (g0, g1) = _ref_backward(g, x, w, out, gout, (d0, d1))
    assert_close(x.grad, dx.float().numpy(), what="dx")
    want0 = g0.sum() if mode == 0 else g0.sum(0)
    want1 = g1.sum() if mode == 0 else g1.sum(0)
    assert_close(p0.grad / max(1.0, float(want0.abs().max())), (want0 / max(1.0, float(want0.abs().max()))).float().numpy(),
                 what="dp0")
    assert_close(p1.grad / max(1.0, float(want1.abs().max())), (want1 / max(1.0, float(want1.abs().max()))).float().numpy(),
                 what="dp1")
    # run to run: bit-identical
    grads = (x.grad.clone(), p0.grad.clone(), p1.grad.clone())
    x.grad = p0.grad = p1.grad = None
    ops.aggregate_max(g, x, noise, seg_len=32).backward(gout)
    for a, b in zip(grads, (x.grad, p0.grad, p1.grad)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("D", [3, 8, 32, 64, 256])               # 8, 32: 2 and 8 lanes per row
def test_backward_explicit_weights(dev, D):
    from stag_amd import ops
    g = random_graph(400, 5000, seed=12, hub=600, device=dev)
    torch.manual_seed(D)
    x = torch.randn(400, D, device=dev, requires_grad=True)
    w = (torch.rand(g.number_of_edges(), D, device=dev) + 0.5).requires_grad_(True)
    out = ops.aggregate_max(g, x, w, seg_len=16)
    gout = torch.randn_like(out)
    out.backward(gout)
    dx, dw, _ = _ref_backward(g, x, w, out, gout)
    assert_close(x.grad, dx.float().numpy(), what="dx")
    assert_close(w.grad, dw.float().numpy(), what="dw")
    gx, gw = x.grad.clone(), w.grad.clone()
    x.grad = w.grad = None
    ops.aggregate_max(g, x, w, seg_len=16).backward(gout)
    assert torch.equal(gx, x.grad) and torch.equal(gw, w.grad)


def test_routes_agree_for_graphsage_pool(dev, monkeypatch):
    """ops.FUSED_MAX: the fused and the composed route give the same GraphSAGE('pool') forward and gradients, and the
    same StagLayer(GraphSAGE pool, vi=True) training step (no maximum is +-0 here: positive weights and features)."""
    import stag_amd
    from stag_amd import ops
    g = random_graph(300, 3000, seed=3, hub=400, device=dev)
    torch.manual_seed(0)
    x0 = torch.rand(300, 24, device=dev) + 0.1
    w = torch.rand(g.number_of_edges(), 24, device=dev) + 0.5
    layer = stag_amd.zoo.GraphSAGE(24, 9, aggregator_type="pool").to(dev)
    with torch.no_grad():                      # fc_pool keeps every pre-activation positive: no zero maxima
        layer.fc_pool.weight.abs_()
        layer.fc_pool.bias.abs_().add_(0.1)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "FUSED_MAX", fused)
        x = x0.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        out = layer(g, x, edge_weight=ww)
        out.backward(torch.ones_like(out))
        res[fused] = (out.detach(), x.grad, ww.grad, [p.grad.clone() for p in layer.parameters()])
    a, b = res[True], res[False]
    assert_close(a[0], b[0].cpu().numpy(), what="out")
    assert_close(a[1], b[1].cpu().numpy(), what="dx")
    assert_close(a[2], b[2].cpu().numpy(), what="dw")
    for p, q in zip(a[3], b[3]):
        sc = max(1.0, float(q.abs().max()))
        assert_close(p / sc, (q / sc).cpu().numpy(), what="dparam")
    # a StagLayer step with vi=True (reparameterised Normal; loc / scale receive gradients)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "FUSED_MAX", fused)
        torch.manual_seed(4)
        base = stag_amd.zoo.GraphSAGE(24, 9, aggregator_type="pool").to(dev)
        with torch.no_grad():
            base.fc_pool.weight.abs_()
            base.fc_pool.bias.abs_().add_(0.1)
        sl = stag_amd.layers.StagLayer(base, q_a=torch.distributions.Normal(3.0, 0.2), vi=True).to(dev)
        opt = torch.optim.SGD(sl.parameters(), lr=0.01)
        stag_amd.manual_seed(77)
        out = sl(g, x0)
        loss = (out ** 2).mean()
        loss.backward()
        grads = {k: p.grad.clone() for k, p in sl.named_parameters() if p.grad is not None}
        opt.step()
        res[fused] = (out.detach(), grads)
    assert_close(res[True][0], res[False][0].cpu().numpy(), what="stag out")
    assert set(res[True][1]) == set(res[False][1]) and any("q_a" in k for k in res[True][1])
    for k, v in res[True][1].items():
        q = res[False][1][k]
        sc = max(1.0, float(q.abs().max()))
        assert_close(v / sc, (q / sc).cpu().numpy(), what=f"stag d {k}")


def test_dispatcher_ops_bit_identical_to_ctypes(dev, monkeypatch):
    from stag_amd import ops
    g = random_graph(300, 4000, seed=13, hub=500, device=dev)
    torch.manual_seed(9)
    D = 40
    x = torch.randn(300, D, device=dev)
    res = {}
    for front in ("ctypes", "torch_ops"):
        if front == "torch_ops":
            monkeypatch.setenv("STAG_TORCH_OPS", "1")
        else:
            monkeypatch.delenv("STAG_TORCH_OPS", raising=False)
        noise = _noise(g, D, N_, 1, True, dev)
        xr = x.clone().requires_grad_(True)
        out = ops.aggregate_max(g, xr, noise, seg_len=32)
        out.backward(torch.ones_like(out))
        wt = (torch.rand(g.number_of_edges(), D, device=dev, generator=torch.Generator(dev).manual_seed(1)) + 0.5)
        wt.requires_grad_(True)
        o2 = ops.aggregate_max(g, xr, wt, seg_len=32)
        o2.backward(torch.ones_like(o2))
        res[front] = (out.detach(), xr.grad.clone(), o2.detach(), wt.grad.clone())
    for a, b in zip(res["ctypes"], res["torch_ops"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_update_all_copy_e_and_broadcast(dev):
    """update_all(copy_e, max) and u_mul_e with [E, H, 1] edge data against [N, H, F] features (DGL broadcasting)."""
    import stag_amd
    import stag_amd.function as fn
    g = random_graph(200, 2000, seed=14, hub=300, device=dev)
    src, dst = (t.cpu() for t in _edges(g))
    E, n = g.number_of_edges(), 200
    torch.manual_seed(3)
    we = torch.randn(E, 3, 5, device=dev)
    gl = g.local_var()
    gl.edata["w"] = we
    gl.update_all(fn.copy_e("w", "m"), fn.max("m", "o"))
    ref = torch.zeros(n, 15).scatter_reduce(0, dst.unsqueeze(1).expand(-1, 15), we.cpu().reshape(E, 15), "amax",
                                            include_self=False)
    assert gl.dstdata["o"].shape == (n, 3, 5) and torch.equal(gl.dstdata["o"].reshape(n, 15).cpu(), ref)
    h = torch.randn(n, 3, 4, device=dev)
    a = torch.rand(E, 3, 1, device=dev) + 0.1
    gl = g.local_var()
    gl.srcdata["h"], gl.edata["a"] = h, a
    gl.update_all(fn.u_mul_e("h", "a", "m"), fn.max("m", "o"))
    m = (h.cpu()[src] * a.cpu()).reshape(E, 12)
    ref = torch.zeros(n, 12).scatter_reduce(0, dst.unsqueeze(1).expand(-1, 12), m, "amax", include_self=False)
    assert gl.dstdata["o"].shape == (n, 3, 4) and torch.equal(gl.dstdata["o"].reshape(n, 12).cpu(), ref)


def test_memory_at_arxiv_shape(dev):
    """A forward with x.requires_grad at the arxiv shape (D = 128, Normal) holds O(N * D): out, the tie counts and the
    plan workspace — the composed route needs at least three [E, D] tensors."""
    import stag_amd
    from stag_amd import ops, synthetic
    src, dst = synthetic.arxiv_like()
    N = int(max(src.max(), dst.max())) + 1
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), N, device=dev)
    D = 128
    x = torch.randn(N, D, device=dev, requires_grad=True)
    noise = stag_amd.EdgeNoise(g, D, N_, 1.0, 0.5, seed=3, offset=1)
    with torch.no_grad():
        ops.aggregate_max(g, x, noise)               # plans and CSR views built outside the measurement
    g.csr_t
    torch.cuda.synchronize()
    plan = g.csr.plan(64)
    ws = plan["n_seg"] * 2 * D * 4 if plan is not None else 0
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = ops.aggregate_max(g, x, noise)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    E = g.number_of_edges()
    assert peak < 3 * N * D * 4 + ws + (1 << 20), (peak, N, E)
    assert 3 * E * D * 4 > 3 * N * D * 4 + ws
    out.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
