"""stag_gat_fwd_half — the cooperative GAT forward on fp16 / bf16 ft rows gathered as they are.  Widening is exact and
the kernel keeps the fp32 kernel's arithmetic and its order, so the contract is bit-identity with stag_gat_fwd on
ft.float(), in out and in stats; on top of that: the oracle on the widened rows at the bar the fp32 kernel is held to,
degenerate graphs, addressing past 2^24 rows, autograd, the routing of ops.gat_aggregate and zoo.GAT under autocast."""
import numpy as np
import pytest
import torch

from util import TOL, assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [(8, 32), (3, 4), (1, 64), (2, 40), (8, 64), (16, 64)]
KINDS = ("none", "explicit", "normal", "normal_head_relu", "bernoulli_norm", "normal_drop")

GRAPHS = {
    "hub": lambda dev: random_graph(300, 2500, seed=5, hub=700, device=dev),     # zero-in-degree rows, many segments
    "one_edge": lambda dev: random_graph(4, 1, seed=2, device=dev),
    "no_edges": lambda dev: random_graph(5, 0, seed=2, device=dev),
}


def _inputs(n, H, F, dtype, dev, seed=0):
    """el, er fp32 and a half ft with the values a widening could get wrong planted in it: -0.0, the dtype's largest
    finite value (+ in one channel, - in another: no inf - inf in a sum), and for fp16 subnormals."""
    gen = torch.Generator().manual_seed(100 * H + F + seed)
    el = torch.randn(n, H, generator=gen).to(dev)
    er = torch.randn(n, H, generator=gen).to(dev)
    ft = torch.randn(n, H, F, generator=gen).to(dtype)
    big = torch.finfo(dtype).max
    flat = ft.view(n, H * F)
    rows = torch.arange(n)
    flat[rows % 5 == 0, 0] = -0.0
    flat[rows % 7 == 1, 1] = big
    flat[rows % 7 == 2, 2] = -big
    if dtype == torch.float16:
        flat[rows % 3 == 0, 3] = 2.0 ** -24            # the smallest subnormal
        flat[rows % 3 == 1, 3] = -(2.0 ** -15 - 2.0 ** -24)
    return el, er, ft.to(dev)


def _weight(g, H, kind, dev):
    """(weight argument of ops.gat_aggregate, attn_drop) of a kind."""
    import stag_amd
    from stag_amd import _lib
    E = g.number_of_edges()
    if kind == "none":
        return None, None
    if kind == "explicit":
        return (torch.rand(E, H, generator=torch.Generator().manual_seed(E + H)) + 0.5).to(dev), None
    if kind == "normal":
        return stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=17, offset=3), None
    if kind == "normal_head_relu":
        p0 = torch.linspace(0.6, 1.2, H).to(dev)
        p1 = torch.linspace(0.3, 0.9, H).to(dev)
        return stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, p0, p1, relu=True, seed=19, offset=5), None
    if kind == "bernoulli_norm":
        return stag_amd.EdgeNoise(g, H, _lib.NOISE_BERNOULLI, 0.7, None, in_norm=True, seed=23, offset=7), None
    if kind == "normal_drop":
        return stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=29, offset=11), (0.6, 0xD00D, 4)
    raise KeyError(kind)


def _raw_pair(g, el, er, fth, weight, attn_drop, seg_len, xcd=False):
    """(out, stats) of stag_gat_fwd on fth.float() and of stag_gat_fwd_half on fth: both entry points called directly,
    with the same plan struct contents, spec, in-norm factors and dropout."""
    import stag_amd
    from stag_amd import _lib, ops
    csrv, dev = g.csr, el.device
    H, F = fth.shape[1], fth.shape[2]
    noise = weight if isinstance(weight, stag_amd.EdgeNoise) else None
    if noise is not None:
        spec = noise.spec()
    elif weight is not None:
        spec = ops._targs_or_c(ops._explicit_spec(weight))
    else:
        spec = ops._targs_or_c(ops._none_spec())
    nscale = ops._gat_norm_scale(csrv, noise, H, seg_len, dev) if spec.in_norm else None
    drop = ops._gat_drop_struct(attn_drop)
    plan_t = csrv.plan(seg_len, need=True)
    if xcd:
        csrv._add_xcd_order(plan_t)
    res = []
    for half in (False, True):
        out = torch.full((csrv.n_dst, H, F), float("nan"), device=dev)
        stats = torch.full((csrv.n_dst, 2 * H), float("nan"), device=dev)
        if half:
            plan_c, _keep = ops._gat_fwd_half_raw(csrv, plan_t, el, er, fth, H, F, 0.2, spec, nscale, drop, out, stats,
                                                  seg_len, dev)
            if xcd:
                assert plan_c.xcd_order, "the launch was handed the XCD-aware batches"
        else:
            ops._gat_fwd_into(csrv, plan_t, el, er, fth.float(), H, F, 0.2, spec, nscale, drop, out, stats, dev)
        res += [out, stats]
    return res


def _counted(monkeypatch):
    from stag_amd import ops
    calls = []
    real = ops._gat_fwd_half_raw

    def wrapper(*a, **kw):
        calls.append(a[4].dtype)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "_gat_fwd_half_raw", wrapper)
    return calls


# ---- 1. bit-identity with the fp32 entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("H,F", SHAPES)
def test_bit_identical_to_the_fp32_entry(dev, monkeypatch, H, F, dname):
    """out and stats of stag_gat_fwd_half equal stag_gat_fwd on ft.float() for every kind, at seg_len 64 and 16 (the
    700-edge row: 11 and 44 segments), and ops.gat_aggregate on the half ft takes the new entry (counted) and returns
    what it returns on ft.float()."""
    from stag_amd import ops
    g = GRAPHS["hub"](dev)
    n = g.number_of_nodes()
    el, er, fth = _inputs(n, H, F, DTYPES[dname], dev)
    calls = _counted(monkeypatch)
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    for kind in KINDS:
        weight, drop = _weight(g, H, kind, dev)
        for seg_len in (64, 16):
            o32, s32, oh, sh = _raw_pair(g, el, er, fth, weight, drop, seg_len)
            assert not torch.isnan(oh).any() and not torch.isnan(sh).any(), (kind, seg_len)
            assert torch.equal(oh, o32), (kind, seg_len, "out")
            assert torch.equal(sh, s32), (kind, seg_len, "stats")
            with torch.no_grad():
                n0 = len(calls)
                got = ops.gat_aggregate(g, el, er, fth, 0.2, weight, seg_len=seg_len, attn_drop=drop)
                assert len(calls) == n0 + 1 and calls[-1] == DTYPES[dname]
                ref = ops.gat_aggregate(g, el, er, fth.float(), 0.2, weight, seg_len=seg_len, attn_drop=drop)
                assert len(calls) == n0 + 1
            assert got.dtype == torch.float32 and torch.equal(got, ref) and torch.equal(got, oh), (kind, seg_len)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("H,F", [(8, 32), (8, 64)])
def test_bit_identical_on_xcd_local_batches(dev, H, F, dname):
    """The plan's XCD-aware batches handed over (a non-NULL xcd_order: at (8, 64), two chunks per lane, the launch
    takes the instantiation with the rows in flight of XCD-local gathers)."""
    g = GRAPHS["hub"](dev)
    el, er, fth = _inputs(g.number_of_nodes(), H, F, DTYPES[dname], dev, seed=1)
    for kind in ("none", "normal", "normal_drop"):
        weight, drop = _weight(g, H, kind, dev)
        o32, s32, oh, sh = _raw_pair(g, el, er, fth, weight, drop, 64, xcd=True)
        assert torch.equal(oh, o32) and torch.equal(sh, s32), kind


# ---- 2. against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("H,F", [(8, 32), (2, 40)])
def test_against_the_oracle_on_widened_rows(dev, oracle, monkeypatch, H, F, dname):
    from stag_amd import ops
    g = GRAPHS["hub"](dev)
    n, E = g.number_of_nodes(), g.number_of_edges()
    og = oracle_graph(oracle, g)
    gen = torch.Generator().manual_seed(H * 31 + F)
    el, er = torch.randn(n, H, generator=gen), torch.randn(n, H, generator=gen)
    fth = torch.randn(n, H, F, generator=gen).to(DTYPES[dname])
    calls = _counted(monkeypatch)
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    specs = {
        "none": oracle.make_spec("none"),
        "normal": oracle.make_spec("normal", 1.0, 0.5, Dn=H, n_edges=E, seed=17, offset=3),
        "bernoulli_norm": oracle.make_spec("bernoulli", 0.7, None, Dn=H, n_edges=E, seed=23, offset=7, in_norm=True),
    }
    for kind, spec in specs.items():
        weight, _ = _weight(g, H, kind, dev)
        out, attn = ops.gat_aggregate(g, el.to(dev), er.to(dev), fth.to(dev), 0.2, weight, want_attn=True)
        with hw_normals(oracle, dev):
            ref, ref_attn = oracle.gat_fwd(og, el.numpy(), er.numpy(), fth.float().numpy(), 0.2, spec, want_attn=True)
        assert_close(out, ref, what=f"gat half out {kind} {dname} H={H} F={F}")
        assert_close(attn, ref_attn, what=f"gat half attn {kind} {dname}")
    assert calls == [DTYPES[dname]] * 3


# ---- 3. degenerate graphs, run to run ------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_degenerate_graphs_and_run_to_run(dev, gname, dname):
    g = GRAPHS[gname](dev)
    n, H, F = g.number_of_nodes(), 8, 32
    el, er, fth = _inputs(n, H, F, DTYPES[dname], dev, seed=2)
    for kind in ("none", "normal_drop"):
        weight, drop = _weight(g, H, kind, dev)
        o32, s32, oh, sh = _raw_pair(g, el, er, fth, weight, drop, 64)
        assert torch.equal(oh, o32) and torch.equal(sh, s32), kind
        deg = g.csr.degrees
        assert (deg == 0).any()                             # every graph here has rows without in-edges
        assert (oh[deg == 0] == 0).all() and torch.equal(oh[deg == 0], o32[deg == 0])
        _, _, oh2, sh2 = _raw_pair(g, el, er, fth, weight, drop, 64)
        assert torch.equal(oh2, oh) and torch.equal(sh2, sh), "two launches, the same bits"


# ---- 4. addressing past 2^24 rows ----------------------------------------------------------------------------------
def test_rows_past_the_24_bit_row_index(dev):
    """n_src >= 2^24: the 24-bit multiply behind the buffer descriptor does not reach every row, and the kernel takes
    64-bit addresses.  Three destination rows gather five rows around 2^24 of an otherwise zero [2^24 + 5, 1, 4] table;
    the result is the rows' softmax-weighted sum, computed on the host in float64."""
    from stag_amd import ops
    from stag_amd.graph import CsrView
    n_src, H, F = (1 << 24) + 5, 1, 4
    rows = [0, (1 << 24) - 1, (1 << 24) + 1, (1 << 24) + 4, 5]
    indptr = [0, 2, 2, 5]
    csrv = CsrView(3, n_src, torch.tensor(indptr, dtype=torch.int32, device=dev),
                   torch.tensor(rows, dtype=torch.int32, device=dev))
    gen = torch.Generator().manual_seed(4)
    el5, er3 = torch.randn(5, H, generator=gen), torch.randn(3, H, generator=gen)
    el = torch.zeros(n_src, H, device=dev)
    el[torch.tensor(rows, device=dev)] = el5.to(dev)
    er = er3.to(dev)
    spec = ops._targs_or_c(ops._none_spec())
    plan_t = csrv.plan(64, need=True)
    for dname, dtype in DTYPES.items():
        vals = torch.randn(5, H, F, generator=gen).to(dtype)
        ft = torch.zeros(n_src, H, F, device=dev, dtype=dtype)
        ft[torch.tensor(rows, device=dev)] = vals.to(dev)
        out = torch.full((3, H, F), float("nan"), device=dev)
        stats = torch.full((3, 2 * H), float("nan"), device=dev)
        ops._gat_fwd_half_raw(csrv, plan_t, el, er, ft, H, F, 0.2, spec, None, None, out, stats, 64, dev)
        ref = np.zeros((3, H, F))
        for v in range(3):
            p = list(range(indptr[v], indptr[v + 1]))
            if not p:
                continue
            s = el5[p].double().numpy() + er3[v].double().numpy()                   # [deg, H]
            e = np.where(s > 0, s, 0.2 * s)
            a = np.exp(e - e.max(0))
            a /= a.sum(0)
            ref[v] = (a[:, :, None] * vals[p].double().numpy()).sum(0)
        assert_close(out, ref, what=f"wide addressing {dname}")
        del ft


# ---- 5. autograd -----------------------------------------------------------------------------------------------------
def _vi_noise(g, H, dev):
    import stag_amd
    from stag_amd import _lib
    p0 = torch.linspace(0.8, 1.2, H).to(dev).requires_grad_(True)
    p1 = torch.linspace(0.3, 0.6, H).to(dev).requires_grad_(True)
    return stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, p0, p1, seed=31, offset=13, differentiable=True), (p0, p1)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("kind", ["none", "normal", "normal_drop", "vi"])
def test_autograd_is_the_cast_route_s(dev, monkeypatch, kind, dname):
    """Gradients w.r.t. el, er, the half ft (and live per-head parameters) equal the cast route's bit for bit — its d ft
    cast to the half dtype, which autograd does for both routes — and what is kept for the backward is the half ft.
    (`out`, fp32 and of ft's shape on a square graph, is saved by both routes: it is the result itself, not a copy of
    ft, and is excluded from the dtype check by its storage.)"""
    from stag_amd import ops
    g = GRAPHS["hub"](dev)
    n, H, F = g.number_of_nodes(), 8, 32
    el0, er0, fth0 = _inputs(n, H, F, DTYPES[dname], dev, seed=3)
    fth0 = (fth0.float().clamp(-4, 4)).to(DTYPES[dname])       # finite gradients: no largest-finite values here
    G = torch.randn(n, H, F, device=dev)
    calls = _counted(monkeypatch)
    grads = {}
    for route in (True, False):
        monkeypatch.setattr(ops, "GAT_HALF_ROWS", route)
        el, er, ft = (t.clone().requires_grad_(True) for t in (el0, er0, fth0))
        if kind == "vi":
            weight, params = _vi_noise(g, H, dev)
            drop = None
        else:
            (weight, drop), params = _weight(g, H, kind, dev), ()
        saved = []
        n0 = len(calls)
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
            out = ops.gat_aggregate(g, el, er, ft, 0.2, weight, attn_drop=drop)
        assert len(calls) == n0 + (1 if route else 0)
        if route:
            same_shape = [t for t in saved if t.shape == ft.shape and t.untyped_storage().data_ptr() != out.untyped_storage().data_ptr()]
            assert same_shape and all(t.dtype == DTYPES[dname] for t in same_shape), [(t.shape, t.dtype) for t in saved]
            assert any(t.data_ptr() == ft.data_ptr() for t in same_shape), "the half ft itself is what is saved"
        out.backward(G)
        assert ft.grad.dtype == DTYPES[dname]
        grads[route] = [out.detach(), el.grad, er.grad, ft.grad] + [p.grad for p in params]
    for a, b in zip(grads[True], grads[False]):
        assert a is not None and torch.isfinite(a).all() and torch.equal(a, b)


# ---- 6. routing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
def test_every_fallback_is_the_cast_route(dev, monkeypatch, dname):
    import stag_amd
    from stag_amd import _lib, ops
    g = GRAPHS["hub"](dev)
    n = g.number_of_nodes()
    dt = DTYPES[dname]
    calls = _counted(monkeypatch)
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    why = ops.gat_half_rows_why_not

    def inputs(H, F):
        el, er, ft = _inputs(n, H, F, dt, dev, seed=4)
        return el, er, ft

    with torch.no_grad():
        el, er, ft = inputs(4, 6)                                            # F % 4 != 0
        assert why(ft, 64, g) == "shape"
        assert torch.equal(ops.gat_aggregate(g, el, er, ft), ops.gat_aggregate(g, el, er, ft.float()))
        el, er, ft = inputs(32, 4)                                           # H > 16
        assert why(ft, 64, g) == "shape"
        assert torch.equal(ops.gat_aggregate(g, el, er, ft), ops.gat_aggregate(g, el, er, ft.float()))
        el, er, ft = inputs(8, 32)
        buf = torch.zeros(n * 8 * 32 + 2, dtype=dt, device=dev)             # a view 4 bytes into an allocation
        ftm = buf[2:].view(n, 8, 32)
        ftm.copy_(ft)
        assert ftm.is_contiguous() and ftm.data_ptr() % 8 == 4 and why(ftm, 64, g) == "alignment"
        ref = ops.gat_aggregate(g, el, er, ft.float())
        assert torch.equal(ops.gat_aggregate(g, el, er, ftm), ref)
        nz = stag_amd.EdgeNoise(g, 8, _lib.NOISE_NORMAL, 1.0, 0.5, seed=3, offset=1)          # a Monte-Carlo batch
        nz.n_samples, nz.offset_stride = 3, 1
        assert why(ft, 64, g, nz) == "monte-carlo"
        mc = ops.gat_aggregate(g, el, er, ft, 0.2, nz)
        assert mc.shape == (3, n, 8, 32) and torch.equal(mc, ops.gat_aggregate(g, el, er, ft.float(), 0.2, nz))
        assert not calls
        assert why(ft, 64, g) is None
        assert torch.equal(ops.gat_aggregate(g, el, er, ft), ref)
        assert len(calls) == 1
        monkeypatch.setattr(ops, "GAT_HALF_ROWS", False)                    # the switch
        assert why(ft, 64, g) == "switch"
        assert torch.equal(ops.gat_aggregate(g, el, er, ft), ref)
        assert len(calls) == 1
        monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
        assert why(ft.cpu(), 64, g) == "device"                              # a CPU tensor: no CPU path, as before
        with pytest.raises(_lib.StagHipError, match="HIP device only"):
            ops.gat_aggregate(g, el, er, ft.cpu())
        assert len(calls) == 1


# ---- 7. the layer under autocast -------------------------------------------------------------------------------------
def _layer_step(layer, g, x0, seed, autocast=True):
    import stag_amd
    for p in layer.parameters():
        p.grad = None
    stag_amd.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = layer(g, x0)
    out.square().mean().backward()
    return out.detach(), [p.grad.clone() for p in layer.parameters() if p.requires_grad]


@pytest.mark.parametrize("F_out", [8, 7])
def test_gat_layer_under_autocast_gathers_bf16_rows(dev, monkeypatch, F_out):
    """StagLayer(zoo.GAT) under bf16 autocast with ops.GAT_HALF_FT: ft comes out of a bf16 GEMM and is gathered as it is
    (one call of the new entry with bf16; a head width of 7 runs padded to 8); toggling GAT_HALF_ROWS changes no bit; a
    training step reaches every parameter; with GAT_HALF_FT off the layer computes what it computes without this
    change's code path."""
    import stag_amd
    from stag_amd import ops
    g = GRAPHS["hub"](dev)
    n = g.number_of_nodes()
    torch.manual_seed(0)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GAT(24, F_out, num_heads=4, attn_drop=0.6),
                                      q_a=torch.distributions.Normal(1.0, 0.3)).to(dev)
    layer.train()
    x0 = torch.randn(n, 24, device=dev)
    calls = _counted(monkeypatch)
    monkeypatch.setattr(ops, "GAT_HALF_FT", True)
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    out_on, grads_on = _layer_step(layer, g, x0, 77)
    assert calls == [torch.bfloat16]
    assert out_on.dtype == torch.float32 and out_on.shape == (n, 4 * F_out) and torch.isfinite(out_on).all()
    assert len(grads_on) >= 4
    for gr in grads_on:
        assert torch.isfinite(gr).all() and float(gr.abs().max()) > 0
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", False)           # the same bf16 ft through the cast route
    out_cast, grads_cast = _layer_step(layer, g, x0, 77)
    assert calls == [torch.bfloat16]
    assert torch.equal(out_cast, out_on)
    for a, b in zip(grads_on, grads_cast):
        assert torch.equal(a, b)
    # GAT_HALF_FT off: never the new entry, and the output of the layer as it is without this change's code path
    monkeypatch.setattr(ops, "GAT_HALF_FT", False)
    out_parent, _ = _layer_step(layer, g, x0, 77)              # (GAT_HALF_ROWS is off too)
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    out_off, _ = _layer_step(layer, g, x0, 77)
    assert calls == [torch.bfloat16]
    assert torch.equal(out_off, out_parent)
    # and the half-GEMM layer agrees with the fp32 one to bf16 precision (not bit for bit).  el / er are fp32 on both
    # sides, so the attention and the dropout mask agree and the difference is the rounding of ft alone: a bf16 GEMM of
    # K = 24 terms is off by about 2^-8 of |ft|, an output is a kept-and-rescaled (1 / 0.4) convex combination of ft rows:
    # 2.5 x 2^-8 ~ 1 % of the largest output; 5 % is the bar.
    assert float((out_on - out_parent).abs().max()) <= 0.05 * (1.0 + float(out_parent.abs().max()))
