"""stag_agg_fwd_half — fp16 / bf16 feature rows gathered as they are — against the CPU oracle on the widened rows
(widening is exact, so oracle.agg_fwd on x.float() with the same spec is the reference, at the bar the fp32 kernel is
held to: util.TOL), its draws bit for bit against EdgeNoise.materialize(), and the routing of ops.aggregate."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import TOL, assert_close, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("none", "normal", "uniform", "bernoulli")

GRAPHS = {
    "hub": lambda dev: random_graph(300, 2500, seed=5, hub=700, device=dev),     # zero-in-degree rows, many segments
    "one_edge": lambda dev: random_graph(4, 1, seed=2, device=dev),
    "no_edges": lambda dev: random_graph(5, 0, seed=2, device=dev),
}


def _params(kind, mode, D, dev, seed=0):
    """(p0, p1) of a sampled kind: python floats (mode 0) or [D] device rows (mode 1)."""
    gen = torch.Generator().manual_seed(1234 + 7 * D + seed + {"normal": 0, "uniform": 1, "bernoulli": 2}[kind])

    def par(lo, hi):
        t = lo + (hi - lo) * torch.rand((D,) if mode else (), generator=gen)
        return t.to(dev) if mode else float(t)
    if kind == "normal":
        return par(-0.5, 1.0), par(0.3, 1.2)
    if kind == "uniform":
        return par(-0.5, 0.2), par(0.5, 1.5)
    return par(0.2, 0.8), None


def _noise(g, D, kind, p0, p1, **kw):
    import stag_amd
    from stag_amd import _lib
    k = {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM, "bernoulli": _lib.NOISE_BERNOULLI}[kind]
    return stag_amd.EdgeNoise(g, D, k, p0, p1, **kw)


def _np(p):
    return p.detach().cpu().numpy() if torch.is_tensor(p) else p


def _ospec(O, g, D, kind, p0, p1, **kw):
    if kind == "none":
        return O.make_spec("none")
    return O.make_spec(kind, _np(p0), _np(p1), Dn=D, n_edges=g.number_of_edges(), **kw)


def _spec_of(noise):
    from stag_amd import ops
    return ops._targs_or_c(ops._noise_spec(noise) if noise is not None else ops._none_spec())


def _raw(csrv, x, noise, reduce="sum", ss=None, ds=None, seg_len=64):
    from stag_amd import ops
    return ops._agg_half_raw(csrv, x, x.shape[1], _spec_of(noise), ops._REDUCE[reduce], ss, ds, seg_len)


def _raw_xcd(csrv, x, noise, seg_len):
    """The same launch with the plan's XCD-aware order handed over (stag_plan.xcd_order: the entry point ignores it)."""
    from stag_amd import _lib, ops
    D, dev = x.shape[1], x.device
    plan_t = csrv.plan(seg_len, need=True)
    csrv._add_xcd_order(plan_t)
    nbytes = _lib.lib().stag_plan_workspace_bytes(plan_t["n_seg"], D, 0)
    plan_c, _keep = ops._plan_struct(csrv, seg_len, (D + 255) // 256, nbytes, dev, plan_t, width=D)
    assert plan_c.xcd_order, "the plan carries an XCD-aware order"
    out = torch.empty((csrv.n_dst, D), dtype=torch.float32, device=dev)
    spec, cs = _spec_of(noise), csrv.struct()
    rc = _lib.lib().stag_agg_fwd_half(C.byref(cs), C.byref(plan_c), x.data_ptr(), ops._HALF_DTYPES[x.dtype], x.stride(0), D,
                                      C.byref(spec), 0, None, None, out.data_ptr(), D, _lib.stream_of(dev))
    assert rc == 0
    return out


# ---- 1. parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 16, 24, 64, 128, 136, 256, 264, 512, 520, 1432])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_parity_with_oracle_on_widened_rows(dev, oracle, gname, dname, D):
    """kind x parameter mode x relu x reduce x with / without the two scales, at every width class: one lane, partial
    teams, a team that is not full, past a 256 and a 512 boundary, a row of several channel tiles."""
    g = GRAPHS[gname](dev)
    n = g.number_of_nodes()
    og = oracle_graph(oracle, g)
    x = torch.randn(n, D, device=dev).to(DTYPES[dname])
    xf = x.float().cpu().numpy()
    rng = np.random.default_rng(D)
    ss = rng.uniform(0.5, 1.5, n).astype(np.float32)
    ds = rng.uniform(0.5, 1.5, n).astype(np.float32)
    ssd, dsd = torch.from_numpy(ss).to(dev), torch.from_numpy(ds).to(dev)
    cases = [("none", 0, False)] + [(k, m, r) for k in KINDS[1:] for m in (0, 1) for r in (False, True)]
    with hw_normals(oracle, dev):
        for kind, mode, relu in cases:
            p0, p1 = (None, None) if kind == "none" else _params(kind, mode, D, dev)
            kw = dict(relu=relu, seed=11, offset=2)
            noise = None if kind == "none" else _noise(g, D, kind, p0, p1, **kw)
            spec = _ospec(oracle, g, D, kind, p0, p1, **kw)
            for reduce in ("sum", "mean"):
                red = oracle.REDUCE_MEAN if reduce == "mean" else oracle.REDUCE_SUM
                for scaled in (False, True):
                    got = _raw(g.csr, x, noise, reduce, ssd if scaled else None, dsd if scaled else None)
                    ref = oracle.agg_fwd(og, xf, spec, reduce=red, src_scale=ss if scaled else None,
                                         dst_scale=ds if scaled else None)
                    assert got.dtype == torch.float32 and got.shape == (n, D)
                    assert_close(got, ref, what=f"{gname} {dname} D={D} {kind}/{mode} relu={relu} {reduce} scaled={scaled}")


# ---- 2. the draws, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 24, 264])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS[1:])
def test_draws_are_the_fp32_launch_s_bit_for_bit(dev, kind, mode, D):
    """Every destination has exactly one in-edge and x = 1: out[dst_e] IS w[e], the weight stag_noise_materialize
    writes for the same spec."""
    import stag_amd
    n = 64
    src = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    dst = torch.arange(n)
    g = stag_amd.Graph(src, dst, n, device=dev)
    p0, p1 = _params(kind, mode, D, dev)
    noise = _noise(g, D, kind, p0, p1, seed=0xABCDEF12345, offset=2**33 + 5)
    wm = noise.materialize()                                    # [E, D] by edge id; edge e ends at dst[e] = e
    for dt in DTYPES.values():
        out = _raw(g.csr, torch.ones(n, D, device=dev, dtype=dt), noise)
        assert torch.equal(out.view(torch.int32), wm.view(torch.int32))
        assert torch.equal(_raw(g.csr, torch.ones(n, D, device=dev, dtype=dt), noise, seg_len=0).view(torch.int32),
                           wm.view(torch.int32))


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS[1:])
def test_chunk_base_column_halves_equal_one_launch(dev, kind, dname):
    """Two launches on the column halves of a D = 128 tensor (ldx = 128; the second with chunk_base = 16) are the one
    launch on the whole width: the same draws, and a lane's sums do not depend on the launch's width."""
    g = GRAPHS["hub"](dev)
    n, D = g.number_of_nodes(), 128
    x = torch.randn(n, D, device=dev).to(DTYPES[dname])
    p0, p1 = _params(kind, 1, D, dev)
    kw = dict(relu=True, seed=5, offset=9)
    whole = _raw(g.csr, x, _noise(g, D, kind, p0, p1, **kw))
    halves = []
    for h in (0, 1):
        sl = slice(64 * h, 64 * h + 64)
        nz = _noise(g, 64, kind, p0[sl].contiguous(), None if p1 is None else p1[sl].contiguous(), chunk_base=16 * h, **kw)
        xs = x[:, sl]
        assert xs.stride(0) == 128
        halves.append(_raw(g.csr, xs, nz))
    assert torch.equal(torch.cat(halves, 1).view(torch.int32), whole.view(torch.int32))


# ---- 3. the transposed walk ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("kind,mode,relu", [("normal", 1, True), ("uniform", 0, False), ("bernoulli", 1, False)])
@pytest.mark.parametrize("seg_len", [4, 64])
def test_transposed_walk_redraws_forward_positions(dev, oracle, dname, kind, mode, relu, seg_len):
    g = GRAPHS["hub"](dev)
    n, D = g.number_of_nodes(), 72
    assert g.csr_t.nidx is not None
    G = torch.randn(n, D, device=dev).to(DTYPES[dname])
    p0, p1 = _params(kind, mode, D, dev)
    kw = dict(relu=relu, seed=21, offset=7)
    got = _raw(g.csr_t, G, _noise(g, D, kind, p0, p1, **kw), seg_len=seg_len)
    with hw_normals(oracle, dev):
        ref, _, _ = oracle.agg_bwd(oracle_graph(oracle, g, transposed=True), G.float().cpu().numpy(),
                                   _ospec(oracle, g, D, kind, p0, p1, **kw), want_dp=False)
    assert_close(got, ref, what=f"transposed {dname} {kind}/{mode} seg_len={seg_len}")


# ---- 4. plan forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("D", [24, 128, 520])
def test_plan_forms_and_determinism(dev, oracle, dname, D):
    g = GRAPHS["hub"](dev)
    n = g.number_of_nodes()
    og = oracle_graph(oracle, g)
    x = torch.randn(n, D, device=dev).to(DTYPES[dname])
    p0, p1 = _params("normal", 1, D, dev)
    kw = dict(seed=3, offset=1)
    noise = _noise(g, D, "normal", p0, p1, **kw)
    with hw_normals(oracle, dev):
        ref = oracle.agg_fwd(og, x.float().cpu().numpy(), _ospec(oracle, g, D, "normal", p0, p1, **kw))
    outs = {}
    for seg_len in (0, 16, 64):                              # 0: plan == NULL, the 700-edge hub row is one unit
        assert (g.csr.plan(seg_len) is None) == (seg_len == 0)
        outs[seg_len] = _raw(g.csr, x, noise, seg_len=seg_len)
        assert_close(outs[seg_len], ref, what=f"{dname} D={D} seg_len={seg_len}")
        again = _raw(g.csr, x, noise, seg_len=seg_len)
        assert torch.equal(again.view(torch.int32), outs[seg_len].view(torch.int32)), "two launches, the same bits"
    for seg_len in (16, 64):
        assert g.csr.plan(seg_len)["n_seg"] > 0
        xo = _raw_xcd(g.csr, x, noise, seg_len)
        assert torch.equal(xo.view(torch.int32), outs[seg_len].view(torch.int32)), "xcd_order changes no bit"


@pytest.mark.parametrize("kind", ["normal", "none"])
@pytest.mark.parametrize("D", [512, 64])
def test_merge_of_more_segments_than_one_round(dev, oracle, D, kind):
    """seg_len = 4 cuts the hub row into at least 175 segments.  The merge (agg_half_merge_kernel: unit_sum.hpp's
    seg_merge at 8 channels a lane, written out) adds them in groups of 16, one group per team and round, T = 256 / LPE
    teams: at D = 512 (LPE = 64, T = 4) a round takes 64 segments, so the hub needs three and ends on a partial group;
    at D = 64 (LPE = 8, T = 32) it needs one, with most teams idle."""
    g = GRAPHS["hub"](dev)
    n, seg_len = g.number_of_nodes(), 4
    T = 256 // max(8, min(64, D // 8))
    plan = g.csr.plan(seg_len, need=True)
    hub_segs = int(np.diff(plan["long_seg_ptr"].cpu().numpy()[:plan["n_long"] + 1]).max())
    assert hub_segs >= 175 and hub_segs % 16 != 0, "the last group of the hub row is partial"
    if D == 512:
        assert T == 4 and plan["n_seg"] > 16 * T and hub_segs > 2 * 16 * T, "three rounds"
    og = oracle_graph(oracle, g)
    x = torch.randn(n, D, device=dev).to(torch.bfloat16)
    ds = np.random.default_rng(D).uniform(0.5, 1.5, n).astype(np.float32)
    dsd = torch.from_numpy(ds).to(dev)
    p0, p1 = (None, None) if kind == "none" else _params(kind, 1, D, dev)
    kw = dict(seed=13, offset=4)
    noise = None if kind == "none" else _noise(g, D, kind, p0, p1, **kw)
    spec = _ospec(oracle, g, D, kind, p0, p1, **kw)
    for reduce in ("sum", "mean"):
        with hw_normals(oracle, dev):
            ref = oracle.agg_fwd(og, x.float().cpu().numpy(), spec, dst_scale=ds,
                                 reduce=oracle.REDUCE_MEAN if reduce == "mean" else oracle.REDUCE_SUM)
        got = _raw(g.csr, x, noise, reduce, None, dsd, seg_len=seg_len)
        assert_close(got, ref, what=f"D={D} {kind} {reduce} seg_len={seg_len}")
        again = _raw(g.csr, x, noise, reduce, None, dsd, seg_len=seg_len)
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)), "two launches, the same bits"
        whole = _raw(g.csr, x, noise, reduce, None, dsd, seg_len=0)             # no plan: the hub row is one unit
        assert_close(got, whole.cpu().numpy(), what=f"D={D} {kind} {reduce} seg_len={seg_len} against no plan")


# ---- 5. strided input -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
def test_strided_rows_and_misaligned_rows(dev, oracle, dname, monkeypatch):
    from stag_amd import _lib, ops
    g = GRAPHS["hub"](dev)
    n = g.number_of_nodes()
    big = torch.randn(n, 144, device=dev).to(DTYPES[dname])
    p0, p1 = _params("uniform", 0, 128, dev)
    kw = dict(seed=8, offset=4)
    noise = _noise(g, 128, "uniform", p0, p1, **kw)
    x = big[:, 8:136]
    assert x.stride(0) == 144 and x.data_ptr() % 16 == 0 and not x.is_contiguous()
    ref = oracle.agg_fwd(oracle_graph(oracle, g), x.float().cpu().numpy(), _ospec(oracle, g, 128, "uniform", p0, p1, **kw))
    assert_close(_raw(g.csr, x, noise), ref, what=f"{dname} rows of stride 144")
    xm = big[:, 4:132]
    assert xm.data_ptr() % 16 == 8
    with pytest.raises(_lib.StagHipError, match="rc=-38"):
        _raw(g.csr, xm, noise)
    monkeypatch.setattr(ops, "HALF_ROWS", True)
    assert not ops.half_rows_ok(xm, None, noise, False, g) and ops.half_rows_ok(x, None, noise, False, g)
    with torch.no_grad():
        assert torch.equal(ops.aggregate(g, xm, noise), ops.aggregate(g, xm.float(), noise))
        assert torch.equal(ops.aggregate(g, x, noise), _raw(g.csr, x, noise))


def test_rows_past_the_24_bit_row_index(dev, oracle):
    """n_src >= 2^24: the 24-bit multiply behind the buffer descriptor does not reach every row, and the kernel takes
    64-bit addresses.  Three destination rows gather five rows around 2^24 of a [2^24 + 5, 8] table."""
    from stag_amd import _lib
    from stag_amd.graph import CsrView
    n_src, D = (1 << 24) + 5, 8
    rows = [0, (1 << 24) + 1, 5, (1 << 24) - 1, (1 << 24) + 4]
    indptr = torch.tensor([0, 2, 2, 5], dtype=torch.int32, device=dev)
    csrv = CsrView(3, n_src, indptr, torch.tensor(rows, dtype=torch.int32, device=dev))
    small = oracle.CsrGraph(indptr.cpu().numpy(), np.arange(5, dtype=np.int32), n_src=5)
    for dname, kind in (("bf16", "normal"), ("fp16", "none")):
        x = torch.zeros(n_src, D, device=dev, dtype=DTYPES[dname])
        vals = torch.randn(5, D, device=dev).to(DTYPES[dname])
        x[torch.tensor(rows, device=dev)] = vals
        spec = _lib.NoiseSpec()
        ospec = oracle.make_spec("none")
        if kind == "normal":
            spec.kind, spec.p0_scalar, spec.p1_scalar, spec.seed, spec.offset = _lib.NOISE_NORMAL, 1.0, 0.5, 7, 3
            ospec = oracle.make_spec("normal", 1.0, 0.5, seed=7, offset=3, Dn=D, n_edges=5)
        from stag_amd import ops
        got = ops._agg_half_raw(csrv, x, D, spec, 0, None, None, 0)
        with hw_normals(oracle, dev):
            ref = oracle.agg_fwd(small, vals.float().cpu().numpy(), ospec)
        assert_close(got, ref, what=f"wide addressing {dname} {kind}")
        del x


# ---- 6. routing and autograd -------------------------------------------------------------------------------------
def _counted(monkeypatch):
    from stag_amd import ops
    calls = []
    real = ops._agg_half_raw

    def wrapper(*a, **kw):
        calls.append(a[1].dtype)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "_agg_half_raw", wrapper)
    return calls


@pytest.mark.parametrize("dname", list(DTYPES))
def test_aggregate_routes_half_rows_and_backward_is_the_cast_route_s(dev, dname, monkeypatch):
    from stag_amd import ops
    g = GRAPHS["hub"](dev)
    n, D = g.number_of_nodes(), 64
    xh = torch.randn(n, D, device=dev).to(DTYPES[dname])
    p0, p1 = _params("normal", 1, D, dev)
    noise = _noise(g, D, "normal", p0, p1, relu=True, seed=13, offset=6)
    ss, ds = torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) + 0.5
    G = torch.randn(n, D, device=dev)
    calls = _counted(monkeypatch)
    monkeypatch.setattr(ops, "HALF_ROWS", True)
    with torch.no_grad():
        out = ops.aggregate(g, xh, noise, reduce="mean", src_scale=ss, dst_scale=ds)
    assert len(calls) == 1 and out.dtype == torch.float32
    assert torch.equal(out, _raw(g.csr, xh, noise, "mean", ss, ds))
    assert torch.equal(ops.aggregate(g, xh, None), _raw(g.csr, xh, None))
    xg = xh.clone().requires_grad_(True)
    n_before = len(calls)
    og = ops.aggregate(g, xg, noise, reduce="mean", src_scale=ss, dst_scale=ds)
    assert len(calls) == n_before + 1 and torch.equal(og.detach(), out)
    og.backward(G)
    assert xg.grad.dtype == DTYPES[dname]
    monkeypatch.setattr(ops, "HALF_ROWS", False)
    xf = xh.float().requires_grad_(True)
    n_before = len(calls)
    of = ops.aggregate(g, xf, noise, reduce="mean", src_scale=ss, dst_scale=ds)
    of.backward(G)
    assert len(calls) == n_before
    assert torch.equal(xg.grad, xf.grad.to(DTYPES[dname]))


@pytest.mark.parametrize("dname", list(DTYPES))
def test_every_fallback_is_the_cast_route(dev, dname, monkeypatch):
    import stag_amd
    from stag_amd import _lib, ops
    g = GRAPHS["hub"](dev)
    n, E = g.number_of_nodes(), g.number_of_edges()
    calls = _counted(monkeypatch)
    monkeypatch.setattr(ops, "HALF_ROWS", True)
    x64 = torch.randn(n, 64, device=dev).to(DTYPES[dname])
    x50 = torch.randn(n, 50, device=dev).to(DTYPES[dname])
    cases = {
        "D = 50": (x50, _noise(g, 50, "normal", 1.0, 0.4, seed=2, offset=1)),
        "in-norm": (x64, _noise(g, 64, "bernoulli", 0.7, None, in_norm=True, seed=2, offset=1)),
        "explicit weights": (x64, torch.rand(E, 64, device=dev)),
        "per-edge parameters": (x64, stag_amd.EdgeNoise(g, 64, _lib.NOISE_NORMAL, torch.rand(E, 1, device=dev),
                                                        torch.rand(E, 1, device=dev), seed=2, offset=1)),
    }
    with torch.no_grad():
        for name, (x, w) in cases.items():
            assert torch.equal(ops.aggregate(g, x, w), ops.aggregate(g, x.float(), w)), name
        assert not calls
        nz = _noise(g, 64, "normal", 1.0, 0.4, seed=2, offset=1)
        ops.aggregate(g, x64, nz)
        assert len(calls) == 1
        monkeypatch.setattr(ops, "HALF_ROWS", False)
        assert torch.equal(ops.aggregate(g, x64, nz), ops.aggregate(g, x64.float(), nz))
        assert len(calls) == 1


# ---- 7. a layer under autocast ---------------------------------------------------------------------------------
def test_layer_under_autocast_takes_the_half_rows(dev, monkeypatch):
    """Under torch.autocast a dense transform hands the next layer a bf16 h = x @ W: StagLayer(GCN) aggregates it as
    it is, returns fp32, and a training step reaches every parameter."""
    import stag_amd
    from stag_amd import ops
    g = GRAPHS["hub"](dev)
    n = g.number_of_nodes()
    calls = _counted(monkeypatch)
    monkeypatch.setattr(ops, "HALF_ROWS", True)
    torch.manual_seed(0)
    pre = torch.nn.Linear(24, 16).to(dev)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(16, 64), q_a=torch.distributions.Normal(1.0, 0.3)).to(dev)
    x0 = torch.randn(n, 24, device=dev)
    stag_amd.manual_seed(77)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = pre(x0)
        assert h.dtype == torch.bfloat16
        out = layer(g, h)
    assert calls == [torch.bfloat16]
    assert out.dtype == torch.float32 and out.shape == (n, 64) and torch.isfinite(out).all()
    out.square().mean().backward()
    params = list(pre.parameters()) + [p for p in layer.parameters() if p.requires_grad]
    assert len(params) >= 4
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
