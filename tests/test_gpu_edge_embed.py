"""The wide edge embedding h = SiLU(ps[src] + pd[dst]) on the GPU: stag_edge_embed_fwd / _bwd and ops.edge_embed against
float64 arithmetic on the same fp32 inputs (torch on the CPU), determinism, degenerate graphs, the segment merge over
more than one round, the composed expression, AmortizedDistribution.condition with the switch on and off, and the memory
the forward retains."""
import numpy as np
import pytest
import torch

from util import TOL, assert_close, assert_close_cond

pytestmark = pytest.mark.gpu

N = 60
WIDTHS = (1, 5, 16, 20, 132, 260, 1436)


def _base_edges():
    """400 random edges with destinations in [0, N - 1) (the last node has no in-edge), a 1,300-edge hub into node 3;
    multi-edges and self loops included."""
    rng = np.random.default_rng(0)
    src = np.concatenate([rng.integers(0, N, 400), rng.integers(0, N, 1300)])
    dst = np.concatenate([rng.integers(0, N - 1, 400), np.full(1300, 3)])
    src[:8], dst[:8] = dst[:8], dst[:8]                   # self loops
    src[8:16], dst[8:16] = src[16:24], dst[16:24]         # multi-edges
    return src, dst


@pytest.fixture(scope="module")
def base(dev):
    import stag_amd
    src, dst = _base_edges()
    return stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), N, device=dev)


def _tables(n, hidden, seed, E):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, hidden, generator=gen) * 2.0, torch.randn(n, hidden, generator=gen) * 2.0,
            torch.randn(E, hidden, generator=gen))


_REF = {}


def _reference(key, src, dst, ps, pd, g, n):
    """float64 on the same fp32 inputs: h, d ps, d pd and the sums of |g SiLU'| per row (computed once per case)."""
    if key not in _REF:
        s, d = torch.from_numpy(np.asarray(src)).long(), torch.from_numpy(np.asarray(dst)).long()
        pre = ps.double()[s] + pd.double()[d]
        sg = torch.sigmoid(pre)
        term = g.double() * (sg * (1.0 + pre * (1.0 - sg)))
        zeros = torch.zeros(n, ps.shape[1], dtype=torch.float64)
        _REF[key] = tuple(t.numpy() for t in (
            pre * sg, zeros.index_add(0, s, term), zeros.index_add(0, d, term),
            zeros.index_add(0, s, term.abs()), zeros.index_add(0, d, term.abs())))
    return _REF[key]


def _padded(t, dev):
    """t as the second half of an [n, 2 hidden] table: rows hidden floats long, 2 hidden apart."""
    hidden = t.shape[1]
    full = torch.full((t.shape[0], 2 * hidden), float("nan"), device=dev)
    full[:, hidden:] = t.to(dev)
    return full[:, hidden:]


def _run(graph, ps, pd, g, dev, seg_len=None, padded=False):
    from stag_amd import ops
    from stag_amd.graph import DEFAULT_SEG_LEN
    seg_len = DEFAULT_SEG_LEN if seg_len is None else seg_len
    put = (lambda t: _padded(t, dev)) if padded else (lambda t: t.to(dev))
    psd, pdd, gd = put(ps), put(pd), put(g)
    if padded:
        assert psd.stride(0) == 2 * ps.shape[1] and ops._rows32(psd) is psd
    h = ops._edge_embed_fwd_raw(graph._src, graph._dst, psd, pdd, out=put(torch.zeros_like(g)) if padded else None)
    d_src = ops._edge_embed_bwd_raw(graph.csr_t, psd, pdd, gd, seg_len=seg_len)
    d_dst = ops._edge_embed_bwd_raw(graph.csr, pdd, psd, gd, seg_len=seg_len)
    return h, d_src, d_dst


CASES = [(w, 16, False) for w in WIDTHS] + [(w, None, False) for w in WIDTHS] + [(20, 16, True), (16, None, True), (5, 16, True)]


@pytest.mark.parametrize("hidden,seg_len,padded", CASES)
def test_forward_and_both_backward_orientations_against_float64(dev, base, hidden, seg_len, padded):
    src, dst = _base_edges()
    ps, pd, g = _tables(N, hidden, hidden, len(src))
    h_ref, ds_ref, dd_ref, ds_abs, dd_abs = _reference(("base", hidden), src, dst, ps, pd, g, N)
    if seg_len == 16:
        plan = base.csr.plan(16)
        assert plan is not None and plan["n_seg"] > 16, "the hub is cut into segments"
    h, d_src, d_dst = _run(base, ps, pd, g, dev, seg_len, padded)
    assert_close(h, h_ref, what=f"h, hidden {hidden}")
    assert_close_cond(d_src, ds_ref, ds_abs, what=f"d ps, hidden {hidden}, seg_len {seg_len}")
    assert_close_cond(d_dst, dd_ref, dd_abs, what=f"d pd, hidden {hidden}, seg_len {seg_len}")
    assert not d_dst[N - 1].any(), "a row without edges is zeros"


@pytest.mark.parametrize("hidden,seg_len", [(5, 16), (132, 16), (260, None)])
def test_two_runs_give_identical_bits(dev, base, hidden, seg_len):
    src, _ = _base_edges()
    ps, pd, g = _tables(N, hidden, hidden, len(src))
    a = _run(base, ps, pd, g, dev, seg_len)
    b = _run(base, ps, pd, g, dev, seg_len)
    for x, y, what in zip(a, b, ("h", "d ps", "d pd")):
        assert torch.equal(x, y), what


@pytest.mark.parametrize("edges", [0, 1])
def test_degenerate_graphs(dev, edges):
    import stag_amd
    from stag_amd import ops
    n, hidden = 5, 20
    src = torch.tensor([2][:edges], dtype=torch.int64)
    dst = torch.tensor([4][:edges], dtype=torch.int64)
    graph = stag_amd.Graph(src, dst, n, device=dev)
    ps, pd, g = _tables(n, hidden, 3, edges)
    psd, pdd, gd = ps.to(dev), pd.to(dev), g.to(dev)
    h = ops._edge_embed_fwd_raw(graph._src, graph._dst, psd, pdd)
    assert h.shape == (edges, hidden)
    h_ref, ds_ref, dd_ref, _, _ = _reference(("degenerate", edges), src.numpy(), dst.numpy(), ps, pd, g, n)
    assert_close(h, h_ref, what="h")
    for view, own, other, ref, row in ((graph.csr_t, psd, pdd, ds_ref, 2), (graph.csr, pdd, psd, dd_ref, 4)):
        out = torch.full((n, hidden), float("nan"), device=dev)
        got = ops._edge_embed_bwd_raw(view, own, other, gd, out=out)
        assert got is out and not torch.isnan(out).any()
        assert_close(out, ref, what="d_own")
        keep = torch.ones(n, dtype=torch.bool)
        if edges:
            keep[row] = False
        assert not out[keep.to(dev)].any(), "rows without edges come back as zeros"


@pytest.mark.parametrize("hidden,hub,seg_len", [(256, 0, 16), (16, 16400, 16)])
def test_segment_merge_over_more_than_one_round(dev, base, hidden, hub, seg_len):
    """A merge workgroup has 256 / lanes teams and a team adds one group of 16 partials per round: hidden 256 (64 lanes,
    4 teams) on the base graph at seg_len 16 has 82 segments in the hub row, more than 4 x 16; hidden 16 (4 lanes, 64
    teams) needs more than 1,024 segments, which a 16,400-edge hub at seg_len 16 gives."""
    import stag_amd
    if hub:
        rng = np.random.default_rng(5)
        src = np.concatenate([rng.integers(0, N, 200), rng.integers(0, N, hub)])
        dst = np.concatenate([rng.integers(0, N - 1, 200), np.full(hub, 3)])
        graph = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), N, device=dev)
    else:
        (src, dst), graph = _base_edges(), base
    plan = graph.csr.plan(seg_len)
    teams = 256 // max(4, min(64, hidden // 4))
    assert plan["n_seg"] > 16 * teams, "more than one round of the merge"
    ps, pd, g = _tables(N, hidden, 100 + hidden, len(src))
    _, ds_ref, dd_ref, ds_abs, dd_abs = _reference(("merge", hidden), src, dst, ps, pd, g, N)
    _, d_src, d_dst = _run(graph, ps, pd, g, dev, seg_len)
    assert_close_cond(d_dst, dd_ref, dd_abs, what=f"d pd, hidden {hidden}")
    assert_close_cond(d_src, ds_ref, ds_abs, what=f"d ps, hidden {hidden}")


@pytest.mark.parametrize("hidden", [5, 132])
def test_op_against_the_composed_expression(dev, base, hidden):
    from stag_amd import ops
    src, dst = _base_edges()
    ps, pd, g = _tables(N, hidden, hidden, len(src))
    h_ref, ds_ref, dd_ref, ds_abs, dd_abs = _reference(("base", hidden), src, dst, ps, pd, g, N)
    gd = g.to(dev)
    got = []
    for fused in (True, False):
        a, b = ps.to(dev).requires_grad_(True), pd.to(dev).requires_grad_(True)
        h = (ops.edge_embed(base, a, b) if fused else
             torch.nn.functional.silu(ops.gather_rows(base, a, "src") + ops.gather_rows(base, b, "dst")))
        h.backward(gd)
        got.append((h.detach(), a.grad, b.grad))
    for (h, da, db), route in zip(got, ("fused", "composed")):
        assert_close(h, h_ref, what=f"{route} h")
        assert_close_cond(da, ds_ref, ds_abs, what=f"{route} d p_src")
        assert_close_cond(db, dd_ref, dd_abs, what=f"{route} d p_dst")
    # only the second table needs a gradient: the other launch is skipped
    a, b = ps.to(dev), pd.to(dev).requires_grad_(True)
    ops.edge_embed(base, a, b).backward(gd)
    assert torch.equal(b.grad, got[0][2])
    # half-typed tables under autocast come in as fp32 copies
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h16 = ops.edge_embed(base, ps.to(dev).bfloat16(), pd.to(dev).bfloat16())
    assert h16.dtype == torch.float32
    with pytest.raises(ValueError):
        ops.edge_embed(base, ps.to(dev)[:-1], pd.to(dev)[:-1])


def test_condition_with_the_switch_on_against_off(dev, base, monkeypatch):
    from stag_amd import ops
    from stag_amd.distributions import AmortizedDistribution
    torch.manual_seed(4)
    q = AmortizedDistribution(16, 16).to(dev)
    x0 = torch.randn(N, 16, generator=torch.Generator().manual_seed(9)).to(dev)
    res = {}
    calls = []
    real = ops.edge_embed
    monkeypatch.setattr(ops, "edge_embed", lambda *a: (calls.append(1), real(*a))[1])
    for fused in (False, True):
        monkeypatch.setattr(ops, "EDGE_EMBED_FUSED", fused)
        q.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        q.condition(base, x)
        loc, ls = q.new_parameters["loc"], q.new_parameters["log_scale"]
        (loc.sum() + (ls ** 2).sum()).backward()
        res[fused] = (loc.detach(), ls.detach(), x.grad.clone(), {k: p.grad.clone() for k, p in q.named_parameters()})
        assert len(calls) == int(fused)
    off, on = res[False], res[True]
    assert_close(on[0], off[0].cpu().numpy(), what="loc")
    assert_close(on[1], off[1].cpu().numpy(), what="log_scale")
    for got, ref, what in [(on[2], off[2], "d/dx")] + [(on[3][k], off[3][k], f"d/d{k}") for k in off[3]]:
        ref = ref.cpu().numpy()
        s = max(1.0, float(np.abs(ref).max()))
        assert_close(got / s, ref / s, what=what)


def test_forward_retains_no_pre_activation(dev):
    """E = 4,096, hidden = 128: after the forward with requires_grad tables the composed route holds the output and the
    pre-activation for SiLU's backward, the fused one the output alone."""
    import stag_amd
    from stag_amd import ops
    n, E, hidden = 512, 4096, 128
    gen = torch.Generator().manual_seed(1)
    graph = stag_amd.Graph(torch.randint(0, n, (E,), generator=gen), torch.randint(0, n, (E,), generator=gen), n, device=dev)
    ps = torch.randn(n, hidden, generator=gen).to(dev).requires_grad_(True)
    pd = torch.randn(n, hidden, generator=gen).to(dev).requires_grad_(True)
    held = {}
    for fused in (False, True, False, True):      # (the first pair also builds whatever the graph caches)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        h = (ops.edge_embed(graph, ps, pd) if fused else
             torch.nn.functional.silu(ops.gather_rows(graph, ps, "src") + ops.gather_rows(graph, pd, "dst")))
        torch.cuda.synchronize()
        held[fused] = torch.cuda.memory_allocated() - before
        del h
    assert held[False] - held[True] >= E * hidden * 4, held
