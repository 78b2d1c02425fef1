"""The wide edge embedding across the float range: stag_edge_embed_fwd and both orientations of stag_edge_embed_bwd at
hidden 5, 16 and 260 (4 lanes unvectorised, 4 lanes vectorised, 64 lanes and two channel tiles), without a plan and at
seg_len 16, against float64 on the same fp32 inputs with the pre-activation rounded to fp32 first (the kernel's documented
function is of the rounded sum).  tests/edge_embed_range_cases.py holds the graph and the references;
tests/test_edge_embed_range_host.py shows that a float32 restatement of the formula meets the same bars on the same
inputs, so the bars (util.TOL: assert_close for h, assert_close_cond for the sums over a row's edges) are properties of
the inputs.

PLANTED: pre-activations of +-100, +-1000, around the overflow of expf(-pre) (-87, -88.5, -88.75, -104), where 1 - sg
vanishes (16, 17, 18), at the zero of SiLU' and at 0, each through the own row and through the gathered row, each summed
with ordinary terms.  MAGNITUDES: tables at 2^-60 and g at 2^+-60, compared after an exact rescaling.  CONTAINMENT: a NaN
row of either table or of g makes NaN exactly the outputs that read it and leaves every other output bit for bit what the
clean run gives; +-inf rows give the NaN / inf pattern of the documented formula."""
import numpy as np
import pytest
import torch

import edge_embed_range_cases as ec
from util import assert_close, assert_close_cond

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def graph(dev):
    import stag_amd
    src, dst = ec.edges()
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), ec.N, device=dev)
    plan = g.csr.plan(16, need=True)
    assert plan["n_long"] >= 1 and plan["n_seg"] >= 9, "the hub is cut into segments"
    return g


def _run(graph, ps, pd, g, dev, seg_len):
    """(h, d ps, d pd) of one forward and the two backward launches, as numpy arrays"""
    from stag_amd import ops
    psd, pdd, gd = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (ps, pd, g))
    h = ops._edge_embed_fwd_raw(graph._src, graph._dst, psd, pdd)
    d_src = ops._edge_embed_bwd_raw(graph.csr_t, psd, pdd, gd, seg_len=seg_len)
    d_dst = ops._edge_embed_bwd_raw(graph.csr, pdd, psd, gd, seg_len=seg_len)
    return [t.cpu().numpy() for t in (h, d_src, d_dst)]


def _clean(hidden):
    if hidden not in _REF:
        t = ec.tables(hidden)
        _REF[hidden] = (t, ec.reference(*t))
    return _REF[hidden]


@pytest.mark.parametrize("hidden", ec.HIDDENS)
def test_planted_pre_activations(dev, graph, hidden):
    (ps, pd, g), (h_ref, ds_ref, dd_ref, ds_abs, dd_abs) = _clean(hidden)
    src, dst = ec.edges()
    pl = ec.planted_edges()
    for seg in ec.SEGS:
        what = f"hidden {hidden} seg_len {seg}"
        h, d_src, d_dst = _run(graph, ps, pd, g, dev, seg)
        for a, nm in ((h, "h"), (d_src, "d ps"), (d_dst, "d pd")):
            assert np.isfinite(a).all(), f"{what}: {nm} is not finite at {np.argwhere(~np.isfinite(a))[:4].tolist()}"
        assert_close(h, h_ref, what=f"{what} h")
        assert_close_cond(d_src, ds_ref, ds_abs, what=f"{what} d ps")
        assert_close_cond(d_dst, dd_ref, dd_abs, what=f"{what} d pd")
        for i, v in enumerate(ec.PLANTED):                      # a failure names the planted value
            e = pl[i]
            assert_close(h[e], h_ref[e], what=f"{what} h at pre = {v}")
            assert_close_cond(d_src[src[e]], ds_ref[src[e]], ds_abs[src[e]], what=f"{what} d ps at pre = {v}")
            assert_close_cond(d_dst[dst[e]], dd_ref[dst[e]], dd_abs[dst[e]], what=f"{what} d pd at pre = {v}")
        assert not d_src[ec.N - 1].any() and not d_dst[ec.N - 1].any(), "a node without edges"


@pytest.mark.parametrize("g_exp", (60, -60))
@pytest.mark.parametrize("hidden", ec.HIDDENS)
def test_magnitudes(dev, graph, hidden, g_exp):
    """Tables at 2^-60, g at 2^+-60; both sides are multiplied by the exact inverse power of two before the comparison."""
    ps, pd, g = ec.tables(hidden, scale=2.0 ** -60, g_scale=2.0 ** g_exp)
    h_ref, ds_ref, dd_ref, ds_abs, dd_abs = ec.reference(ps, pd, g)
    k, kg = 2.0 ** 60, 2.0 ** -g_exp
    for seg in ec.SEGS:
        what = f"hidden {hidden} g 2^{g_exp} seg_len {seg}"
        h, d_src, d_dst = (a.astype(np.float64) for a in _run(graph, ps, pd, g, dev, seg))
        assert_close(h * k, h_ref * k, what=f"{what} h")
        assert_close_cond(d_src * kg, ds_ref * kg, ds_abs * kg, what=f"{what} d ps")
        assert_close_cond(d_dst * kg, dd_ref * kg, dd_abs * kg, what=f"{what} d pd")


def _same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).view(np.int32) == np.ascontiguousarray(b, np.float32).view(np.int32)


def _contained(got, clean, hit, what):
    """NaN in every channel of the rows of `hit`, the bits of the clean run in every other row"""
    nan = np.isnan(got)
    assert (nan == hit[:, None]).all(), (f"{what}: NaN in rows {np.flatnonzero(nan.any(1) & ~hit)[:8].tolist()} that do not read "
                                         f"the planted row, none in rows {np.flatnonzero(~nan.all(1) & hit)[:8].tolist()} that do")
    assert _same_bits(got[~hit], clean[~hit]).all(), f"{what}: a row that does not read the planted row changed"


@pytest.mark.parametrize("where", ("ps", "pd", "g"))
@pytest.mark.parametrize("hidden", ec.HIDDENS)
def test_a_nan_row_stays_inside_the_rows_that_read_it(dev, graph, hidden, where):
    (ps, pd, g), _ = _clean(hidden)
    src, dst = ec.edges()
    node = ec.NAN_NODE
    e0 = int(np.flatnonzero(dst == ec.HUB)[40])                 # an edge inside the hub's row: one segment of several
    nodes = np.arange(ec.N)
    if where == "g":
        g = g.copy()
        g[e0] = np.nan
        hit_h = np.zeros(len(src), bool)                       # the forward does not read g
        hit_s, hit_d = nodes == src[e0], nodes == dst[e0]
    else:
        t = (ps if where == "ps" else pd).copy()
        t[node] = np.nan
        ps, pd = (t, pd) if where == "ps" else (ps, t)
        mine, far = (src, dst) if where == "ps" else (dst, src)
        hit_h = mine == node
        own_hit, other_hit = nodes == node, np.isin(nodes, far[hit_h])
        hit_s, hit_d = (own_hit, other_hit) if where == "ps" else (other_hit, own_hit)
        assert hit_h.sum() >= 2 and 2 <= other_hit.sum() < ec.N // 2
    for seg in ec.SEGS:
        what = f"NaN row of {where}, hidden {hidden}, seg_len {seg}"
        clean = _run(graph, *_clean(hidden)[0], dev, seg)
        h, d_src, d_dst = _run(graph, ps, pd, g, dev, seg)
        _contained(h, clean[0], hit_h, f"{what}: h")
        _contained(d_src, clean[1], hit_s, f"{what}: d ps")
        _contained(d_dst, clean[2], hit_d, f"{what}: d pd")


@pytest.mark.parametrize("hidden", ec.HIDDENS)
def test_infinite_rows_give_the_pattern_of_the_documented_formula(dev, graph, hidden):
    """ps[NAN_NODE] = +inf and pd[NAN_NODE + 1] = -inf: SiLU(+inf) = +inf, SiLU(-inf) = -inf * 0 = NaN, SiLU' = NaN on both
    sides (inf * 0 inside it), inf - inf = NaN where the two nodes share an edge.  Where the float64 restatement of the
    formula is NaN the kernel's output is NaN, where it is +-inf the kernel's is the same infinity, and everything else is
    finite and within the bars."""
    (ps, pd, g), _ = _clean(hidden)
    ps, pd = ps.copy(), pd.copy()
    ps[ec.NAN_NODE], pd[ec.NAN_NODE + 1] = np.inf, -np.inf
    refs = ec.reference(ps, pd, g, silu=ec.silu_formula64)
    assert np.isposinf(refs[0]).any() and np.isnan(refs[0]).any() and np.isnan(refs[1]).any() and np.isnan(refs[2]).any()
    for seg in ec.SEGS:
        got = _run(graph, ps, pd, g, dev, seg)
        for a, r, ab, nm in zip(got, refs[:3], (None, refs[3], refs[4]), ("h", "d ps", "d pd")):
            what = f"hidden {hidden} seg_len {seg} {nm}"
            assert (np.isnan(a) == np.isnan(r)).all(), f"{what}: NaN where the formula has none, or the reverse"
            inf = np.isinf(r)
            assert (np.isinf(a) == inf).all() and (a[inf] == r[inf]).all(), f"{what}: another set of infinities"
            ok = np.isfinite(r)
            if ab is None:
                assert_close(a[ok], r[ok], what=what)
            else:
                assert_close_cond(a[ok], r[ok], ab[ok], what=what)
