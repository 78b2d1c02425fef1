"""The entry points that came after tests/test_gpu_address_forms.py, on both sides of their address-form switches, by the
same method: tables random everywhere, every launch against a float64 reference on the relabelled gathered rows at
util.TOL and bit for bit (torch.equal) against the same launch on the packed layout, which takes the narrow form.

stag_edge_embed_bwd carries two switches (csrc/edge_embed.hip, gather4): x_bytes on the gathered node table and g_bytes
on the [E, hidden] gradient table gathered by edge id; both share one `xvec`.  stag_agg_bwd_pedge carries one, g_bytes
on the gathered g rows (csrc/agg_bwd_pedge.hip), and reads and writes [E, D] parameter tables by edge id.
stag_edge_embed_fwd has no switch but forms e * ldh in 64 bits over a grid of E edges.  FORMS, the structure of four
destination rows and the per-edge graph of 2^24 + 64 positions are those of tests/test_gpu_address_forms.py;
tests/test_address_forms_new_host.py places every shape on the intended side of narrow_rows."""
import numpy as np
import pytest
import torch

import edge_embed_range_cases as ec
import test_gpu_address_forms as G
from test_gpu_address_forms import FORMS, K24, N_EDGES, PE_EDGES, PE_N_DST, PE_N_SRC, SEGS, _Checker, _dev, _Spec
from util import TOL, assert_close, assert_close_cond, hw_normals

pytestmark = pytest.mark.gpu

PE_HIDDEN = 8                 # the [E, 8] gradient table of the per-edge run: 2^29 + 2^11 bytes, rows past 2^24
PE_SEG = 64
FWD_NODES = K24 + 5           # stag_edge_embed_fwd: node ids past 2^24
FWD_WIDTHS = (8, 6)
FWD_LDH = 160                 # ... and h rows 160 floats apart at hidden 8: e * ldh passes 2^31 elements, its bytes 2^32
FWD_STRIDE = 4099             # the strided sample of its edges


@pytest.fixture(autouse=True)
def _ctypes_front_end(monkeypatch):
    from stag_amd import _torch_ext
    monkeypatch.setattr(_torch_ext, "available", lambda: False)


def _silu_d(pre32):
    return ec.silu64(np.asarray(pre32, np.float32).astype(np.float64))[1]


def _embed_ref(view, own, other, g):
    """(d_own, sum |terms|) in float64 over an oracle CsrGraph: rows own, columns gathered, g by edge id"""
    rows = view.dst_of_pos
    term = g[view.eid].astype(np.float64) * _silu_d(own[rows] + other[view.indices])
    out, ab = np.zeros((view.n_dst, own.shape[1])), np.zeros((view.n_dst, own.shape[1]))
    np.add.at(out, rows, term)
    np.add.at(ab, rows, np.abs(term))
    return out, ab


# ---- stag_edge_embed_bwd: the gathered node table through the forms ---------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_edge_embed_bwd_other_table_in_each_form(dev, oracle, form):
    """`other` has n_src rows in the layout of the form, `own` the four destination rows, g the 46 edges (narrow): x_bytes
    switches, g_bytes stays narrow — the wide x with the narrow g of the mixed runs.  A vectorised and an unvectorised
    width, without a plan and at seg_len 16 (the hub in three segments)."""
    from stag_amd import ops
    f = FORMS[form]
    n_src, src = f["n_src"], torch.tensor(f["sources"], device=dev)
    og, ogt = G._structure(oracle, len(f["sources"]), seed=ord(form))
    views = G._views(ogt, f["sources"], n_src, dev)
    check = _Checker(f"form ({form})")
    rng = np.random.default_rng(ord(form) + 100)
    ld = f["stride_bytes"] // 4
    flat = G._table(n_src, ld, torch.float32, dev)
    for D in f["widths"]:
        xt = flat.as_strided((n_src, D), (ld, 1))
        assert xt.stride(0) * 4 == f["stride_bytes"] and xt.data_ptr() % 16 == 0
        xp = xt[src].contiguous()
        own = rng.standard_normal((4, D)).astype(np.float32)
        g = rng.standard_normal((N_EDGES, D)).astype(np.float32)
        ownd, gd = _dev(own, dev), _dev(g, dev)
        ref, ab = _embed_ref(ogt, own, xp.cpu().numpy(), g)
        for seg in SEGS:
            got = [ops._edge_embed_bwd_raw(v, ownd, x, gd, seg_len=seg) for v, x in ((views[0], xt), (views[1], xp))]
            check(f"stag_edge_embed_bwd D={D} seg_len={seg}", [got[0]], [got[1]], [(ref, 1.0)])     # (40 terms: the plain bar)
    assert not check.errs, "\n".join(check.errs)


# ---- the per-edge graph: g gathered by permuted edge ids past 2^24 ------------------------------------------------------------
def test_edge_embed_bwd_gradient_rows_past_2_24_ids(dev, oracle):
    """E = 2^24 + 64, hidden 8: g [E, 8] is gathered at permuted edge ids on both sides of 2^24 (g_bytes wide) while `other`
    (1000 rows) stays narrow — the other mixed run.  Every row against float64 arithmetic on the device (torch, the same
    fp32 inputs), the checked rows of the per-edge graph against numpy float64 on the host, and those rows bit for bit
    against the launch on the compact graph with g packed (both narrow; a row's segments depend on its length alone).  The
    bar is util.assert_close_cond's: a row adds some 2097 terms g SiLU' of both signs, each rounded to fp32 once by the kernel
    and formed in double by the reference, so a sum that cancels misses the plain bar whatever the order of addition
    (observed over the 8000 x 8 sums: 9.4e-06 plain, 0.12 of the conditioned bar; profiles/r26/new_suites.txt)."""
    from stag_amd import ops
    from stag_amd.graph import CsrView
    E, D = PE_EDGES, PE_HIDDEN
    view, indptr_h, rows = G._pe_graph(dev)
    og, pos, ids = G._pe_compact(oracle, view, indptr_h, rows)
    rows_d, ids_d = torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev)
    assert (ids >= K24).sum() >= 8 and (ids < K24).sum() >= 8 and pos.max() == E - 1
    own = torch.randn(PE_N_DST, D, device=dev)
    other = torch.randn(PE_N_SRC, D, device=dev)
    g = torch.randn(E, D, device=dev)
    got = ops._edge_embed_bwd_raw(view, own, other, g, seg_len=PE_SEG)
    # every row, float64 on the device
    u_of = torch.repeat_interleave(torch.arange(PE_N_DST, device=dev), view.degrees.long())
    pre = (own[u_of] + other[view.indices.long()]).double()
    sg = torch.sigmoid(pre)
    term = g[view.eid.long()].double() * (sg * (1.0 + pre * torch.sigmoid(-pre)))
    del pre, sg
    zeros = torch.zeros(PE_N_DST, D, dtype=torch.float64, device=dev)
    ref_all, ab_all = zeros.index_add(0, u_of, term), zeros.index_add(0, u_of, term.abs())
    del term, u_of
    assert_close_cond(got, ref_all.cpu().numpy(), ab_all.cpu().numpy(), what="stag_edge_embed_bwd, g past 2^24 ids, every row")
    # the checked rows, float64 on the host
    ref, ab = _embed_ref(og, own[rows_d].cpu().numpy(), other.cpu().numpy(), g[ids_d].cpu().numpy())
    assert_close_cond(got[rows_d], ref, ab, what="stag_edge_embed_bwd, g past 2^24 ids, checked rows")
    # ... and the same rows from the compact graph with g packed: the narrow form of both switches
    compact = CsrView(len(rows), PE_N_SRC, _dev(og.indptr, dev), _dev(og.indices, dev), eid=_dev(og.eid, dev))
    packed = ops._edge_embed_bwd_raw(compact, own[rows_d].contiguous(), other, g[ids_d].contiguous(), seg_len=PE_SEG)
    assert torch.equal(got[rows_d], packed), "not the bits of the packed layout"


# ---- stag_edge_embed_fwd: 64-bit e * ldh, a grid over E, node ids past 2^24 ------------------------------------------------------
@pytest.mark.parametrize("hidden,ldh", [(w, w) for w in FWD_WIDTHS] + [(8, FWD_LDH)])
def test_edge_embed_fwd_past_2_24_edges_and_nodes(dev, hidden, ldh):
    """E = 2^24 + 64 edges over 2^24 + 5 nodes: planted edges (the first, the last, the ones around edge 2^24) join the node
    ids 0, 2^24 - 1, 2^24 and 2^24 + 4; they and every 4099th edge against float64 on the host, every edge against torch's
    SiLU of the same rounded sum in float64 on the device.  ldh = 160: h is the head of rows 160 floats apart (a 10.7 GB
    buffer that is never filled), so the row offset e * ldh needs more than 32 bits, in elements and in bytes."""
    from stag_amd import ops
    E, n = PE_EDGES, FWD_NODES
    src = torch.randint(0, n, (E,), device=dev, dtype=torch.int32)
    dst = torch.randint(0, n, (E,), device=dev, dtype=torch.int32)
    planted = np.array([0, 1, K24 - 1, K24, K24 + 1, E - 2, E - 1])
    nodes = np.array([0, K24 - 1, K24, K24 + 4, 0, K24 + 4, K24], np.int32)
    src[torch.from_numpy(planted).to(dev)] = torch.from_numpy(nodes).to(dev)
    dst[torch.from_numpy(planted).to(dev)] = torch.from_numpy(nodes[::-1].copy()).to(dev)
    ps, pd = torch.randn(n, hidden, device=dev), torch.randn(n, hidden, device=dev)
    out = None if ldh == hidden else torch.empty(E * ldh, device=dev).as_strided((E, hidden), (ldh, 1))
    h = ops._edge_embed_fwd_raw(src, dst, ps, pd, out=out)
    assert h.shape == (E, hidden) and h.stride(0) == ldh and ((E - 1) * ldh < (1 << 31)) == (ldh == hidden)
    sample = torch.from_numpy(np.unique(np.concatenate([planted, np.arange(0, E, FWD_STRIDE)]))).to(dev)
    s, d = src[sample].long(), dst[sample].long()
    assert int(s.max()) >= K24 and int(d.max()) >= K24
    pre = (ps[s] + pd[d]).cpu().numpy()
    assert_close(h[sample], ec.silu64(pre.astype(np.float64))[0], what=f"stag_edge_embed_fwd hidden {hidden}, planted and sampled edges")
    # every edge against the same expression on the device (fp32: torch's SiLU of the same rounded sum)
    worst = 0.0
    for a in range(0, E, 1 << 22):
        b = min(E, a + (1 << 22))
        want = torch.nn.functional.silu((ps[src[a:b].long()] + pd[dst[a:b].long()]).double())
        worst = max(worst, float(((h[a:b].double() - want).abs() / (1.0 + want.abs())).max()))
    assert worst <= TOL, f"stag_edge_embed_fwd hidden {hidden}: scaled error {worst:.3e} over all edges"


# ---- stag_agg_bwd_pedge: the gathered g rows through the forms -----------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_agg_bwd_pedge_g_in_each_form(dev, oracle, form):
    """g [n_src, D] in the layout of the form, x the four rows the units own, [E, D] parameter tables of the 46 edges:
    normal with a log-scale and uniform, with and without the two scales, at seg_len 0 and 16.  dx and both parameter
    gradients against the oracle (dx: its forward sum on the view every launch walks; d p_i: oracle.agg_bwd_w with deriv
    i + 1 on the scaled rows, as tests/test_gpu_bwd_pedge.py does), and the bits of the packed launch."""
    from stag_amd import ops
    f = FORMS[form]
    n_src, src = f["n_src"], torch.tensor(f["sources"], device=dev)
    og, ogt = G._structure(oracle, len(f["sources"]), seed=ord(form))
    views = G._views(ogt, f["sources"], n_src, dev)
    check = _Checker(f"form ({form})")
    rng = np.random.default_rng(ord(form) + 200)
    E = N_EDGES
    gst = 0.5 + torch.rand(n_src, device=dev)                  # g_scale over the table's rows
    gsp = gst[src].contiguous()
    rs = rng.uniform(0.5, 1.5, 4).astype(np.float32)           # row_scale over the four
    rsd = _dev(rs, dev)
    ld = f["stride_bytes"] // 4
    flat = G._table(n_src, ld, torch.float32, dev)
    with hw_normals(oracle, dev):
        for D in f["widths"]:
            gt = flat.as_strided((n_src, D), (ld, 1))
            gp = gt[src].contiguous()
            gn, gsn = gp.cpu().numpy(), gsp.cpu().numpy()
            x = rng.standard_normal((4, D)).astype(np.float32)
            xd = _dev(x, dev)
            q0, q1 = rng.uniform(0.2, 1.2, (E, D)).astype(np.float32), rng.uniform(0.3, 0.9, (E, D)).astype(np.float32)
            ql = rng.uniform(-1.0, 0.0, (E, D)).astype(np.float32)
            mk = lambda kind, p0, p1, **kw: _Spec(oracle, dev, kind, p0, p1, D=D, n_edges=E, **kw)
            for name, sp in (("normal_log", mk("normal", q0, ql, p1_log=True)), ("uniform", mk("uniform", q0, q0 + q1))):
                for scaled in (True, False):
                    ss_n, ds_n = (gsn, rs) if scaled else (None, None)
                    refs = [oracle.agg_fwd(ogt, gn, sp.o(), src_scale=ss_n, dst_scale=ds_n)]
                    gg = gn * gsn[:, None] if scaled else gn
                    refs += [oracle.agg_bwd_w(og, x, gg, src_scale=ds_n, spec=sp.o(deriv=dv)) for dv in (1, 2)]
                    refs = [(r, G._sc(r)) for r in refs]
                    for seg in SEGS:
                        got = [list(ops._agg_bwd_pedge_raw(v, t, xd, D, sp.c, gs if scaled else None, rsd if scaled else None, seg))
                               for v, t, gs in ((views[0], gt, gst), (views[1], gp, gsp))]
                        check(f"stag_agg_bwd_pedge {name} D={D} scaled={scaled} seg_len={seg}", got[0], got[1], refs)
    assert not check.errs, "\n".join(check.errs)


def test_agg_bwd_pedge_tables_past_2_24_ids(dev, oracle):
    """D = 4 on the per-edge graph: the [E, 4] parameter tables are read, and both gradient tables written, at permuted edge
    ids on both sides of 2^24.  dx and the gradient rows of the checked rows' edges against the oracle; d p0 at EVERY edge
    id against x[u] g[v] formed on the device (a Normal's weight is p0 + exp(p1) z, so d w / d p0 = 1: a gradient row
    written to another edge's id shows there); dx of every row against stag_agg_fwd_mc_pedge's single sample on the same
    view, whose bits it is documented to give (tests/test_gpu_bwd_pedge.py) and which the address-form suite covers."""
    from stag_amd import _lib, ops
    E, D = PE_EDGES, 4
    view, indptr_h, rows = G._pe_graph(dev)
    og, pos, ids = G._pe_compact(oracle, view, indptr_h, rows)
    rows_d, ids_d = torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev)
    assert (ids >= K24).sum() >= 8 and (ids < K24).sum() >= 8
    g = torch.randn(PE_N_SRC, D, device=dev)                   # the gathered table
    x = torch.randn(PE_N_DST, D, device=dev)                   # the rows the units own
    q0, q1 = 0.2 + torch.rand(E, D, device=dev), -torch.rand(E, D, device=dev)
    s = _lib.NoiseSpec()
    s.kind, s.param_mode, s.p0, s.p1, s.seed, s.offset, s.p1_log = (_lib.NOISE_NORMAL, _lib.PARAM_PER_EDGE, _lib.ptr(q0),
                                                                    _lib.ptr(q1), G.SEED, G.OFFSET, 1)
    dx, d0, d1 = ops._agg_bwd_pedge_raw(view, g, x, D, s, None, None, PE_SEG)
    gather = lambda t: t[ids_d].cpu().numpy()
    gn, xn = g.cpu().numpy(), x[rows_d].cpu().numpy()
    ospec = lambda deriv: oracle.make_spec("normal", gather(q0), gather(q1), seed=G.SEED, offset=G.OFFSET, Dn=D,
                                           n_edges=len(ids), p1_log=True, deriv=deriv)
    with hw_normals(oracle, dev):
        ref, ab = G._oracle_cond(oracle, og, gn, None, None, spec=ospec(0))
        assert_close_cond(dx[rows_d], ref, ab, what="stag_agg_bwd_pedge dx, checked rows")
        # the oracle's per-edge gradients want the transpose of the checked rows (as test_per_edge_tables_past_2_24_ids)
        u = np.repeat(np.arange(len(rows)), np.diff(og.indptr))
        ip, ix, eid_f, _, _ = oracle.csr_build(u, og.indices, len(rows), PE_N_SRC)
        ogf = oracle.CsrGraph(ip, ix, eid=eid_f, nidx=og.nidx[eid_f], n_src=len(rows))
        for dv, got in ((1, d0), (2, d1)):
            r = oracle.agg_bwd_w(ogf, xn, gn, spec=ospec(dv)).astype(np.float64)
            sc = G._sc(r)
            assert_close(got[ids_d] / sc, r / sc, what=f"stag_agg_bwd_pedge d p{dv - 1}, checked rows' edge ids")
    # d p0 at every edge id
    u_of = torch.repeat_interleave(torch.arange(PE_N_DST, device=dev), view.degrees.long())
    want = torch.empty(E, D, dtype=torch.float64, device=dev)
    want[view.eid.long()] = x[u_of].double() * g[view.indices.long()].double()
    sc = max(1.0, float(want.abs().max()))
    worst = float(((d0.double() - want).abs() / sc / (1.0 + want.abs() / sc)).max())
    assert worst <= TOL, f"stag_agg_bwd_pedge d p0 at every edge id: scaled error {worst:.3e}"
    del want, u_of
    mc = ops._agg_fwd_mc_pedge_raw(view, g, G._Noise(s), 1, 1, _lib.REDUCE_SUM, None, None, PE_SEG)
    assert torch.equal(dx, mc[0]), "dx is not stag_agg_fwd_mc_pedge's single sample on the same view"


# ---- the fp32 GAT family: narrow_extent (csrc/gat.hip) fills ft_bytes and g_bytes ----------------------------------------------
# GAT rows are contiguous, so there is no form (b).  (a) rows past 2^24 at 16 bytes a row, (c) an extent past 2^32 bytes with
# 2^20 + 3 rows of 4096 bytes — H F = 1024: only the cooperative kernels have a shape for it — and (d) the top of the narrow
# form, 2^24 - 1 rows of 256 bytes.  The graph is square, so el, er, ft, G, out and every gradient have n rows: the
# destinations sit at the top and the bottom of the node range too, which is what g_bytes (the backward's gather of G by
# destination) needs.
GAT_FORMS = {
    "a": dict(n=K24 + 5, H=1, F=4, nodes=[0, 5, K24 - 1, K24, K24 + 4], wide=True),
    "c": dict(n=(1 << 20) + 3, H=4, F=256, wide=True,
              nodes=[0, (1 << 19) - 1, 1 << 19, (1 << 20) - 1, 1 << 20, (1 << 20) + 2]),
    "d": dict(n=K24 - 1, H=4, F=16, nodes=[0, (1 << 23) - 1, 1 << 23, K24 - 2], wide=False),
}
GAT_SEG = 16
GAT_SLOPE = 0.2
GAT_MC_S, GAT_MC_STRIDE = 5, 2          # a pass of four samples and one of one


def _gat_graphs(oracle, f, form, dev):
    """(the graph on n nodes, the same edges on the m gathered nodes relabelled in order, the oracle's view of the latter):
    the four destination rows of tests/test_gpu_address_forms.py at the nodes [top, middle, next to the top, 0]."""
    import stag_amd
    from util import oracle_graph
    nodes = np.asarray(f["nodes"], np.int64)
    m = len(nodes)
    _, ogt = G._structure(oracle, m, seed=ord(form))
    dn = np.array([m - 1, 2, m - 2, 0])                       # destination row j sits at nodes[dn[j]]
    src_i, dst_i = np.empty(N_EDGES, np.int64), np.empty(N_EDGES, np.int64)
    src_i[ogt.eid], dst_i[ogt.eid] = ogt.indices, dn[ogt.dst_of_pos]
    big = stag_amd.Graph(torch.from_numpy(nodes[src_i]), torch.from_numpy(nodes[dst_i]), f["n"], device=dev)
    small = stag_amd.Graph(torch.from_numpy(src_i), torch.from_numpy(dst_i), m, device=dev)
    for g in (big, small):
        for v in (g.csr, g.csr_t):
            plan = v.plan(GAT_SEG, need=True)
            plan["xcd_decided"] = True                         # plan order on both layouts, whatever the policy would do later
            assert not plan.get("xcd_on")
        assert g.csr.plan(GAT_SEG)["n_long"] == 1 and g.csr.plan(GAT_SEG)["n_seg"] == 3, "the hub is cut into three segments"
    assert torch.equal(big.csr.eid, small.csr.eid) and torch.equal(big.csr_t.eid, small.csr_t.eid), "the same walk order"
    return big, small, oracle_graph(oracle, small)


def _gat_fwd(g, el, er, ft, H, F, spec, dev, blocks=True):
    """One stag_gat_fwd on the plan of GAT_SEG: (out, stats).  blocks = False: the plan without its unit batches, which
    takes gat_fwd_kernel, one unit per team."""
    import ctypes as C
    from stag_amd import _lib, ops
    csrv = g.csr
    plan_t = csrv.plan(GAT_SEG, need=True)
    out = torch.full((csrv.n_dst, H, F), float("nan"), device=dev)
    stats = torch.full((csrv.n_dst, 2 * H), float("nan"), device=dev)
    if blocks:
        ops._gat_fwd_into(csrv, plan_t, el, er, ft, H, F, GAT_SLOPE, spec, None, None, out, stats, dev)
        return out, stats
    nbytes = _lib.lib().stag_gat_workspace_bytes(plan_t["n_seg"], H, F)
    shared, _keep = ops._plan_struct(csrv, GAT_SEG, 1, nbytes, dev, plan_t=plan_t)
    plan_c = _lib.Plan.from_buffer_copy(shared)
    plan_c.block_ptr, plan_c.n_blocks = None, 0
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_gat_fwd(C.byref(cs), C.byref(plan_c), _lib.ptr(el), _lib.ptr(er), _lib.ptr(ft), H, F, GAT_SLOPE,
                                     C.byref(spec), None, None, _lib.ptr(out), _lib.ptr(stats), _lib.stream_of(dev))
    _lib.check(rc, "stag_gat_fwd without unit batches")
    return out, stats


@pytest.mark.parametrize("form", list(GAT_FORMS))
def test_gat_fp32_family_in_each_form(dev, oracle, monkeypatch, form):
    """stag_gat_fwd in its cooperative form and (forms a and d: H F <= 256) in its one-unit-per-team form, stag_gat_fwd_mc
    (S = 5), stag_gat_bwd (one gather) and stag_gat_bwd_two_pass, under Normal(1, 0.5) noise at seg_len 16 (the hub in three
    segments).  Forward: oracle.gat_fwd on the relabelled graph at util.TOL, and the bits of the launch on the packed
    layout (a row's walk does not depend on the other rows of the plan).  Backward: util.assert_gat_grads_vs_oracle, rows
    that no edge touches stay zero, and the bits of the packed launch for d el, d er and d ft (the source pass walks the
    same rows in the same order on both layouts; the [E, H] scratch of d s is indexed by nidx, which is the same
    permutation)."""
    from stag_amd import ops
    from util import assert_gat_grads_vs_oracle
    f = GAT_FORMS[form]
    n, H, F = f["n"], f["H"], f["F"]
    assert ops.gat_cooperative_shape(H, F, GAT_SEG)
    big, small, og = _gat_graphs(oracle, f, form, dev)
    idx = torch.tensor(f["nodes"], device=dev)
    el, er = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev)
    ft, Gt = torch.randn(n, H, F, device=dev), torch.randn(n, H, F, device=dev)
    pk = [t[idx].contiguous() for t in (el, er, ft, Gt)]
    eln, ern, ftn, Gn = (t.cpu().numpy() for t in pk)
    sp = _Spec(oracle, dev, "normal", 1.0, 0.5, D=H, n_edges=N_EDGES)
    errs = []

    def compare(what, got_t, got_p, ref):
        if not torch.equal(got_t[idx], got_p):
            errs.append(f"form ({form}) {what}: not the bits of the packed layout")
        try:
            assert_close(got_t[idx], ref, what=f"form ({form}) {what}")
        except AssertionError as e:
            errs.append(str(e))
        rest = torch.ones(n, dtype=torch.bool, device=dev)
        rest[idx] = False
        if torch.count_nonzero(torch.nan_to_num(got_t[rest], nan=1.0)):
            errs.append(f"form ({form}) {what}: rows without an edge are not zero")

    with hw_normals(oracle, dev):
        ref = oracle.gat_fwd(og, eln, ern, ftn, GAT_SLOPE, sp.o())
        refs_mc = [oracle.gat_fwd(og, eln, ern, ftn, GAT_SLOPE, sp.o(offset=G.OFFSET + s * GAT_MC_STRIDE)) for s in range(GAT_MC_S)]
    # ---- forward -----------------------------------------------------------------------------------------------------------
    out_t, stats_t = _gat_fwd(big, el, er, ft, H, F, sp.c, dev)
    out_p, stats_p = _gat_fwd(small, *pk[:3], H, F, sp.c, dev)
    compare("stag_gat_fwd, cooperative", out_t, out_p, ref)
    if H * F <= 256:
        one_t, _ = _gat_fwd(big, el, er, ft, H, F, sp.c, dev, blocks=False)
        one_p, _ = _gat_fwd(small, *pk[:3], H, F, sp.c, dev, blocks=False)
        compare("stag_gat_fwd, one unit per team", one_t, one_p, ref)
        del one_t
    mc_t, _ = ops._gat_fwd_mc_raw(big.csr, el, er, ft, G._Noise(sp.c), GAT_MC_S, GAT_MC_STRIDE, GAT_SLOPE, GAT_SEG, False)
    mc_p, _ = ops._gat_fwd_mc_raw(small.csr, *pk[:3], G._Noise(sp.c), GAT_MC_S, GAT_MC_STRIDE, GAT_SLOPE, GAT_SEG, False)
    for s in range(GAT_MC_S):
        compare(f"stag_gat_fwd_mc sample {s}", mc_t[s], mc_p[s], refs_mc[s])
    del mc_t
    # ---- backward ----------------------------------------------------------------------------------------------------------
    monkeypatch.setattr(ops, "_GAT_BWD_FUSED", True)
    for name, one_gather in (("stag_gat_bwd", True), ("stag_gat_bwd_two_pass", False)):
        monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", one_gather)
        r_t = ops._gat_bwd_fused(big.csr, big.csr_t, el, er, ft, stats_t, Gt, out_t, H, F, GAT_SLOPE, sp.c, None, False, GAT_SEG, dev)
        r_p = ops._gat_bwd_fused(small.csr, small.csr_t, *pk[:3], stats_p, pk[3], out_p, H, F, GAT_SLOPE, sp.c, None, False,
                                 GAT_SEG, dev)
        assert r_t is not None and r_p is not None, f"{name} has a form for ({H}, {F})"
        rest = torch.ones(n, dtype=torch.bool, device=dev)
        rest[idx] = False
        for a, b, nm in zip(r_t[:3], r_p[:3], ("d el", "d er", "d ft")):
            if not torch.equal(a[idx], b):
                errs.append(f"form ({form}) {name} {nm}: not the bits of the packed layout")
            if torch.count_nonzero(torch.nan_to_num(a[rest], nan=1.0)):
                errs.append(f"form ({form}) {name} {nm}: rows without an edge are not zero")
        try:
            assert_gat_grads_vs_oracle(oracle, og, eln, ern, ftn, Gn, sp.o(), [a[idx] for a in r_t[:3]],
                                       what=f"form ({form}) {name}", dev=dev)
        except AssertionError as e:
            errs.append(str(e))
        del r_t
    assert not errs, "\n".join(errs)
