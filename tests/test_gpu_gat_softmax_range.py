"""The GAT kernels' shifted softmax where the shift matters.  Every kernel in csrc/gat.hip carries its own copy of it — the
online form (corr = exp(m - mn)), the per-segment (acc, m, l) states and their last-arriver merge, the recomputation
exp(logit - stats_m) / stats_l of stag_gat_attn and of every backward form — and a softmax is shift-invariant: with
unit-scale logits a kernel that subtracts the wrong value (a first batch's maximum, a maximum that missed segments, a
stale m) still gives the right answer.  Here the logits span [-160, 160] (e^150 overflows fp32, e^-150 underflows), so a
wrong shift shows as NaN, as a row of zeros through the (l > 0 ? 1 / l : 0) guard, or as a wrong distribution.

Also pinned here: `stats` ([n_dst, 2H]: the row maximum m, then l = sum exp(logit - m)) against a reference of its own
(every backward form and stag_gat_attn consume it), neg_slope away from 0.2, and hub-row attention relative to the row's
own scale (each value of a 4100-edge row is ~2e-4: the flat bar alone passes one that is 10 % wrong).

Inputs (builders in test_gat_softmax_range_host.py, which pins the oracle on them against float64 autograd): 4300 nodes
of 0-5 in-edges, hub rows of 4100 and 700 in-edges (257 and 44 segments of 16: more than the 192 the partitioned
maximum fetch of the cooperative forward covers per round at (8, 32), and many rounds of its 12-state merge; 65 and 11
segments of 64), edge order permuted.  Three plantings:
  w      explicit weights, el = er = 0.5, so the logit IS w: eight profiles over the heads by CSR position inside the hub
         rows (ascending, descending, one peak, all low, all high, plateau, the maximum in every segment, random);
  elr    no weights, el / er multiples of 1/8 with |s| up to 680 at an exact slope (0.25, 0.5): the slope forms the
         negative logits;
  drawn  Normal(1, 0.5) noise on 40 N(0,1) logits rounded to 1/8, the oracle drawing from the device's tables.
The oracle forms each logit as the same fp32 product the kernels form, so a comparison shows the softmax alone."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_gat_softmax_range_host as host
from util import TOL, assert_close, assert_gat_grads_vs_oracle, hw_normals, oracle_graph

pytestmark = pytest.mark.gpu

N, HUBS = 4300, [4100, 700]
SLOPE_OF = {"w": 0.2, "w4": 0.2, "elr": 0.25, "drawn": 0.2}     # (w: s = 1 > 0 on every edge, the slope is not used)
NOISE = dict(seed=17, offset=3)
_CACHE = {}


# ---- inputs, built once per module -----------------------------------------------------------------------------------
def _graph(dev):
    if "g" not in _CACHE:
        import stag_amd
        src, dst, rows = host.hub_coo(N, HUBS, seed=1)
        g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), N, device=dev)
        c = g.csr
        _CACHE["g"] = dict(g=g, src=src, dst=dst, rows=rows, indptr=c.indptr.cpu().numpy(), indices=c.indices.cpu().numpy(),
                           eid=c.eid.cpu().numpy(), deg=np.bincount(dst, minlength=N))
        for sl, segs in ((16, 257 + 44), (64, 65 + 11)):
            assert c.plan(sl, need=True)["n_seg"] == segs
    return _CACHE["g"]


def _ft(H, F):
    key = ("ft", H, F)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * H + F)
        _CACHE[key] = (rng.standard_normal((N, H, F)).astype(np.float32), rng.standard_normal((N, H, F)).astype(np.float32))
    return _CACHE[key]


def _planting(dev, oracle, name, H, slope=None):
    """dict(el, er [N, H] fp32 numpy, w [E, H] numpy | None, weight: the argument of ops.gat_aggregate, spec: the oracle's,
    slope, hw: the oracle draws from the device's tables)."""
    slope = SLOPE_OF[name] if slope is None else slope
    key = ("p", name, H, slope)
    if key in _CACHE:
        return _CACHE[key]
    import stag_amd
    from stag_amd import _lib
    G_ = _graph(dev)
    E = len(G_["eid"])
    p = dict(name=name, slope=slope, w=None, weight=None, spec=oracle.make_spec("none"), hw=False)
    if name in ("w", "w4"):
        p["el"] = p["er"] = np.full((N, H), 0.5, np.float32)
        p["w"] = host.plant_w(G_["indptr"], G_["eid"], G_["rows"], H, seed=7, rot=4 if name == "w4" else 0)
        p["weight"] = torch.from_numpy(p["w"]).to(dev)
        p["spec"] = oracle.make_spec("explicit", p["w"])
        p["profiles"] = host.head_profiles(H, 4 if name == "w4" else 0)
    elif name == "elr":
        p["el"], p["er"] = host.plant_elr(G_["indptr"], G_["indices"], G_["rows"], N, H, slope, seed=9)
    elif name == "ties":
        p["el"], p["er"] = host.plant_ties(N, H, seed=13)
    elif name in ("drawn", "ordinary"):
        rng = np.random.default_rng(21 + H)
        scale = 40.0 if name == "drawn" else 1.0
        rnd = (lambda a: np.round(a * 8.0) / 8.0) if name == "drawn" else (lambda a: a)
        p["el"] = rnd(scale * rng.standard_normal((N, H))).astype(np.float32)
        p["er"] = rnd(scale * rng.standard_normal((N, H))).astype(np.float32)
        p["weight"] = stag_amd.EdgeNoise(G_["g"], H, _lib.NOISE_NORMAL, 1.0, 0.5, **NOISE)
        p["spec"] = oracle.make_spec("normal", 1.0, 0.5, Dn=H, n_edges=E, **NOISE)
        p["hw"] = True
    else:
        raise KeyError(name)
    p["eld"], p["erd"] = torch.from_numpy(p["el"]).to(dev), torch.from_numpy(p["er"]).to(dev)
    _CACHE[key] = p
    return p


class _tables:
    """hw_normals where the planting draws, nothing where it does not."""

    def __init__(self, oracle, dev, p):
        self.ctx = hw_normals(oracle, dev) if p["hw"] else None

    def __enter__(self):
        if self.ctx:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx:
            self.ctx.__exit__(*exc)
        return False


def _reference(oracle, dev, p, H, F, ft):
    """(out, attn) of the oracle, once per (planting, shape, ft)."""
    key = ("ref", p["name"], p["slope"], H, F, id(ft))
    if key not in _CACHE:
        og = oracle_graph(oracle, _graph(dev)["g"])
        with _tables(oracle, dev, p):
            _CACHE[key] = oracle.gat_fwd(og, p["el"], p["er"], ft, p["slope"], p["spec"], want_attn=True) + (ft,)
    return _CACHE[key][:2]


def _stats_reference(dev, p, w=None):
    """(m [N, H] fp32, l [N, H] float64) from logits formed in numpy float32 exactly as the kernels form them —
    s = el[u] + er[v], lr = s > 0 ? s : slope * s, logit = w * lr, each step rounded to fp32 (the library is built
    with -ffp-contract=off; without weights the kernels multiply by 1.0f, which is exact) — the maximum is exact and
    order-free, l is summed in float64.  w: [E, H] by edge id (drawn weights: noise.materialize(), bit-equal to the
    in-kernel draw)."""
    G_ = _graph(dev)
    u, v = G_["indices"], np.repeat(np.arange(N), np.diff(G_["indptr"]))
    s = p["el"][u] + p["er"][v]
    assert s.dtype == np.float32
    lr = np.where(s > 0, s, np.float32(p["slope"]) * s)
    w = p["w"] if w is None else w
    logit = lr if w is None else (w[G_["eid"]].astype(np.float32) * lr)
    assert logit.dtype == np.float32
    m = np.full((N, p["el"].shape[1]), -np.inf, np.float32)
    np.maximum.at(m, v, logit)
    l = np.zeros(m.shape, np.float64)
    np.add.at(l, v, np.exp(logit.astype(np.float64) - m[v].astype(np.float64)))
    return m, l


def _show(what, err, tol):
    if os.environ.get("STAG_PRINT_ERR"):
        print(f"ERR {what}: {err:.3e} (tol {tol:.1e})")


def _check_stats(dev, p, stats, tol, what, w=None):
    """stats[:, :H] EQUALS the row maximum of the fp32 logits; stats[:, H:] is sum exp(logit - m) within tol, relative;
    rows with in-edges only."""
    H = p["el"].shape[1]
    m, l = _stats_reference(dev, p, w)
    has = _graph(dev)["deg"] > 0
    st = stats.detach().cpu().numpy()
    assert np.isfinite(st[has]).all(), f"{what}: stats not finite"
    assert np.array_equal(st[has, :H], m[has]), (f"{what}: stats m is not the row maximum of the logits "
                                                f"({int((st[has, :H] != m[has]).sum())} of {m[has].size} differ)")
    err = float(np.max(np.abs(st[has, H:] - l[has]) / l[has]))
    _show(f"{what} stats l (relative)", err, tol)
    assert err <= tol, f"{what}: stats l relative error {err:.3e} > {tol:.1e}"


def _check_attn(dev, attn, ref_attn, tol, what):
    """Each row and head of both sides divided by that row's largest reference attention, then the flat bar: the 1e-5
    holds relative to a hub row's own scale."""
    dst = _graph(dev)["dst"]
    attn = attn.detach().cpu().numpy()
    assert np.isfinite(attn).all(), f"{what}: attention not finite"
    top = np.zeros((N, ref_attn.shape[1]), np.float64)
    np.maximum.at(top, dst, ref_attn.astype(np.float64))
    sc = top[dst]
    assert (sc > 0).all()
    assert_close(attn / sc, ref_attn / sc, tol=tol, what=f"{what} attn (row-scaled)")


def _check_profiles(dev, p, out, attn, ft, tol, what):
    """What profiles 3 and 6 promise whatever the reference says: a one-hot row is its peak's ft row, a plateau is
    uniform attention."""
    G_ = _graph(dev)
    out = out.detach().cpu().numpy()
    attn = None if attn is None else attn.detach().cpu().numpy()
    for r in G_["rows"]:
        b, e = int(G_["indptr"][r]), int(G_["indptr"][r + 1])
        for h, idx in enumerate(p.get("profiles", ())):
            if idx == 3:
                assert_close(out[r, h], ft[G_["indices"][b + (e - b) // 2], h], tol=tol, what=f"{what} one-hot row {r} head {h}")
            if idx == 6 and attn is not None:
                assert_close(attn[G_["eid"][b:e], h] * (e - b), np.ones(e - b), tol=tol, what=f"{what} plateau row {r} head {h}")


def _raw_spec(p):
    import stag_amd
    from stag_amd import ops
    if isinstance(p["weight"], stag_amd.EdgeNoise):
        return p["weight"].spec()
    if p["weight"] is not None:
        return ops._targs_or_c(ops._explicit_spec(p["weight"]))
    return ops._targs_or_c(ops._none_spec())


def _fwd_raw(dev, p, ftd, seg_len):
    """(out, stats) of one stag_gat_fwd launch: ops._gat_fwd_into on the plan of seg_len, or — seg_len 0, no plan — the
    entry point as _GatAggregate.forward calls it."""
    from stag_amd import _lib, ops
    csrv = _graph(dev)["g"].csr
    H, F = ftd.shape[1], ftd.shape[2]
    out = torch.full((N, H, F), float("nan"), device=dev)
    stats = torch.full((N, 2 * H), float("nan"), device=dev)
    spec = _raw_spec(p)
    if seg_len:
        ops._gat_fwd_into(csrv, csrv.plan(seg_len, need=True), p["eld"], p["erd"], ftd, H, F, p["slope"], spec, None, None,
                          out, stats, dev)
        return out, stats
    cs = csrv.struct()
    with _lib.on_device(dev):
        rc = _lib.lib().stag_gat_fwd(C.byref(cs), None, _lib.ptr(p["eld"]), _lib.ptr(p["erd"]), _lib.ptr(ftd), H, F,
                                     float(p["slope"]), C.byref(spec), None, None, _lib.ptr(out), _lib.ptr(stats),
                                     _lib.stream_of(dev))
    _lib.check(rc, "stag_gat_fwd")
    return out, stats


def _forward_case(dev, oracle, name, H, F, seg_len, slope=None):
    from stag_amd import ops
    G_ = _graph(dev)
    p = _planting(dev, oracle, name, H, slope)
    ft, _ = _ft(H, F)
    ftd = torch.from_numpy(ft).to(dev)
    ref, ref_attn = _reference(oracle, dev, p, H, F, ft)
    tol = TOL if seg_len else 2 * TOL          # the project's allowance for one unsegmented hub sum
    what = f"{name} slope={p['slope']} H={H} F={F} seg_len={seg_len}"
    with torch.no_grad():
        out, attn = ops.gat_aggregate(G_["g"], p["eld"], p["erd"], ftd, p["slope"], p["weight"], want_attn=True, seg_len=seg_len)
    assert torch.isfinite(out).all(), f"{what}: NaN / Inf in out"
    assert_close(out, ref, tol=tol, what=f"{what} out")
    _check_attn(dev, attn, ref_attn, tol, what)
    _check_profiles(dev, p, out, attn, ft, tol, what)
    if H <= 16 and H * F <= 1024:              # (the composed path keeps no stats)
        out2, stats = _fwd_raw(dev, p, ftd, seg_len)
        assert torch.equal(out2, out), f"{what}: the raw launch and ops.gat_aggregate differ"
        w = p["weight"].materialize().cpu().numpy() if p["hw"] else None
        _check_stats(dev, p, stats, tol, what, w)


def _cases(shapes, seg_lens):
    """(planting, H, F, seg_len): shapes of fewer than 8 heads run the explicit weights twice (profiles 1.. and 5..)."""
    return [(name, H, F, sl) for H, F in shapes for sl in seg_lens for name in ("w", "w4", "elr", "drawn")
            if not (name == "w4" and H >= 8)]


# ---- forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H,F,seg_len", _cases([(8, 32), (4, 16)], [16, 64]))
def test_forward_cooperative_partitioned_max(dev, oracle, name, H, F, seg_len):
    """gat_fwd_block_kernel<fp32, LPE, 1>, one 4-channel chunk per lane and F / 4 a power of two of at most 16 lanes per head:
    the last arriver fetches the row maximum partitioned (a head's lanes take every lph-th segment, 12 states at a
    time; at (8, 32) 192 segments per round, the 4100-edge row has 257 at seg_len 16)."""
    _forward_case(dev, oracle, name, H, F, seg_len)


@pytest.mark.parametrize("name,H,F,seg_len", _cases([(3, 8), (4, 40)], [16]))
def test_forward_cooperative_plain_max(dev, oracle, name, H, F, seg_len):
    """gat_fwd_block_kernel<fp32, LPE, 1> without the partitioned fetch: (3, 8) leaves lanes of the team without a head,
    (4, 40) gives a head 16 lanes for 10 chunks."""
    _forward_case(dev, oracle, name, H, F, seg_len)


@pytest.mark.parametrize("name,H,F,seg_len", _cases([(8, 64), (4, 256)], [16]))
def test_forward_cooperative_wide_rows(dev, oracle, name, H, F, seg_len):
    """gat_fwd_block_kernel<fp32, 64, 2> and <fp32, 64, 4>: 2 and 4 chunks per lane, the merge takes one segment state at a time."""
    _forward_case(dev, oracle, name, H, F, seg_len)


@pytest.mark.parametrize("name,H,F,seg_len", _cases([(3, 7), (4, 5)], [16]))
def test_forward_unit_per_team_scalar(dev, oracle, name, H, F, seg_len):
    """gat_fwd_kernel<LPE, false> (F % 4 != 0: no cooperative form): four softmax states per lane — a lane's channels
    straddle heads — the online corr inside a segment, then the segment merge of the last arriver."""
    _forward_case(dev, oracle, name, H, F, seg_len)


@pytest.mark.parametrize("name,H,F,seg_len", _cases([(8, 32)], [0]))
def test_forward_online_without_a_plan(dev, oracle, name, H, F, seg_len):
    """gat_fwd_kernel<64, true> without a plan: one team walks the 4100 edges in batches of 64, rescaling its state by
    corr = exp(m - mn) at every batch (2 TOL: one unsegmented 4100-term sum)."""
    _forward_case(dev, oracle, name, H, F, seg_len)


@pytest.mark.parametrize("name", ["w", "elr", "drawn"])
def test_forward_composed(dev, oracle, name):
    """(20, 16), H > 16 and H * F > 256: ops._gat_composed — logits and the shifted exp as torch ops (scatter amax), the
    sums on the aggregation kernel.  out and attention (this path has no stats)."""
    _forward_case(dev, oracle, name, 20, 16, 16)


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("H,F", [(8, 32), (8, 64)])
def test_forward_half_rows(dev, oracle, H, F, dname):
    """stag_gat_fwd_half (gat_fwd_block_kernel<bf16 | fp16, ...>, one and two chunks per lane) through ops._gat_fwd_half_raw: the
    oracle on the widened rows, stats against their own reference, and out / stats equal to the fp32 entry's on
    ft.float() bit for bit, as tests/test_gpu_gat_half.py asserts at narrow logits."""
    from stag_amd import ops
    G_ = _graph(dev)
    csrv = G_["g"].csr
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[dname]
    fth = torch.from_numpy(_ft(H, F)[0]).to(dtype)
    key = ("fth", H, F, dname)
    ft = _CACHE.setdefault(key, fth.float().numpy())
    fth = fth.to(dev)
    for name in ("w", "elr", "drawn"):
        p = _planting(dev, oracle, name, H)
        ref, ref_attn = _reference(oracle, dev, p, H, F, ft)
        what = f"half {dname} {name} H={H} F={F}"
        out = torch.full((N, H, F), float("nan"), device=dev)
        stats = torch.full((N, 2 * H), float("nan"), device=dev)
        ops._gat_fwd_half_raw(csrv, csrv.plan(16, need=True), p["eld"], p["erd"], fth, H, F, p["slope"], _raw_spec(p), None,
                              None, out, stats, 16, dev)
        o32, s32 = _fwd_raw(dev, p, fth.float(), 16)
        assert torch.isfinite(out).all(), f"{what}: NaN / Inf in out"
        assert torch.equal(out, o32) and torch.equal(stats, s32), f"{what}: not the fp32 entry's bits"
        assert_close(out, ref, what=f"{what} out")
        _check_stats(dev, p, stats, TOL, what, p["weight"].materialize().cpu().numpy() if p["hw"] else None)
        with torch.no_grad():
            out2, attn = ops.gat_aggregate(G_["g"], p["eld"], p["erd"], fth, p["slope"], p["weight"], want_attn=True, seg_len=16)
        assert torch.equal(out2, out)
        _check_attn(dev, attn, ref_attn, TOL, what)
        _check_profiles(dev, p, out, attn, ft, TOL, what)


def test_forward_monte_carlo(dev, oracle):
    """stag_gat_fwd_mc (gat_fwd_mc_block_kernel) at (8, 32), 3 samples of Normal noise from one row gather: sample s is the
    oracle at offset + s; stats per sample against the materialised draw of that offset."""
    from stag_amd import ops
    G_ = _graph(dev)
    H, F, S = 8, 32, 3
    p = _planting(dev, oracle, "drawn", H)
    ft, _ = _ft(H, F)
    ftd = torch.from_numpy(ft).to(dev)
    og = oracle_graph(oracle, G_["g"])
    E = len(G_["eid"])
    out, stats = ops._gat_fwd_mc_raw(G_["g"].csr, p["eld"], p["erd"], ftd, p["weight"], S, 1, p["slope"], 16, want_stats=True)
    assert out.shape == (S, N, H, F) and stats.shape == (S, N, 2 * H) and torch.isfinite(out).all()
    for s in range(S):
        spec = oracle.make_spec("normal", 1.0, 0.5, Dn=H, n_edges=E, seed=NOISE["seed"], offset=NOISE["offset"] + s)
        with hw_normals(oracle, dev):
            ref = oracle.gat_fwd(og, p["el"], p["er"], ft, p["slope"], spec)
        assert_close(out[s], ref, what=f"mc sample {s} out")
        nz = copy.copy(p["weight"])
        nz.offset = p["weight"].offset + s
        _check_stats(dev, p, stats[s], TOL, f"mc sample {s}", nz.materialize().cpu().numpy())


# ---- backward ----------------------------------------------------------------------------------------------------------
FORMS = {"one_gather": (True, True), "two_pass": (False, True), "edge": (True, False)}


def _grads_vs_oracle(oracle, dev, p, H, F, got, got_dw, what):
    """util.assert_gat_grads_vs_oracle as it is on the drawn planting: it states the oracle's backward at slope 0.2 and
    scales d el / d er by the largest cancelling term a <G, ft[u]>, which is that term where the derivative factor of the
    logit, c = w lr'(s) (lr' = s > 0 ? 1 : slope), is of order 1.  Elsewhere — another slope, explicit weights up to 160 —
    the same comparison with the slope passed on and c in the term:
        d s[e,h] = c a (<G[v,h], ft[u,h]> - <G[v,h], out[v,h]>),
    two fp32 dot products (the kernels form them in different orders: gat_rowdot_kernel on out, the edge pass on ft[u])
    that cancel exactly on a one-hot row — and with logits over +-160 nearly every row of 1-5 edges is one-hot — each
    carrying c.  The largest cancelling term is therefore |c| a |<G, ft[u]>|; the rounding of either dot, 2^-24 of its
    terms' sum, is multiplied by c = 160 before it reaches d er, where the exact answer is 0.  (With the term without
    c, one-gather d er on the explicit weights: 1.43e-5 at (8, 32), 1.29e-5 at (3, 8), 1.66e-5 at (8, 64) of 1e-5.)"""
    og = oracle_graph(oracle, _graph(dev)["g"])
    ft, G = _ft(H, F)
    if p["name"] == "drawn" and p["slope"] == 0.2:
        assert_gat_grads_vs_oracle(oracle, og, p["el"], p["er"], ft, G, p["spec"], got, got_dw=got_dw, what=what, dev=dev)
        return
    key = ("bwd", p["name"], p["slope"], H, F)
    if key not in _CACHE:
        _, attn = _reference(oracle, dev, p, H, F, ft)
        with _tables(oracle, dev, p):
            ref = oracle.gat_bwd(og, p["el"], p["er"], ft, G, p["slope"], p["spec"], want_dw=p["w"] is not None)
        u, v = og.indices, og.dst_of_pos
        dots = np.einsum("phf,phf->ph", G[v].astype(np.float64), ft[u].astype(np.float64))
        c = np.where(p["el"][u] + p["er"][v] > 0, 1.0, p["slope"])
        w = p["weight"].materialize().cpu().numpy() if p["hw"] else p["w"]
        if w is not None:
            c = c * w[og.eid].astype(np.float64)
        _CACHE[key] = ref + (float(np.abs(c * attn[og.eid].astype(np.float64) * dots).max()),)
    d_el, d_er, d_ft, dw, term = _CACHE[key]
    for g_, r_, nm in zip(got, (d_el, d_er, d_ft), ("d el", "d er", "d ft")):
        assert torch.isfinite(g_).all(), f"{what} {nm}: not finite"
        sc = max(1.0, float(np.abs(r_).max()), term if nm != "d ft" else 0.0)
        assert_close(g_.detach().cpu().numpy() / sc, r_.astype(np.float64) / sc, what=f"{what} {nm} vs oracle")
    if got_dw is not None:
        sc = max(1.0, float(np.abs(dw).max()))
        assert_close(got_dw.detach().cpu().numpy() / sc, dw.astype(np.float64) / sc, what=f"{what} d w vs oracle")


def _backward_case(dev, oracle, monkeypatch, name, H, F, forms, slope=None):
    from stag_amd import ops
    G_ = _graph(dev)
    p = _planting(dev, oracle, name, H, slope)
    ft, G = _ft(H, F)
    Gd = torch.from_numpy(G).to(dev)
    for form in forms:
        monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", FORMS[form][0])
        monkeypatch.setattr(ops, "_GAT_BWD_FUSED", FORMS[form][1])
        t = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (p["el"], p["er"], ft)]
        weight = p["weight"]
        if p["w"] is not None:
            weight = p["weight"].clone().requires_grad_(True)
        out = ops.gat_aggregate(G_["g"], *t, p["slope"], weight, seg_len=16)
        out.backward(Gd)
        what = f"bwd {form} {name} slope={p['slope']} H={H} F={F}"
        for a in t:
            assert torch.isfinite(a.grad).all(), f"{what}: NaN / Inf in a gradient"
        _grads_vs_oracle(oracle, dev, p, H, F, [a.grad for a in t], weight.grad if p["w"] is not None else None, what)
    monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", True)
    monkeypatch.setattr(ops, "_GAT_BWD_FUSED", True)


@pytest.mark.parametrize("name,H,F,seg_len", _cases([(8, 32), (3, 8), (8, 64),
                                                     (1, 16), (4, 16), (8, 16)], [16]))      # 4, 16 and 32 lanes per row
def test_backward_forms(dev, oracle, monkeypatch, name, H, F, seg_len):
    """d el, d er, d ft (and d w of the explicit weights) through the one-gather backward (stag_gat_bwd), the two-pass
    form (stag_gat_bwd_two_pass) and with the fused backward off — stag_gat_bwd_edge plus aggregations at (8, 32) and
    (3, 8); at (8, 64), 512 channels, that switch leaves the composed path's autograd.  Each recomputes the attention as
    exp(logit - stats_m) / stats_l from the forward's statistics."""
    _backward_case(dev, oracle, monkeypatch, name, H, F, list(FORMS))


@pytest.mark.parametrize("pmode", ["scalar", "head"])
@pytest.mark.parametrize("H,F", [(8, 32), (3, 8), (8, 64)])
def test_backward_vi_parameter_gradients(dev, oracle, monkeypatch, H, F, pmode):
    """stag_gat_bwd_dp on the drawn planting (logits over +-200): the finished gradients of loc / scale, scalar and per
    head, as test_gpu_parity.py::test_gat_vi_parameter_gradients_in_the_kernels compares them — the oracle's backward
    with the weights as explicit weights gives dL/dw, dp_i[h] = sum_e dL/dw dw/dp_i with the oracle's own standard draw.
    The explicit weights are the oracle's fp32 draw itself (bit-equal to the kernel's on the device's tables), not
    p0 + p1 z formed in double: at these logits one ulp of w moves an attention value by 1e-5."""
    import stag_amd
    from stag_amd import _lib, ops
    G_ = _graph(dev)
    g = G_["g"]
    E = len(G_["eid"])
    og = oracle_graph(oracle, g)
    p = _planting(dev, oracle, "drawn", H)
    ft, G = _ft(H, F)
    if pmode == "scalar":
        p0h, p1h = np.full(H, 1.0, np.float32), np.full(H, 0.5, np.float32)
        p0 = torch.tensor(1.0, device=dev, requires_grad=True)
        p1 = torch.tensor(0.5, device=dev, requires_grad=True)
    else:
        p0h, p1h = np.linspace(0.8, 1.2, H).astype(np.float32), np.linspace(0.3, 0.6, H).astype(np.float32)
        p0 = torch.tensor(p0h, device=dev, requires_grad=True)
        p1 = torch.tensor(p1h, device=dev, requires_grad=True)
    noise = stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, p0, p1, seed=31, offset=4, differentiable=True)
    monkeypatch.setattr(stag_amd.EdgeNoise, "materialize",
                        lambda self: (_ for _ in ()).throw(AssertionError("an [E, H] tensor was materialised")))
    t = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (p["el"], p["er"], ft)]
    out = ops.gat_aggregate(g, *t, 0.2, noise, seg_len=16)
    out.backward(torch.from_numpy(G).to(dev))
    monkeypatch.undo()
    with hw_normals(oracle, dev):
        std = oracle.noise_materialize(og, oracle.make_spec("normal", 0.0, 1.0, seed=31, offset=4, Dn=H, n_edges=E), H).astype(np.float64)
        wmat = oracle.noise_materialize(og, oracle.make_spec("normal", p0h, p1h, seed=31, offset=4, Dn=H, n_edges=E), H)
    spec = oracle.make_spec("explicit", wmat)
    what = f"vi {pmode} H={H} F={F}"
    assert torch.isfinite(out).all()
    assert_close(out, oracle.gat_fwd(og, p["el"], p["er"], ft, 0.2, spec), what=f"{what} forward")
    d_el, d_er, d_ft, dw = oracle.gat_bwd(og, p["el"], p["er"], ft, G, 0.2, spec, want_dw=True)
    dw = dw.astype(np.float64)
    d0, d1 = dw.sum(0), (dw * std).sum(0)
    if pmode == "scalar":
        d0, d1 = d0.sum(), d1.sum()
    for got, ref, nm in ((p0.grad, d0, "d p0"), (p1.grad, d1, "d p1")):
        ref = np.asarray(ref, np.float64)
        sc = max(1.0, float(np.abs(ref).max()), float(np.abs(dw).max()))
        assert_close(got.cpu().numpy().reshape(ref.shape) / sc, ref / sc, what=f"{what} {nm}")
    for got, ref, nm in ((t[0].grad, d_el, "d el"), (t[1].grad, d_er, "d er"), (t[2].grad, d_ft, "d ft")):
        sc = max(1.0, float(np.abs(ref).max()))
        assert_close(got / sc, ref.astype(np.float64) / sc, what=f"{what} {nm}")


# ---- slopes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.0, 0.05, 1.0, 1.5])
def test_slopes_ordinary_logits(dev, oracle, monkeypatch, slope):
    """neg_slope away from 0.2 on N(0,1) logits with Normal noise: the forward (lr = s > 0 ? s : slope * s) on the
    cooperative kernel (8, 32) and the unit-per-team kernel (3, 7) — out, attention, stats — and the backward
    (sc1 = w (s > 0 ? 1 : slope)) in its one-gather and per-edge forms."""
    for H, F in ((8, 32), (3, 7)):
        _forward_case(dev, oracle, "ordinary", H, F, 16, slope=slope)
    _backward_case(dev, oracle, monkeypatch, "ordinary", 8, 32, ["one_gather", "edge"], slope=slope)


def test_slopes_planted_el_er_at_one_half(dev, oracle, monkeypatch):
    """The el / er planting at the other exact slope, 0.5 (0.25 runs in every case above)."""
    for H, F in ((8, 32), (3, 7)):
        _forward_case(dev, oracle, "elr", H, F, 16, slope=0.5)
    _backward_case(dev, oracle, monkeypatch, "elr", 8, 32, ["one_gather", "edge"], slope=0.5)


@pytest.mark.parametrize("slope", [0.0, 0.05])
def test_slope_branch_at_ties(dev, oracle, monkeypatch, slope):
    """el[u] = -er[v] exactly on a third of the edges: s == 0, where the derivative of the leaky relu is the slope
    (s > 0 ? 1 : slope), as torch and the oracle have it (test_gat_softmax_range_host.py shows that the other branch
    would be told apart)."""
    G_ = _graph(dev)
    p = _planting(dev, oracle, "ties", 8, slope)
    s = p["el"][G_["src"]] + p["er"][G_["dst"]]
    assert 0.25 < float((s == 0).mean()) < 0.45
    _forward_case(dev, oracle, "ties", 8, 32, 16, slope=slope)
    _backward_case(dev, oracle, monkeypatch, "ties", 8, 32, ["one_gather", "edge"], slope=slope)


def test_layer_negative_slope_reaches_the_kernels(dev):
    """zoo.GAT(16, 4, num_heads=3, negative_slope=0.05) with explicit weights against the float64 torch statement of the
    layer (fc, the attention dots, tests/test_gpu_modules.py::_gat_torch_reference's softmax and sum, bias, flatten):
    the forward and the gradient of every parameter, of the input and of the weights."""
    import stag_amd
    G_ = _graph(dev)
    H, F, D = 3, 4, 16
    E = len(G_["eid"])
    rng = np.random.default_rng(77)
    torch.manual_seed(5)
    layer = stag_amd.zoo.GAT(D, F, num_heads=H, negative_slope=0.05).to(dev)
    with torch.no_grad():
        layer.bias.copy_(torch.from_numpy(rng.standard_normal(H * F).astype(np.float32)))
    x = rng.standard_normal((N, D)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, (E, H)).astype(np.float32)
    gout = rng.standard_normal((N, H * F)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    wd = torch.from_numpy(w).to(dev).requires_grad_(True)
    out = layer(G_["g"], xd, edge_weight=wd)
    out.backward(torch.from_numpy(gout).to(dev))
    # float64, CPU
    prm = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.named_parameters()}
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    w64 = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    S, Dt = torch.from_numpy(G_["src"]), torch.from_numpy(G_["dst"])
    ft = (x64 @ prm["fc.weight"].t()).view(N, H, F)
    el, er = (ft * prm["attn_l"]).sum(-1), (ft * prm["attn_r"]).sum(-1)
    e = w64 * torch.nn.functional.leaky_relu(el[S] + er[Dt], 0.05)
    mx = torch.full((N, H), -float("inf"), dtype=torch.float64).scatter_reduce(0, Dt[:, None].expand(-1, H), e.detach(), "amax")
    ex = torch.exp(e - mx[Dt])
    a = ex / torch.zeros((N, H), dtype=torch.float64).index_add_(0, Dt, ex)[Dt]
    ref = (torch.zeros((N, H, F), dtype=torch.float64).index_add_(0, Dt, a[:, :, None] * ft[S]).flatten(1) + prm["bias"])
    ref.backward(torch.tensor(gout, dtype=torch.float64))
    assert_close(out, ref.detach().numpy(), what="layer forward, negative_slope=0.05")
    pairs = [(xd.grad, x64.grad, "d x"), (wd.grad, w64.grad, "d edge_weight")]
    pairs += [(v.grad, prm[k].grad, "d " + k) for k, v in layer.named_parameters()]
    for got, want, nm in pairs:
        want = want.numpy()
        sc = max(1.0, float(np.abs(want).max()))
        assert_close(got.detach().cpu().numpy() / sc, want / sc, what=f"layer {nm}, negative_slope=0.05")
    # and the slope is what made the difference: the same statement at 0.2 is far from the layer's output
    e2 = w64 * torch.nn.functional.leaky_relu(el[S] + er[Dt], 0.2)
    ex2 = torch.exp(e2 - e2.max())
    a2 = ex2 / torch.zeros((N, H), dtype=torch.float64).index_add_(0, Dt, ex2)[Dt]
    other = torch.zeros((N, H, F), dtype=torch.float64).index_add_(0, Dt, a2[:, :, None] * ft[S]).flatten(1) + prm["bias"]
    assert float((other - ref).detach().abs().max()) > 100 * TOL
