"""The loss-side kernels away from ordinary numbers (tests/loss_range_cases.py; the fixtures alone are proven without a
GPU by tests/test_loss_range_host.py).  Every comparison is against a float64 reference of the same operation:
  S1  stag_sample_kl with narrow and wide posteriors: s / |loc| from 2^-4 down to 2^-20, s = 20, relu with 41 % / none / all
      of the elements clipped, in every parameter mode, plain and log-scale
  S2  the mixture's logsumexp where its max shift matters: components 40 sigmas away, responsibilities of exactly (1, 0),
      identical components, a -inf logit, spike and slab, K = 8 (sample_kl_kernel8 at capacity)
  S3  everything times 2^-20 and 2^20
  S4  non-finite parameters stay in their own edge / channel
  N   normal_kl_mean past the first trip of its grid stride, log-scales over [-16, 8], posterior at and next to the prior
  M   edge_mlp past the first trip, saturated SiLU, a NaN row of the projected table
  C   stag_contrastive_nll on target with the narrowest scale, log-scales over [-16, 8], NaN in one edge / one node
  P   node_project and head_dot: partial row teams, scalar and vector loads, every column tile, idle lanes, NaN, 2^+-60
Bars: assert_close at TOL element by element; a gradient that carries 1/E or 1/n is multiplied by E or n first."""
import numpy as np
import pytest
import torch

import loss_range_cases as lc
from util import assert_close, assert_close_cond, random_graph

pytestmark = pytest.mark.gpu

D = torch.distributions
F32 = np.float32
SEED, OFFSET = 21, 5


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dev(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


@pytest.fixture(scope="module")
def graph(dev):
    g = random_graph(lc.GRAPH["n"], lc.GRAPH["e"], seed=lc.GRAPH["seed"], hub=lc.GRAPH["hub"], device=dev)
    assert g.number_of_edges() == lc.E_SMALL
    eid = g.csr.eid.cpu().numpy()
    assert not np.array_equal(eid, np.arange(lc.E_SMALL)), "a permuted eid"
    deg = np.diff(g.csr.indptr.cpu().numpy())
    assert deg.max() >= 100 and deg.min() == 0, "a 100-edge row and an empty row"
    return g


_DRAWS = {}


def _draw(g, dn):
    """The standard draw of (graph, Dn) at (SEED, OFFSET) from the device's counters, computed once and left unchanged."""
    import stag_amd
    from stag_amd import _lib
    if dn not in _DRAWS:
        _DRAWS[dn] = stag_amd.EdgeNoise(g, dn, _lib.NOISE_NORMAL, 0.0, 1.0, seed=SEED,
                                        offset=OFFSET).materialize().cpu().numpy()
    return _DRAWS[dn]


def _torch_mix(mix, dev):
    lw, m, s = (_dev(t, dev) for t in mix)
    return D.MixtureSameFamily(D.Categorical(logits=lw, validate_args=False), D.Normal(m, s, validate_args=False),
                               validate_args=False)


def _mix_of(tm):
    """What the kernel reads of a torch mixture: its (normalised) logits, locs and scales."""
    c = tm.component_distribution
    return tuple(t.cpu().numpy() for t in (tm.mixture_distribution.logits, c.loc, c.scale))


def _launch(g, case, p0, p1, tm, dev):
    """(kl [1], d p0, d p1) of one stag_sample_kl launch, through ops.sampled_kl_mean and autograd where the
    parameters are tensors; the value without gradients must be the same bits."""
    import stag_amd
    from stag_amd import _lib, ops
    mode = {"scalar": _lib.PARAM_SCALAR, "per_channel": _lib.PARAM_PER_CHANNEL, "per_edge1": _lib.PARAM_PER_EDGE1}[case.mode]
    if case.mode != "scalar":
        p0, p1 = _dev(p0, dev, True), _dev(p1, dev, True)
    noise = stag_amd.EdgeNoise(g, case.dn, _lib.NOISE_NORMAL, p0, p1, relu=case.relu, seed=SEED, offset=OFFSET,
                               differentiable=True, p1_log=case.log)
    assert noise.param_mode == mode and noise.p1_log == case.log
    assert ops.sampled_kl_why_not(noise, tm) is None
    plain = ops._sample_kl_raw(noise, tm, False)[0]
    if case.mode == "scalar":
        kl, d0, d1 = ops._sample_kl_raw(noise, tm, True)
    else:
        kl = ops.sampled_kl_mean(noise, tm)
        kl.backward()
        d0, d1 = p0.grad, p1.grad
    assert _same(kl.reshape(1), plain), "the value does not depend on the gradients"
    return kl.detach().cpu().numpy().reshape(()), d0.detach().cpu().numpy(), d1.detach().cpu().numpy()


def _run_s(g, case, dev):
    z = _draw(g, case.dn)
    p0, p1 = lc.s_params(case)
    tm = _torch_mix(lc.s_mixture(case), dev)
    if case.relu:
        assert lc.relu_margin_ok(z, p0, p1, case.log), "no element within 2^-18 of the clip, on the device's draw"
    got = _launch(g, case, p0, p1, tm, dev)
    ref = lc.sample_kl_ref(z, p0, p1, case.log, case.relu, _mix_of(tm))
    sc = lc.s_grad_scale(case.mode, lc.E_SMALL)
    what = f"{case.group} {case.name}"
    if case.mode == "per_edge1" and case.log and case.mix in lc.DEVICE_EXP_CASES:
        # the device's exponential of the log-scale, under a prior 1 / s_spike^2 steep (loss_range_cases.DEVICE_EXP_CASES)
        terms = lc.device_exp_terms(z, p0, p1, case.relu, _mix_of(tm), ref)
        for i, nm in enumerate((" kl", " d p0", " d p1")):
            k = sc if i else 1.0
            assert_close_cond(np.asarray(got[i], np.float64).reshape(ref[i].shape) * k, ref[i] * k,
                              terms[i] * k * 2.0 ** 24, what=what + nm)
        return
    assert_close(got[0], ref[0], what=what + " kl")
    assert_close(got[1].reshape(ref[1].shape).astype(np.float64) * sc, ref[1] * sc, what=what + " d p0")
    assert_close(got[2].reshape(ref[2].shape).astype(np.float64) * sc, ref[2] * sc, what=what + " d p1")
    if case.mix in lc.S_TWINS:        # (b): the dominant component alone gives the gradients; (c): the one component all
        key, with_value = lc.S_TWINS[case.mix]
        alone = lc.sample_kl_ref(z, p0, p1, case.log, case.relu, lc.scaled_mix(key, case.c))
        if with_value:
            assert_close(got[0], alone[0], what=what + " kl against the one component")
        assert_close(got[1].reshape(ref[1].shape).astype(np.float64) * sc, alone[1] * sc, what=what + " d p0 against one")
        assert_close(got[2].reshape(ref[2].shape).astype(np.float64) * sc, alone[2] * sc, what=what + " d p1 against one")


@pytest.mark.parametrize("group", ["S1", "S2", "S3"])
@pytest.mark.parametrize("mode,log", lc.VARIANTS, ids=lambda v: str(v))
def test_group_S(dev, graph, mode, log, group):
    cases = lc.s_cases(group, mode, log)
    assert cases
    failures = []
    for case in cases:
        try:
            _run_s(graph, case, dev)
        except AssertionError as e:          # every case of the table is reported, not the first
            failures.append(str(e).splitlines()[0])
    assert not failures, "\n".join(failures)


def test_group_S4_per_edge_nonfinite_parameters_stay_in_their_edge(dev, graph):
    import stag_amd
    from stag_amd import _lib, ops
    case = next(c for c in lc.s_cases("S1", "per_edge1", True) if c.s == 2.0 ** -10 and not c.relu and c.dn == 6)
    p0, p1 = lc.s_params(case)
    tm = _torch_mix(lc.s_mixture(case), dev)
    e_nan, e_inf = 7, 211

    def run(a, b):
        noise = stag_amd.EdgeNoise(graph, case.dn, _lib.NOISE_NORMAL, _dev(a, dev), _dev(b, dev), seed=SEED,
                                   offset=OFFSET, p1_log=True)
        return ops._sample_kl_raw(noise, tm, True)

    clean = run(p0, p1)
    a, b = p0.copy(), p1.copy()
    a[e_nan], b[e_inf] = np.nan, np.inf
    got = run(a, b)
    keep = torch.ones(lc.E_SMALL, dtype=torch.bool, device=dev)
    keep[[e_nan, e_inf]] = False
    assert torch.isfinite(clean[0]).all() and torch.isfinite(clean[1]).all() and torch.isfinite(clean[2]).all()
    for i in (1, 2):
        assert _same(got[i][keep], clean[i][keep]), "every other edge is bit-identical"
        assert not torch.isfinite(got[i][~keep]).any(), "the planted edges are non-finite"
    assert not torch.isfinite(got[0]).any()


def test_group_S4_per_channel_nan_stays_in_its_column(dev, graph):
    import stag_amd
    from stag_amd import _lib, ops
    case = next(c for c in lc.s_cases("S1", "per_channel", False) if c.s == 2.0 ** -10 and not c.relu)
    p0, p1 = lc.s_params(case)
    tm = _torch_mix(lc.s_mixture(case), dev)
    k_nan = 13

    def run(a):
        noise = stag_amd.EdgeNoise(graph, case.dn, _lib.NOISE_NORMAL, _dev(a, dev), _dev(p1, dev), seed=SEED, offset=OFFSET)
        return ops._sample_kl_raw(noise, tm, True)

    clean = run(p0)
    a = p0.copy()
    a[k_nan] = np.nan
    got = run(a)
    keep = torch.ones(case.dn, dtype=torch.bool, device=dev)
    keep[k_nan] = False
    for i in (1, 2):
        assert torch.isfinite(clean[i]).all()
        assert _same(got[i][keep], clean[i][keep]), "every other column is bit-identical"
        assert torch.isnan(got[i][~keep]).all()
    assert torch.isnan(got[0]).all()


# ---- N ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_scale", lc.PRIOR_SCALES)
@pytest.mark.parametrize("kind", lc.N_KINDS)
def test_group_N_normal_kl(dev, kind, p_scale):
    from stag_amd import ops
    loc, ls, m2, s2 = lc.n_inputs(kind, p_scale)
    n, u = loc.size, lc.prior_grad_units(s2)
    assert n > lc.STRIDE
    ref = lc.normal_kl_ref(loc, ls, m2, s2)
    what = f"N {kind} prior scale {p_scale}"

    def run(learned):
        a, b = _dev(loc, dev, True), _dev(ls, dev, True)
        pm, ps = (torch.tensor([float(v)], device=dev, requires_grad=learned) for v in (m2, s2))
        kl = ops.normal_kl_mean(a, b, pm, ps)
        kl.backward()
        return kl.detach(), a.grad, b.grad, pm.grad, ps.grad

    got = run(True)
    assert_close(got[0], ref[0], what=what + " kl")
    assert_close(got[1].cpu().numpy().astype(np.float64) * n, ref[1] * n, what=what + " n d loc")
    assert_close(got[2].cpu().numpy().astype(np.float64) * n, ref[2] * n, what=what + " n d log_scale")
    assert_close(got[3].cpu().numpy().astype(np.float64) * u, ref[3].reshape(1) * u, what=what + " s2 d prior loc")
    assert_close(got[4].cpu().numpy().astype(np.float64) * u, ref[4].reshape(1) * u, what=what + " s2 d prior scale")
    fixed = run(False)
    assert fixed[3] is None and fixed[4] is None
    for i in range(3):
        assert _same(fixed[i], got[i]), "a fixed prior returns the same bits"
    if kind == "equal":
        for i, k in ((0, 1.0), (1, n), (2, n), (3, u), (4, u)):
            assert_close(got[i].cpu().numpy().astype(np.float64) * k, np.zeros(got[i].shape), what=what + f" [{i}] is 0")


# ---- M ---------------------------------------------------------------------------------------------------------------------
def _edge_mlp_bwd_raw(g, P, wh, gpar):
    """One stag_edge_mlp_bwd: (d pre [E, hidden], d wh, d bh)."""
    from stag_amd import _lib, ops
    dev = P.device
    hidden, n_par = wh.shape
    src, dst = g._src, g._dst
    E = src.shape[0]
    dpre = torch.empty((E, hidden), dtype=torch.float32, device=dev)
    dwh, dbh = torch.empty_like(wh), torch.empty(n_par, dtype=torch.float32, device=dev)
    ws, nbytes = ops._amort_ws(36, dev)
    with _lib.on_device(dev):
        rc = _lib.lib().stag_edge_mlp_bwd(_lib.ptr(src), _lib.ptr(dst), E, _lib.ptr(P), _lib.ptr(P[:, hidden:]),
                                          P.stride(0), hidden, _lib.ptr(wh), n_par, _lib.ptr(gpar), _lib.ptr(dpre),
                                          _lib.ptr(dwh), _lib.ptr(dbh), _lib.ptr(ws), nbytes, _lib.stream_of(dev))
    _lib.check(rc, "stag_edge_mlp_bwd")
    return dpre, dwh, dbh


@pytest.mark.parametrize("hidden", lc.HIDDENS)
def test_group_M_edge_mlp(dev, hidden):
    import stag_amd
    from stag_amd import ops
    src, dst, P, wh, bh, g = lc.m_inputs(hidden)
    E = src.size
    assert E > lc.STRIDE
    gr = stag_amd.Graph(torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64)), lc.N_NODES, device=dev)
    assert np.array_equal(gr._src.cpu().numpy(), src) and np.array_equal(gr._dst.cpu().numpy(), dst)
    ref = lc.edge_mlp_ref(src, dst, P, wh, bh, g)
    Pd, whd, bhd, gd = (_dev(t, dev) for t in (P, wh, bh, g))

    def run(table):
        with torch.no_grad():
            par = torch.cat(ops.edge_mlp(gr, table, whd, bhd), 1).T.contiguous()
        return (par,) + _edge_mlp_bwd_raw(gr, table, whd, gd)

    clean = run(Pd)
    for t, r, nm in zip(clean, ref, ("par", "d pre", "d wh", "d bh")):
        assert_close(t, r, what=f"M hidden={hidden} {nm}")
    assert torch.isfinite(clean[1][:4]).all() and (clean[1][1] == 0).all() and (clean[1][3] == 0).all(), "no NaN where SiLU saturates"
    # a NaN row of the table: the edges incident to that node, and nothing else
    Pn = Pd.clone()
    Pn[lc.NAN_NODE] = float("nan")
    got = run(Pn)
    hit = torch.from_numpy((src == lc.NAN_NODE) | (dst == lc.NAN_NODE)).to(dev)
    assert 0 < int(hit.sum()) < E // 50
    assert torch.isnan(got[0][:, hit]).all() and torch.isnan(got[1][hit]).all()
    assert _same(got[0][:, ~hit], clean[0][:, ~hit]) and _same(got[1][~hit], clean[1][~hit])
    assert torch.isnan(got[2]).all() and _same(got[3], clean[3]), "d wh sums the NaN activations, d bh reads no table"


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", (1, 3))
@pytest.mark.parametrize("kind", lc.C_KINDS)
def test_group_C_contrastive(dev, kind, hidden):
    from stag_amd import ops
    args = lc.c_inputs(kind, hidden)
    ref = lc.contrastive_ref(*args)
    E = args[0].size
    assert E > lc.STRIDE
    loc, ls, fsrc, fdst, P, wh, bh = (_dev(t, dev) for t in args)

    def run(loc_, P_):
        return ops._contrastive_raw(loc_, ls, fsrc, fdst, P_, hidden, wh, bh, (True,) * 5, lc.POS, lc.NEG)

    clean = run(loc, P)
    for i, nm in enumerate(("nll", "E d loc", "E d log_scale", "E d pre", "d wh", "d bh")):
        k = E if nm.startswith("E ") else 1.0
        assert_close(clean[i].cpu().numpy().astype(np.float64).reshape(ref[i].shape) * k, ref[i] * k, what=f"C {kind} hidden={hidden} {nm}")
    if kind != "wide":
        return
    # a NaN in one edge's loc: its own d loc and d log_scale and the value.  (The head sums and d pre belong to the
    # FAKE edges, which read no loc: they stay bit-identical, as they do in the float64 reference.)
    e0 = lc.STRIDE + 17
    ln = loc.clone()
    ln[e0] = float("nan")
    got = run(ln, P)
    keep = torch.ones(E, dtype=torch.bool, device=dev)
    keep[e0] = False
    assert torch.isnan(got[0]).all() and torch.isnan(got[1][e0]) and torch.isnan(got[2][e0])
    assert _same(got[1][keep], clean[1][keep]) and _same(got[2][keep], clean[2][keep])
    for i in (3, 4, 5):
        assert _same(got[i], clean[i])
    # a NaN row of the table: the value and the head sums are NaN, d pre of the fake edges at that node, nothing else
    Pn = P.clone()
    Pn[lc.NAN_NODE] = float("nan")
    got = run(loc, Pn)
    hit = torch.from_numpy((args[2] == lc.NAN_NODE) | (args[3] == lc.NAN_NODE)).to(dev)
    assert bool(hit[lc.STRIDE:].any()) and bool(hit[:lc.STRIDE].any())
    assert torch.isnan(got[0]).all() and torch.isnan(got[4]).all() and torch.isnan(got[5]).all()
    assert torch.isnan(got[3][hit]).all() and _same(got[3][~hit], clean[3][~hit])
    assert _same(got[1], clean[1]) and _same(got[2], clean[2])


# ---- P ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", lc.P_COLS)
@pytest.mark.parametrize("K", lc.P_KS)
@pytest.mark.parametrize("n", lc.P_ROWS)
def test_group_P_node_project(dev, n, K, C):
    from stag_amd import ops
    x, w, b, gy = lc.p_inputs(n, K, C)
    ref = lc.node_project_ref(x, w, b, gy)

    def run(x_, bias=True):
        xd, wd = _dev(x_, dev, True), _dev(w, dev, True)
        bd = _dev(b, dev, True) if bias else None
        y = ops._NodeProject.apply(xd, wd, bd)
        y.backward(_dev(gy, dev))
        return y.detach(), xd.grad, wd.grad, (bd.grad if bias else None)

    clean = run(x)
    for t, r, nm in zip(clean, ref, ("y", "dx", "dw", "db")):
        assert_close(t, r, what=f"P node_project n={n} K={K} C={C} {nm}")
    r0, k0 = n - 2, K - 2
    xn = x.copy()
    xn[r0, k0] = np.nan
    got = run(xn)
    rows = torch.arange(n, device=dev) != r0
    ks = torch.arange(K, device=dev) != k0
    assert torch.isnan(got[0][r0]).all() and _same(got[0][rows], clean[0][rows])
    assert torch.isnan(got[2][k0]).all() and _same(got[2][ks], clean[2][ks])
    assert _same(got[1], clean[1]) and _same(got[3], clean[3]), "dx and db do not read x"
    base = run(x, bias=False)[0]
    for c in lc.POW2:
        assert _same(run(x * F32(c), bias=False)[0], base * c), "a power of two scales y bit for bit"


@pytest.mark.parametrize("H,F", lc.HD_SHAPES)
@pytest.mark.parametrize("n", lc.P_ROWS)
def test_group_P_head_dot(dev, n, H, F):
    from stag_amd import ops
    ft, al, ar, g = lc.hd_inputs(n, H, F)
    ref = lc.head_dot_ref(ft, al, ar, g)

    def run(ft_):
        fd, ald, ard = _dev(ft_, dev, True), _dev(al, dev, True), _dev(ar, dev, True)
        el, er = ops.head_dot(fd, ald, ard)
        torch.autograd.backward([el, er], [_dev(g[0], dev), _dev(g[1], dev)])
        return el.detach(), er.detach(), fd.grad, ald.grad, ard.grad

    clean = run(ft)
    for t, r, nm in zip(clean, ref, ("el", "er", "d ft", "d attn_l", "d attn_r")):
        assert_close(t, r, what=f"P head_dot n={n} H={H} F={F} {nm}")
    r0, h0, f0 = n - 2, H - 1, F - 3
    fn = ft.copy()
    fn[r0, h0, f0] = np.nan
    got = run(fn)
    keep_y = torch.ones((n, H), dtype=torch.bool, device=dev)
    keep_y[r0, h0] = False
    keep_w = torch.ones((H, F), dtype=torch.bool, device=dev)
    keep_w[h0, f0] = False
    for i in (0, 1):
        assert torch.isnan(got[i][r0, h0]) and _same(got[i][keep_y], clean[i][keep_y])
    for i in (3, 4):
        assert torch.isnan(got[i][h0, f0]) and _same(got[i][keep_w], clean[i][keep_w])
    assert _same(got[2], clean[2]), "d ft does not read ft"
    for c in lc.POW2:
        scaled = run(ft * F32(c))
        assert _same(scaled[0], clean[0] * c) and _same(scaled[1], clean[1] * c)
