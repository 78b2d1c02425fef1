"""The GAT oracle (oracle.gat_fwd / oracle.gat_bwd) against float64 torch autograd where the softmax's max shift matters:
logits over [-160, 160] planted on hub rows, and leaky-relu slopes other than 0.2.  tests/test_gpu_gat_softmax_range.py
holds the device kernels to the oracle on the same inputs (it imports the builders below); this file pins the oracle
there.  It extends test_oracle_golden.py::test_gat_bwd_oracle_equals_float64_autograd, which knows slope 0.2 and
unit-scale logits only.

Every planted logit is exact in fp32 AND in float64 (multiples of 1/16 below 2^10, el + er and slope * s included), so the
float64 statement sees the very logits the oracle's fp32 product forms and the comparison shows the softmax and its
derivative alone."""
import numpy as np
import pytest

from util import TOL, assert_close

SLOPES = [0.2, 0.0, 0.05, 0.25, 1.0, 1.5]
N_PROFILES = 8


# ---- input builders (numpy only; shared with the GPU file) ----------------------------------------------------------
def hub_coo(n, hubs, seed):
    """(src, dst, hub rows): n nodes of 0-5 random in-edges, rows 5, 8, ... with hubs[i] in-edges from DISTINCT sources
    (so that a profile can be planted through el), the edge order permuted."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 6, n)
    rows = [5 + 3 * i for i in range(len(hubs))]
    deg[rows] = hubs
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, len(dst))
    ptr = np.concatenate([[0], np.cumsum(deg)])
    for r in rows:
        src[ptr[r]:ptr[r + 1]] = rng.permutation(n)[:deg[r]]
    perm = rng.permutation(len(dst))
    return src[perm].astype(np.int64), dst[perm].astype(np.int64), rows


def profile(idx, deg, rng):
    """Logits of a hub row by CSR position k, profile idx in 1..8 (the issue's table); multiples of 1/16 in [-160, 160]."""
    k = np.arange(deg)
    if idx == 1:
        return -128.0 + k / 16.0                      # ascending: every batch and segment brings a new maximum
    if idx == 2:
        return 128.0 - k / 16.0                       # descending: the first batch holds the maximum
    if idx == 3:
        v = -150.0 + (k % 7) / 8.0                    # one peak in the middle: the row is one-hot
        v[deg // 2] = 150.0
        return v
    if idx == 4:
        return -150.0 + (k % 64) / 16.0               # all low: an unshifted exp underflows, l = 0
    if idx == 5:
        return 150.0 - (k % 64) / 16.0                # all high: an unshifted exp overflows
    if idx == 6:
        return np.full(deg, 100.0)                    # plateau: attention exactly uniform
    if idx == 7:
        return np.where(k % 16 == 0, 120.0, -120.0)   # every segment of 16 holds the maximum
    if idx == 8:
        return rng.integers(-160, 161, deg).astype(np.float64)
    raise KeyError(idx)


def head_profiles(H, rot=0):
    """Profile of each head, cycling from 1 + rot (shapes of fewer than 8 heads run rot = 0 and rot = 4)."""
    return [1 + (rot + h) % N_PROFILES for h in range(H)]


def plant_w(indptr, eid, rows, H, seed, rot=0):
    """Explicit weights [E, H] by edge id for el = er = 0.5 (s = 1, lr = 1: the logit IS w): head h of every hub row
    carries head_profiles(H, rot)[h] by CSR position, every other edge a random multiple of 1/16 in [-160, 160]."""
    rng = np.random.default_rng(seed)
    E = len(eid)
    w = rng.integers(-2560, 2561, (E, H)) / 16.0
    for r in rows:
        b, e = int(indptr[r]), int(indptr[r + 1])
        for h, idx in enumerate(head_profiles(H, rot)):
            w[eid[b:e], h] = profile(idx, e - b, rng)
    return w.astype(np.float32)


EL_PROFILES = (1, 2, 4, 5)


def plant_elr(indptr, indices, rows, n, H, slope, seed):
    """(el, er) multiples of 1/8 for kind 'none' at a slope that is a power of two (0.25, 0.5): the FIRST hub row's
    logits leaky_relu(el[u] + er[v]) follow profiles 1, 2, 4, 5 (cycling over the heads) by CSR position — its sources
    are distinct nodes, s = logit where that is positive and logit / slope where not, |s| up to 640.  Every other row
    (the second hub, whose sources were given their el by the first) sees exact logits of the same range in another
    order."""
    rng = np.random.default_rng(seed)
    el = rng.integers(-320, 321, (n, H)) / 8.0
    er = rng.integers(-320, 321, (n, H)) / 8.0
    r = rows[0]
    b, e = int(indptr[r]), int(indptr[r + 1])
    u = indices[b:e]
    assert len(np.unique(u)) == e - b
    for h in range(H):
        lg = profile(EL_PROFILES[h % 4], e - b, rng)
        s = np.where(lg > 0, lg, lg / slope)
        el[u, h] = s - er[r, h]
    el, er = el.astype(np.float32), er.astype(np.float32)
    s = el[u].astype(np.float64) + er[r].astype(np.float64)
    assert np.array_equal((el[u] + er[r]).astype(np.float64), s), "el + er is exact in fp32"
    return el, er


def plant_ties(n, H, seed):
    """(el, er) with el[u] = -er[v] exactly on the edges out of a third of the nodes (er is one value per head), so
    s == 0 there: the derivative of the leaky relu takes the slope branch (s > 0 ? 1 : slope), as torch has it."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 40, H) / 8.0
    er = np.broadcast_to(c, (n, H)).astype(np.float32).copy()
    el = (rng.integers(-64, 65, (n, H)) / 8.0).astype(np.float32)
    tied = np.arange(n) % 3 == 0
    el[tied] = -er[tied]
    return el, er


def torch_gat(src, dst, n, el, er, ft, w, slope, G=None):
    """float64 torch statement of stag/zoo/gat.py:114-126: (out, attn [E, H] by edge id) and, given d out = G, the
    gradients (d el, d er, d ft, d w | None) by autograd."""
    import torch
    S, D = torch.from_numpy(np.asarray(src)).long(), torch.from_numpy(np.asarray(dst)).long()
    tl, tr, tf = (torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=G is not None) for a in (el, er, ft))
    tw = None if w is None else torch.tensor(np.asarray(w), dtype=torch.float64, requires_grad=G is not None)
    H = tl.shape[1]
    e = torch.nn.functional.leaky_relu(tl[S] + tr[D], slope)
    if tw is not None:
        e = tw * e
    mx = torch.full((n, H), -float("inf"), dtype=torch.float64).scatter_reduce(0, D[:, None].expand(-1, H), e.detach(), "amax")
    ex = torch.exp(e - mx[D])
    a = ex / torch.zeros((n, H), dtype=torch.float64).index_add_(0, D, ex)[D]
    out = torch.zeros((n,) + tuple(tf.shape[1:]), dtype=torch.float64).index_add_(0, D, a[:, :, None] * tf[S])
    if G is None:
        return out.numpy(), a.numpy()
    out.backward(torch.tensor(np.asarray(G), dtype=torch.float64))
    return (out.detach().numpy(), a.detach().numpy(), tl.grad.numpy(), tr.grad.numpy(), tf.grad.numpy(),
            None if tw is None else tw.grad.numpy())


# ---- the oracle against float64 autograd -----------------------------------------------------------------------------
N, HUBS, H, F = 700, [600, 120], 8, 8
_CACHE = {}


def _graph(oracle):
    if "g" not in _CACHE:
        src, dst, rows = hub_coo(N, HUBS, seed=3)
        indptr, indices, eid, *_ = oracle.csr_build(src, dst, N, N)
        rng = np.random.default_rng(4)
        ft = rng.standard_normal((N, H, F)).astype(np.float32)
        G = rng.standard_normal((N, H, F)).astype(np.float32)
        _CACHE["g"] = (oracle.CsrGraph(indptr, indices, eid, n_src=N), src, dst, rows, ft, G)
    return _CACHE["g"]


def _check(oracle, name, slope, el, er, w):
    g, src, dst, rows, ft, G = _graph(oracle)
    spec = oracle.make_spec("none") if w is None else oracle.make_spec("explicit", w)
    out, attn, d_el, d_er, d_ft, dw = torch_gat(src, dst, N, el, er, ft, w, slope, G)
    got, got_attn = oracle.gat_fwd(g, el, er, ft, slope, spec, want_attn=True)
    assert np.isfinite(got).all() and np.isfinite(got_attn).all(), name
    assert_close(got, out, what=f"{name} slope={slope} out")
    assert_close(got_attn, attn, what=f"{name} slope={slope} attn")
    o_el, o_er, o_ft, o_dw = oracle.gat_bwd(g, el, er, ft, G, slope, spec, want_dw=w is not None)
    for a, b, nm in ((o_el, d_el, "d el"), (o_er, d_er, "d er"), (o_ft, d_ft, "d ft")) + (((o_dw, dw, "d w"),) if w is not None else ()):
        assert np.isfinite(a).all(), f"{name} {nm}"
        assert_close(a, b, what=f"{name} slope={slope} {nm}")
    return got, got_attn, d_el, d_er


@pytest.mark.parametrize("slope", SLOPES)
def test_oracle_planted_weights(oracle, slope):
    """All eight profiles through explicit weights (el = er = 0.5: the logit is w bit for bit, whatever the slope)."""
    g, src, dst, rows, ft, G = _graph(oracle)
    w = plant_w(g.indptr, g.eid, rows, H, seed=7)
    half = np.full((N, H), 0.5, np.float32)
    out, attn, *_ = _check(oracle, "planted w", slope, half, half, w)
    # what the profiles promise, on the oracle itself: the one-hot row (profile 3, head 2) is its peak's ft row, the
    # plateau (profile 6, head 5) is uniform
    for r in rows:
        b, e = int(g.indptr[r]), int(g.indptr[r + 1])
        assert_close(out[r, 2], ft[g.indices[b + (e - b) // 2], 2], what="one-hot row")
        assert_close(attn[g.eid[b:e], 5] * (e - b), np.ones(e - b), what="plateau")


@pytest.mark.parametrize("slope", [0.25, 0.5])
def test_oracle_planted_el_er(oracle, slope):
    """Profiles 1, 2, 4, 5 through el / er without weights: here the slope forms the negative logits (down to -160)."""
    g, src, dst, rows, ft, G = _graph(oracle)
    el, er = plant_elr(g.indptr, g.indices, rows, N, H, slope, seed=9)
    _check(oracle, "planted el/er", slope, el, er, None)


@pytest.mark.parametrize("slope", SLOPES)
def test_oracle_ties_take_the_slope_branch(oracle, slope):
    """s == 0 on a third of the edges: d leaky_relu / d s is the slope there (torch's convention and the oracle's), which
    d el / d er show at every slope but 1."""
    g, src, dst, rows, ft, G = _graph(oracle)
    el, er = plant_ties(N, H, seed=13)
    s = el[src] + er[dst]
    assert 0.25 < float((s == 0).mean()) < 0.45
    _, _, d_el, d_er = _check(oracle, "ties", slope, el, er, None)
    if slope != 1.0:        # the case can tell the branches apart: with derivative 1 at s == 0 the gradients differ
        import torch
        S, D = torch.from_numpy(src), torch.from_numpy(dst)
        tl, tr = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (el, er))
        x = tl[S] + tr[D]
        e = torch.where(x >= 0, x, slope * x)
        mx = torch.full((N, H), -float("inf"), dtype=torch.float64).scatter_reduce(0, D[:, None].expand(-1, H), e.detach(), "amax")
        ex = torch.exp(e - mx[D])
        a = ex / torch.zeros((N, H), dtype=torch.float64).index_add_(0, D, ex)[D]
        out = torch.zeros((N, H, F), dtype=torch.float64).index_add_(0, D, a[:, :, None] * torch.tensor(ft, dtype=torch.float64)[S])
        out.backward(torch.tensor(G, dtype=torch.float64))
        other = tl.grad.numpy()
        assert float(np.max(np.abs(other - d_el) / (1.0 + np.abs(d_el)))) > 100 * TOL
