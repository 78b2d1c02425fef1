"""The inputs and references of the float-range tests of the wide edge embedding (no tests in here):
tests/test_edge_embed_range_host.py proves them without a GPU, tests/test_gpu_edge_embed_range.py puts them through
stag_edge_embed_fwd / stag_edge_embed_bwd.  Both import this module, as the loss-range group M does with
tests/loss_range_cases.py.

    h[e, k]     = SiLU(pre),                      pre = ps[src[e], k] + pd[dst[e], k] ROUNDED TO fp32
    d_own[r, k] = sum_{p in row r} g[eid[p], k] SiLU'(pre)
    sg = 1 / (1 + exp(-pre)),  SiLU = pre sg,  SiLU' = sg (1 + pre (1 - sg))          (csrc/edge_embed.hip)

THE GRAPH: 120 nodes.  Planted value i of PLANTED sits on four nodes 4 i .. 4 i + 3: an edge 4i -> 4i + 1 with
ps[4i] = v, pd[4i + 1] = 0 (the value comes through the source's row: the own row of d ps, the gathered row of d pd) and an
edge 4i + 2 -> 4i + 3 with ps = 0, pd = v (the other way round).  Each planted destination also takes three edges from
ordinary nodes and each planted source sends three to ordinary nodes, so a saturated term is summed with ordinary ones and
pre-activations near every planted value occur too.  Nodes from FIRST_FREE on carry 900 random edges, multi-edges and self
loops included, and a hub of 150 in-edges (cut into segments under a plan).  Node N - 1 has no edge at all."""
import numpy as np

F32 = np.float32
N = 120
HIDDENS = (5, 16, 260)        # 4 lanes unvectorised | 4 lanes vectorised | 64 lanes, two channel tiles
SEGS = (0, 16)                # without a plan | planned: the hub is cut
PLANTED = (100.0, -100.0, 1000.0, -1000.0,         # saturated (loss-range group M's)
           -87.0, -88.5, -88.75, -104.0,           # around the overflow of expf(-pre) at pre = -88.72 (and of its fp32 square)
           16.0, 17.0, 18.0,                       # where 1 - sg vanishes in fp32
           -1.2785, 0.0)                           # the zero of SiLU', and 0
FIRST_FREE = 4 * len(PLANTED)
HUB = FIRST_FREE + 3
NAN_NODE = FIRST_FREE + 11
N_RANDOM, N_HUB = 900, 150


def silu64(pre):
    """(SiLU, SiLU') of a float64 array without cancellation or overflow: 1 - sg is formed from the exponential, not by
    subtraction, and the exponent is never positive."""
    pre = np.asarray(pre, np.float64)
    e = np.exp(-np.abs(pre))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    sg, one_minus = np.where(pre >= 0, big, small), np.where(pre >= 0, small, big)
    with np.errstate(invalid="ignore"):
        return pre * sg, sg * (1.0 + pre * one_minus)


def silu_formula64(pre):
    """The documented formula as it stands, in float64: what decides where +-inf and NaN come out."""
    pre = np.asarray(pre, np.float64)
    with np.errstate(all="ignore"):
        sg = 1.0 / (1.0 + np.exp(-pre))
        return pre * sg, sg * (1.0 + pre * (1.0 - sg))


def silu32(pre):
    """The same formula in numpy float32 (tests/loss_range_cases.py: _silu32)."""
    import loss_range_cases as lc
    with np.errstate(all="ignore"):
        return lc._silu32(np.asarray(pre, F32))


_CACHE = {}


def edges():
    """(src, dst) int64 by edge id."""
    if "e" not in _CACHE:
        rng = np.random.default_rng(31)
        src, dst = [], []
        for i in range(len(PLANTED)):
            a = 4 * i
            src += [a, a + 2]
            dst += [a + 1, a + 3]
            for b in (a + 1, a + 3):                         # three ordinary in-edges of each planted destination
                src += rng.integers(FIRST_FREE, N - 1, 3).tolist()
                dst += [b] * 3
            for b in (a, a + 2):                             # three ordinary out-edges of each planted source
                src += [b] * 3
                dst += rng.integers(FIRST_FREE, N - 1, 3).tolist()
        src += rng.integers(FIRST_FREE, N - 1, N_RANDOM).tolist() + rng.integers(FIRST_FREE, N - 1, N_HUB).tolist()
        dst += rng.integers(FIRST_FREE, N - 1, N_RANDOM).tolist() + [HUB] * N_HUB
        src, dst = np.array(src, np.int64), np.array(dst, np.int64)
        order = rng.permutation(len(src))                    # edge ids unrelated to how the edges were listed
        _CACHE["e"] = (src[order], dst[order])
    return _CACHE["e"]


def planted_edges():
    """edge ids [len(PLANTED), 2]: the edge whose value comes through ps, the edge whose value comes through pd"""
    src, dst = edges()
    out = np.empty((len(PLANTED), 2), np.int64)
    for i in range(len(PLANTED)):
        for j, a in enumerate((4 * i, 4 * i + 2)):
            (hit,) = np.flatnonzero((src == a) & (dst == a + 1))
            out[i, j] = hit
    return out


def tables(hidden, scale=1.0, g_scale=1.0):
    """ps, pd [N, hidden], g [E, hidden] float32: N(0, 1) times the (power-of-two) scales, the planted rows on top."""
    rng = np.random.default_rng(700 + hidden)
    E = len(edges()[0])
    ps = (rng.standard_normal((N, hidden)) * scale).astype(F32)
    pd = (rng.standard_normal((N, hidden)) * scale).astype(F32)
    g = (rng.standard_normal((E, hidden)) * g_scale).astype(F32)
    if scale == 1.0:
        for i, v in enumerate(PLANTED):
            a = 4 * i
            ps[a], pd[a + 1] = F32(v), F32(0)
            ps[a + 2], pd[a + 3] = F32(0), F32(v)
    return ps, pd, g


def reference(ps, pd, g, silu=silu64):
    """(h, d ps, d pd, sum |terms| of d ps, of d pd) in float64 on the fp32 inputs, pre rounded to fp32 first."""
    src, dst = edges()
    with np.errstate(all="ignore"):
        pre = (ps[src] + pd[dst]).astype(F32).astype(np.float64)
        h, dh = silu(pre)
        term = g.astype(np.float64) * dh
    outs = [h]
    for t in (term, np.abs(term)):
        for idx in (src, dst):
            acc = np.zeros((N, ps.shape[1]), np.float64)
            with np.errstate(all="ignore"):
                np.add.at(acc, idx, t)
            outs.append(acc)
    return outs[0], outs[1], outs[2], outs[3], outs[4]


def reference32(ps, pd, g):
    """The same in float32 throughout, terms added in edge-id order: what a kernel without compensation computes."""
    src, dst = edges()
    with np.errstate(all="ignore"):
        h, dh = silu32(ps[src] + pd[dst])
        term = (g * dh).astype(F32)
        outs = [h]
        for idx in (src, dst):
            acc = np.zeros((N, ps.shape[1]), F32)
            for e in range(len(src)):
                acc[idx[e]] += term[e]
            outs.append(acc)
    return outs
