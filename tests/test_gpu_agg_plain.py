"""agg_plain_kernel (csrc/agg_plain.hpp) — the fused draw-and-aggregate kernel specialised for the plain forward
launch — against the general agg_kernel and against the oracle.

Every launch is made twice through the C ABI (ops.aggregate -> stag_agg_fwd): once as dispatched, once with
STAG_AGG_PLAIN=0 in the environment, which keeps the general kernel (the library reads it at each launch).  The two
results must be equal BIT FOR BIT — the plain kernel walks the same blocks of two edges, folds them in the same order
(compensated above kKahanMinLen = 16 edges), publishes the same segment partials and runs the same two-level combine —
and both hold the suite's flat 1e-5 against the fp64 oracle (tests/util.py).

The graph is the smallest on which that can go wrong: rows of 0, 1, 2, 3 edges (empty rows, odd tails), 16 and 17
(the Kahan threshold from both sides), 64, 65 and 129 (one, two and three segments at seg_len 64) and 700 (11
partials at seg_len 64: more than the 8 a combine keeps in flight; 44 at seg_len 16: more than one group of 16)."""
import importlib

import numpy as np
import pytest
import torch

from util import assert_close, oracle_graph

pytestmark = pytest.mark.gpu

N = 300
DEGREES = [0, 1, 2, 3, 16, 17, 64, 65, 129, 700]
PARAMS = {"normal": (1.0, 0.5), "uniform": (0.2, 1.8), "bernoulli": (0.7, None)}
_CACHE = {}


def _edges(n_extra=0):
    """(src, dst, n): the rows above, then rows of 0-5 edges up to N nodes; n_extra more rows of one edge each."""
    rng = np.random.default_rng(7)
    deg = np.concatenate([DEGREES, rng.integers(0, 6, N - len(DEGREES)), np.ones(n_extra, np.int64)])
    n = len(deg)
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, len(dst))
    perm = rng.permutation(len(dst))        # edge ids are not CSR positions
    return src[perm], dst[perm], n


def _graph(dev, order, n_extra=0):
    """order: 'plan' (the plan's own order), 'xcd' (its XCD-aware order), 'none' (launched with seg_len 0: no plan)."""
    import stag_amd
    key = (order == "xcd", n_extra)
    if key not in _CACHE:
        gm = importlib.import_module("stag_amd.graph")
        old, gm.XCD_ORDER = gm.XCD_ORDER, "1" if order == "xcd" else "0"
        try:
            src, dst, n = _edges(n_extra)
            g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
            for view in (g.csr, g.csr_t):
                for sl in (64, 16):
                    plan = view.plan(sl, need=True)
                    plan["xcd_decided"] = True      # as built here, whatever the library's own policy would do later
                    assert bool(plan.get("xcd_on")) == (order == "xcd")
        finally:
            gm.XCD_ORDER = old
        _CACHE[key] = g
    return _CACHE[key]


def _x(n, D, dev):
    key = ("x", n, D)
    if key not in _CACHE:
        xh = np.random.default_rng(D).standard_normal((n, D)).astype(np.float32)
        _CACHE[key] = (xh, torch.from_numpy(xh).to(dev))
    return _CACHE[key]


def _noise(g, D, kind, **kw):
    import stag_amd
    from stag_amd import _lib
    k = {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM, "bernoulli": _lib.NOISE_BERNOULLI}[kind]
    p0, p1 = kw.pop("params", PARAMS[kind])
    return stag_amd.EdgeNoise(g, D, k, p0, p1, **kw)


def _both(monkeypatch, launch):
    """launch() as dispatched and with the general kernel forced; the two results, which must be the same bits."""
    monkeypatch.delenv("STAG_AGG_PLAIN", raising=False)
    got = launch()
    monkeypatch.setenv("STAG_AGG_PLAIN", "0")
    general = launch()
    monkeypatch.delenv("STAG_AGG_PLAIN")
    torch.cuda.synchronize()
    return got, general


def _check(monkeypatch, oracle, g, D, kind, what, seg_len=64, reduce="sum", transposed=False, src_scale=None, dev=None,
           oracle_kw=None, **nkw):
    from stag_amd import _lib, ops
    n = g.number_of_nodes()
    xh, x = _x(n, D, dev)
    ss = None if src_scale is None else torch.from_numpy(src_scale).to(dev)

    def launch():
        noise = _noise(g, D, kind, **nkw)
        if transposed:
            return ops._agg_raw(g.csr_t, x, D, ops._noise_spec(noise), _lib.REDUCE_SUM, ss, None, seg_len)[0]
        return ops.aggregate(g, x, noise, reduce=reduce, src_scale=ss, seg_len=seg_len)

    got, general = _both(monkeypatch, launch)
    assert torch.equal(got, general), f"{what}: the dispatched launch and the general kernel differ"
    okw = dict(nkw)
    okw.pop("epoch", None)
    p0, p1 = okw.pop("params", PARAMS[kind])
    okw.update(oracle_kw or {})
    p0, p1 = (p.detach().cpu().numpy() if torch.is_tensor(p) else p for p in (p0, p1))
    spec = oracle.make_spec(kind, p0, p1, Dn=D, n_edges=g.number_of_edges(), **okw)
    ref = oracle.agg_fwd(oracle_graph(oracle, g, transposed=transposed), xh, spec,
                         reduce=oracle.REDUCE_MEAN if reduce == "mean" else oracle.REDUCE_SUM, src_scale=src_scale)
    assert_close(got, ref, what=f"{what} vs oracle")
    assert_close(general, ref, what=f"{what} (general kernel) vs oracle")


@pytest.mark.parametrize("order", ["plan", "xcd", "none"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("kind", ["normal", "uniform", "bernoulli"])
@pytest.mark.parametrize("D", [128, 256, 512])      # 32 lanes per row, 64, and two channel tiles of 64
def test_plain_equals_general(dev, oracle, monkeypatch, D, kind, relu, order):
    g = _graph(dev, order)
    _check(monkeypatch, oracle, g, D, kind, f"D={D} {kind} relu={relu} {order}", seg_len=0 if order == "none" else 64,
           dev=dev, relu=relu, seed=11, offset=3)


@pytest.mark.parametrize("kind", ["normal", "uniform", "bernoulli"])
@pytest.mark.parametrize("D", [128, 256])
def test_plain_many_partials_and_mean(dev, oracle, monkeypatch, D, kind):
    """seg_len 16: the 700-edge row is 44 partials (three groups of the two-level combine); the mean reducer."""
    for order in ("plan", "xcd"):
        _check(monkeypatch, oracle, _graph(dev, order), D, kind, f"D={D} {kind} seg_len=16 {order}", seg_len=16,
               reduce="mean", dev=dev, relu=True, seed=5, offset=1)


@pytest.mark.parametrize("kind", ["normal", "uniform", "bernoulli"])
def test_plain_plan_order_at_32_lanes(dev, oracle, monkeypatch, kind):
    """At D = 128 a plan of at most 49152 units with heavy units takes the two-slot SMALL kernel (general code either
    way); 49200 more one-edge rows make this the launch the plan-order plain kernel serves at 32 lanes per row."""
    g = _graph(dev, "plan", n_extra=49200)
    assert g.csr.plan(64, need=True)["n_units"] > 49152
    _check(monkeypatch, oracle, g, 128, kind, f"D=128 {kind} large plan", dev=dev, seed=2, offset=9)


@pytest.mark.parametrize("order", ["plan", "xcd", "none"])
@pytest.mark.parametrize("D", [128, 256])
def test_plain_counter_words(dev, oracle, monkeypatch, D, order):
    """pos_base above 2^32 (the high bits go into counter word 1) with a channel shard's chunk_base, and the device
    epoch: a launch at (offset O, epoch e) draws what the oracle draws at offset O + e."""
    g = _graph(dev, order)
    epoch = torch.tensor([4], dtype=torch.int64, device=dev)
    for kind in ("normal", "bernoulli"):
        _check(monkeypatch, oracle, g, D, kind, f"D={D} {kind} {order} counters", seg_len=0 if order == "none" else 64,
               dev=dev, seed=0x1234567890, offset=2 ** 32 - 2, pos_base=5 * 2 ** 32 + 12345, chunk_base=7, epoch=epoch,
               oracle_kw=dict(offset=2 ** 32 + 2))


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("case", ["src_scale", "in_norm", "transposed", "per_channel", "D+2"])
def test_launches_that_keep_the_general_kernel(dev, oracle, monkeypatch, D, case):
    """One launch per condition that excludes the plain kernel: the result is the general kernel's (same bits with
    and without STAG_AGG_PLAIN=0) and equals the oracle."""
    g = _graph(dev, "xcd")
    rng = np.random.default_rng(D)
    kw = dict(seed=3, offset=8)
    kind = "uniform"
    if case == "src_scale":
        kw["src_scale"] = rng.uniform(0.5, 1.5, g.number_of_nodes()).astype(np.float32)
    elif case == "in_norm":
        kw["in_norm"] = True
    elif case == "transposed":
        kw["transposed"] = True
    elif case == "per_channel":
        lo = torch.from_numpy(rng.uniform(0.1, 0.5, D).astype(np.float32)).to(dev)
        kw["params"] = (lo, lo + 1.0)
    else:
        D += 2
    _check(monkeypatch, oracle, g, D, kind, f"{case} D={D}", dev=dev, **kw)
