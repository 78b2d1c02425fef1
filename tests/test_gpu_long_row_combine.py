"""The long-row combine of agg_unit (csrc/agg_kernel.hpp) spread over teams: a row of more than 16 segments is added
group by group — the team that draws a group's last ticket Kahan-sums its (at most 16) partials and publishes
(group sum, residual); the team that draws the row's last ticket folds the pairs in group order — against the
single-team combine (STAG_COMBINE_GROUPS=0 in the environment, read at each launch) and against the oracle.

Every case: (1) the two paths give the same bits, (2) the result holds the suite's flat 1e-5 against the fp64 oracle
(Normal: on the device's own tables of the hardware functions, tests/util.py::hw_normals, as the other hub-row tests do),
(3) three consecutive launches on one plan give the same bits, (4) every counter tensor of the plan is zero after each
launch, (5) a launch on a second stream gets counters of its own and the same bits.

Small random graphs (2,000 nodes of 0-5 edges) with planted hub rows; at seg_len 16 the hub lengths sit on the group
edges: 256 edges = 16 segments = one group (the unchanged path), 257 = 17 segments (groups of 16 + 1), 513 = 33
segments (3 groups), 4,097 = 257 segments (17 groups: more pairs than one round trip of the fold holds); two and three
hubs in one graph (pair slots and group counters of neighbouring rows); seg_len 64 with a 1,100-edge hub (18 segments)."""
import numpy as np
import pytest
import torch

from util import assert_close, hw_normals, oracle_graph

pytestmark = pytest.mark.gpu

N = 2000
GRAPHS = {"h256": ([256], 16), "h257": ([257], 16), "h513": ([513], 16), "h4097": ([4097], 16),
          "two": ([513, 257], 16), "three": ([4097, 257, 513], 16), "s64": ([1100], 64)}
WIDTHS = [4, 64, 128, 256, 512]     # slotted narrow shape, 16 / 32 / 64 lanes per row, two channel tiles
_CACHE = {}


def _graph(dev, name, n_extra=0, out_hub=0):
    """The named graph; n_extra more rows of one edge each; out_hub: one SOURCE with that many extra out-edges (a hub row
    of the transposed view)."""
    import stag_amd
    key = (name, n_extra, out_hub)
    if key not in _CACHE:
        hubs, seg_len = GRAPHS[name]
        rng = np.random.default_rng(len(name) + sum(hubs))
        deg = np.concatenate([rng.integers(0, 6, N - len(hubs)), np.ones(n_extra, np.int64)])
        deg = np.insert(deg, [5 + 3 * i for i in range(len(hubs))], hubs)     # hub rows among the others
        n = len(deg)
        dst = np.repeat(np.arange(n), deg)
        src = rng.integers(0, n, len(dst))
        if out_hub:
            src = np.concatenate([src, np.full(out_hub, 11)])
            dst = np.concatenate([dst, rng.integers(0, n, out_hub)])
        perm = rng.permutation(len(dst))
        g = stag_amd.Graph(torch.from_numpy(src[perm]), torch.from_numpy(dst[perm]), n, device=dev)
        _CACHE[key] = (g, seg_len)
    return _CACHE[key]


def _x(n, D, dev):
    key = ("x", n, D)
    if key not in _CACHE:
        xh = np.random.default_rng(D).standard_normal((n, D)).astype(np.float32)
        _CACHE[key] = (xh, torch.from_numpy(xh).to(dev))
    return _CACHE[key]


def _noise_and_spec(oracle, g, D, kind, dev, relu=False, seed=11, offset=3):
    """(device noise or None, oracle spec).  'bernoulli': + in-norm, per-channel probabilities with channel 1 never
    drawn (its weight sums are zero: the `cur == 0` branch of the in-norm factor)."""
    import stag_amd
    from stag_amd import _lib
    E = g.number_of_edges()
    if kind == "none":
        return None, oracle.make_spec("none")
    if kind == "normal":
        return (stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, relu=relu, seed=seed, offset=offset),
                oracle.make_spec("normal", 1.0, 0.5, relu=relu, seed=seed, offset=offset, Dn=D, n_edges=E))
    p = np.full(D, 0.7, np.float32)
    p[1] = 0.0
    return (stag_amd.EdgeNoise(g, D, _lib.NOISE_BERNOULLI, torch.from_numpy(p).to(dev), None, in_norm=True, seed=seed,
                               offset=offset),
            oracle.make_spec("bernoulli", p, None, in_norm=True, seed=seed, offset=offset, Dn=D, n_edges=E))


def _counters_zero(plans, what):
    total = 0
    for plan in plans:
        for c in plan["counters"].values():
            total += c.numel()
            assert int(c.abs().max()) == 0, f"{what}: a counter of the plan is left non-zero"
    return total


def _check(monkeypatch, launch, ref, plans, what, dev):
    """launch() -> tensor; ref: the oracle's result; plans: the plan dicts whose counters the launches use."""
    monkeypatch.delenv("STAG_COMBINE_GROUPS", raising=False)
    runs = []
    for _ in range(3):
        runs.append(launch())
        torch.cuda.synchronize()
        assert _counters_zero(plans, what) > 0
    monkeypatch.setenv("STAG_COMBINE_GROUPS", "0")
    single = launch()
    torch.cuda.synchronize()
    _counters_zero(plans, what + " (single team)")
    monkeypatch.delenv("STAG_COMBINE_GROUPS")
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(runs[0]), bits(single)), f"{what}: group-wise and single-team combine differ"
    assert torch.equal(bits(runs[0]), bits(runs[1])) and torch.equal(bits(runs[0]), bits(runs[2])), f"{what}: launches differ"
    assert_close(runs[0], ref, what=f"{what} vs oracle")
    # a second stream: counters of its own (keyed by stream), the same bits
    before = {id(c) for plan in plans for c in plan["counters"].values()}
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = launch()
    side.synchronize()
    torch.cuda.synchronize()
    after = [c for plan in plans for c in plan["counters"].values()]
    assert len(after) > len(before) and len({c.data_ptr() for c in after}) == len(after), f"{what}: streams share counters"
    _counters_zero(plans, what + " (second stream)")
    assert torch.equal(bits(runs[0]), bits(other)), f"{what}: the launch on a second stream differs"
    for plan in plans:          # the side stream's entries go: the next case starts from the default stream's alone
        for key in [k for k, c in plan["counters"].items() if id(c) not in before]:
            del plan["counters"][key]
            plan.get("_structs", {}).clear()


def _forward_case(monkeypatch, oracle, dev, name, D, kind, reduce="sum", relu=False, n_extra=0):
    from stag_amd import ops
    g, seg_len = _graph(dev, name, n_extra)
    xh, x = _x(g.number_of_nodes(), D, dev)
    noise, spec = _noise_and_spec(oracle, g, D, kind, dev, relu=relu)
    with hw_normals(oracle, dev):
        ref = oracle.agg_fwd(oracle_graph(oracle, g), xh, spec,
                             reduce=oracle.REDUCE_MEAN if reduce == "mean" else oracle.REDUCE_SUM)
    plan = g.csr.plan(seg_len, need=True)
    hubs = GRAPHS[name][0]
    assert plan["n_seg"] >= sum(-(-h // seg_len) for h in hubs)
    _check(monkeypatch, lambda: ops.aggregate(g, x, noise, reduce=reduce, seg_len=seg_len), ref, [plan],
           f"{name} D={D} {kind} {reduce} relu={relu}", dev)
    return plan


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_groupwise_combine_forward(dev, oracle, monkeypatch, name, D):
    for kind in ("none", "normal", "bernoulli"):
        _forward_case(monkeypatch, oracle, dev, name, D, kind)


@pytest.mark.parametrize("D", [64, 128, 512])
def test_groupwise_combine_mean_relu(dev, oracle, monkeypatch, D):
    _forward_case(monkeypatch, oracle, dev, "three", D, "normal", reduce="mean", relu=True)
    _forward_case(monkeypatch, oracle, dev, "h513", D, "bernoulli", reduce="mean")


@pytest.mark.parametrize("D", [128, 512])
def test_groupwise_combine_dispatcher(dev, oracle, monkeypatch, D):
    """The same launches through torch.ops.stag.agg_fwd (csrc/torch_ext.cpp sizes the workspace, ops._plan_args hands
    over the counters) instead of the ctypes binding."""
    from stag_amd import _torch_ext
    monkeypatch.setenv("STAG_TORCH_OPS", "1")
    assert _torch_ext.available()
    for kind in ("normal", "bernoulli"):
        _forward_case(monkeypatch, oracle, dev, "three", D, kind)


@pytest.mark.parametrize("kind", ["none", "normal", "bernoulli"])
def test_groupwise_combine_large_plan(dev, oracle, monkeypatch, kind):
    """At D = 128 the graphs above (at most 49152 units) run the two-slot SMALL twin; 49,200 more one-edge rows make the
    same hub rows part of a launch of the one-slot kernels (the plain kernel for Normal)."""
    plan = _forward_case(monkeypatch, oracle, dev, "three", 128, kind, n_extra=49200)
    assert plan["n_units"] > 49152
    assert _graph(dev, "three")[0].csr.plan(16, need=True)["n_units"] <= 49152


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_groupwise_combine_mc(dev, oracle, monkeypatch, D, norm):
    """aggregate_mc with 2 samples: two outputs per pass (with in-norm: and two sets of weight sums) through the same
    tail; sample s is the oracle's launch at offset + s."""
    import stag_amd
    from stag_amd import _lib, ops
    g, seg_len = _graph(dev, "three")
    xh, x = _x(g.number_of_nodes(), D, dev)
    E = g.number_of_edges()
    if norm:
        noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_BERNOULLI, 0.7, None, in_norm=True, seed=5, offset=2)
        spec = lambda s: oracle.make_spec("bernoulli", 0.7, None, in_norm=True, seed=5, offset=2 + s, Dn=D, n_edges=E)
    else:
        noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=5, offset=2)
        spec = lambda s: oracle.make_spec("normal", 1.0, 0.5, seed=5, offset=2 + s, Dn=D, n_edges=E)
    with hw_normals(oracle, dev):
        ref = np.stack([oracle.agg_fwd(oracle_graph(oracle, g), xh, spec(s)) for s in range(2)])
    _check(monkeypatch, lambda: ops.aggregate_mc(g, x, noise, 2, seg_len=seg_len), ref, [g.csr.plan(seg_len, need=True)],
           f"mc D={D} norm={norm}", dev)


@pytest.mark.parametrize("D", [64, 128])
def test_groupwise_combine_backward(dev, oracle, monkeypatch, D):
    """The backward of ops.aggregate walks the transposed view: a source with 520 out-edges is a 33-segment row there."""
    import stag_amd
    from stag_amd import _lib, ops
    g, seg_len = _graph(dev, "h257", out_hub=520)
    n, E = g.number_of_nodes(), g.number_of_edges()
    xh, x = _x(n, D, dev)
    gh, gout = _x(n + 1, D, dev)
    gh, gout = gh[:n], gout[:n]
    noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=9, offset=4)
    spec = oracle.make_spec("normal", 1.0, 0.5, seed=9, offset=4, Dn=D, n_edges=E)
    with hw_normals(oracle, dev):
        ref = oracle.agg_fwd(oracle_graph(oracle, g, transposed=True), gh, spec)
    plan_t = g.csr_t.plan(seg_len, need=True)
    assert plan_t["n_seg"] >= 33

    def launch():
        xd = x.clone().requires_grad_(True)
        ops.aggregate(g, xd, noise, seg_len=seg_len).backward(gout)
        return xd.grad

    _check(monkeypatch, launch, ref, [g.csr.plan(seg_len, need=True), plan_t], f"backward D={D}", dev)
