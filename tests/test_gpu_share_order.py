"""The share order on the device (stag_plan_share_device) and in the launches that take it (CsrView.share_units):
the builder keeps the contract of the host builder and is deterministic, finds at least 0.7 of the repeated sources the
sequential greedy finds, and no launch changes a bit when it walks the share order instead of plan order."""
import importlib

import numpy as np
import pytest
import torch

from test_share_order_host import check_contract, csr_of, host_plan, share_host

pytestmark = pytest.mark.gpu

N, E, HUB = 2000, 12000, 1200
_CACHE = {}


def _edges(name):
    from stag_amd import synthetic
    if name == "five":
        src = np.array([1, 2, 0, 0, 1, 4, 0], np.int64)
        dst = np.array([0, 0, 1, 3, 3, 3, 4], np.int64)
        return src, dst, 5
    src, dst = synthetic.arxiv_like(n_nodes=N, n_edges=E, max_in_degree=HUB, n_hubs=5, seed=4)
    return src, dst, N


def _graph(dev, name, share):
    """The graph with its plans (seg_len 8 and 64, both views) built under STAG_SHARE_ORDER = share ("0" | "1")."""
    import stag_amd
    key = (name, share)
    if key not in _CACHE:
        gm = importlib.import_module("stag_amd.graph")
        old = gm.SHARE_ORDER, gm.XCD_ORDER
        gm.SHARE_ORDER, gm.XCD_ORDER = share, "0"
        try:
            src, dst, n = _edges(name)
            g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
            for view in (g.csr, g.csr_t):
                for sl in (8, 64):
                    plan = view.plan(sl, need=True)
                    assert bool(plan.get("share_decided")) == (share == "1") and ("share" in plan) == (share == "1")
        finally:
            gm.SHARE_ORDER, gm.XCD_ORDER = old
        _CACHE[key] = g
    return _CACHE[key]


def _host(view, plan):
    nu = plan["n_units"]
    return plan["units"][:nu].cpu().numpy(), view.indices.cpu().numpy()


def test_hub_and_segments_are_what_the_cases_need(dev):
    g = _graph(dev, "skewed", "0")
    assert int(g.csr.degrees.max()) >= HUB * 0.9
    assert g.csr.plan(8)["n_seg"] > 16 and 0 < g.csr.plan(64)["n_seg"]


@pytest.mark.parametrize("name", ["skewed", "five"])
@pytest.mark.parametrize("seg_len", [8, 64])
@pytest.mark.parametrize("transposed", [False, True])
def test_device_builder_contract_and_determinism(dev, name, seg_len, transposed):
    g = _graph(dev, name, "1")
    view = g.csr_t if transposed else g.csr
    plan = view.plan(seg_len)
    units, indices = _host(view, plan)
    first = plan["share"][:plan["n_units"]].cpu().numpy()
    check_contract(units, first, plan["n_seg"], plan["n_heavy"])
    again = view._build_share_units(plan)[:plan["n_units"]].cpu().numpy()
    assert np.array_equal(first, again), "two builds of the same graph differ"
    assert np.array_equal(units, plan["units"][:plan["n_units"]].cpu().numpy()), "the plan's own records changed"


def test_device_builder_finds_the_planted_groups(dev):
    """rows (r, r + 32) share a source; 8, 4 and 2 rows around three more: every group side by side and aligned"""
    from stag_amd.graph import CsrView
    rows, fresh = [], 10_000
    member = {r: 0 for r in (1, 6, 11, 17, 22, 29, 33, 38)}
    member.update({r: 1 for r in (3, 12, 25, 36)})
    member.update({r: 2 for r in (8, 30)})
    for r in range(40):
        row = [member[r]] if r in member else []
        while len(row) < 4:
            row.append(fresh)
            fresh += 1
        rows.append(row)
    for r in range(64):
        rows.append([5000 + r % 32, fresh, fresh + 1])
        fresh += 2
    indptr, indices = csr_of(rows)
    view = CsrView(len(rows), fresh, torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev))
    units, n_seg, n_heavy = host_plan(indptr, 64)
    plan = dict(units=torch.from_numpy(units).to(dev), n_units=len(units), n_seg=n_seg, n_heavy=n_heavy, seg_len=64)
    out = view._build_share_units(plan).cpu().numpy()
    check_contract(units, out, n_seg, n_heavy)
    at = {int(r): i for i, r in enumerate(out[:, 0])}
    for size, s in ((8, 0), (4, 1), (2, 2)):
        where = sorted(at[r] for r in member if member[r] == s)
        assert where[0] % size == 0 and where == list(range(where[0], where[0] + size)), (size, where)
    for r in range(32):
        a, b = sorted((at[40 + r], at[40 + r + 32]))
        assert a % 2 == 0 and b == a + 1, (r, a, b)


def test_device_builder_against_the_sequential_greedy(dev):
    from stag_amd.graph import repeated_sources
    g = _graph(dev, "skewed", "1")
    plan = g.csr.plan(64)
    units, indices = _host(g.csr, plan)
    n_seg = plan["n_seg"]
    greedy = share_host(units, n_seg, plan["n_heavy"], 64, indices)
    found = repeated_sources(plan["share"][:plan["n_units"]].cpu().numpy(), n_seg, indices)
    wanted = repeated_sources(greedy, n_seg, indices)
    print(f"repeated sources per block of 8: plan order {repeated_sources(units, n_seg, indices)}, "
          f"device builder {found}, sequential greedy {wanted}")
    assert wanted >= 100 and found >= 0.7 * wanted


def _launches(g, D, seg_len, dev):
    """name -> tensor: every launch that takes the share order, on g"""
    import stag_amd
    from stag_amd import _lib, ops
    n, ne = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(D)
    x = torch.randn(n, D, generator=gen).to(dev)
    gout = torch.randn(n, D, generator=gen).to(dev)
    ss, ds = (torch.rand(n, generator=gen) + 0.5).to(dev), (torch.rand(n, generator=gen) + 0.5).to(dev)
    loc, ls = (torch.rand(ne, 1, generator=gen) + 0.5).to(dev), (torch.rand(ne, 1, generator=gen) - 1.5).to(dev)
    w_full, w_one = torch.rand(ne, D, generator=gen).to(dev), (torch.rand(ne, generator=gen) - 0.2).to(dev)
    N_, U_, B_ = _lib.NOISE_NORMAL, _lib.NOISE_UNIFORM, _lib.NOISE_BERNOULLI
    mk = lambda kind, p0, p1=None, dn=D, **kw: stag_amd.EdgeNoise(g, dn, kind, p0, p1, seed=9, offset=5, **kw)
    spec = lambda noise: ops._targs_or_c(ops._noise_spec(noise))
    out = {}
    with torch.no_grad():
        out["none"] = ops.aggregate(g, x, None, seg_len=seg_len)
        out["explicit"] = ops.aggregate(g, x, w_full, seg_len=seg_len)
        out["normal"] = ops.aggregate(g, x, mk(N_, 1.0, 0.5), seg_len=seg_len)
        out["normal relu per channel"] = ops.aggregate(g, x, mk(N_, torch.rand(D, generator=gen).to(dev), 0.5, relu=True),
                                                       src_scale=ss, dst_scale=ds, seg_len=seg_len)
        out["uniform"] = ops.aggregate(g, x, mk(U_, 0.2, 1.8), seg_len=seg_len)
        out["bernoulli"] = ops.aggregate(g, x, mk(B_, 0.7), seg_len=seg_len)
        out["bernoulli in-norm"] = ops.aggregate(g, x, mk(B_, 0.7, in_norm=True), seg_len=seg_len)
        out["normal in-norm mean"] = ops.aggregate(g, x, mk(N_, 1.0, 0.5, relu=True, in_norm=True), reduce="mean", seg_len=seg_len)
        out["uniform mean"] = ops.aggregate(g, x, mk(U_, 0.2, 1.8), reduce="mean", seg_len=seg_len)
        out["per-edge parameters"] = ops._agg_raw(g.csr, x, D, ops._noise_spec(mk(N_, loc, ls, p1_log=True)), _lib.REDUCE_SUM,
                                                  None, None, seg_len)[0]
        out["mc x3"] = ops._agg_fwd_mc_raw(g.csr, x, mk(N_, 1.0, 0.5), 3, 1, _lib.REDUCE_SUM, ss, None, seg_len)
        out["mc x2 in-norm"] = ops._agg_fwd_mc_raw(g.csr, x, mk(U_, 0.2, 1.8, in_norm=True), 2, 7, _lib.REDUCE_MEAN, None, None,
                                                   seg_len)
        out["mc edge x3"] = ops._agg_fwd_mc_edge_raw(g.csr, x, mk(N_, loc, ls, p1_log=True), 3, 1, _lib.REDUCE_SUM, ss, ds, seg_len)
        if D % 8 == 0:
            for dt in (torch.float16, torch.bfloat16):
                out[f"half rows {dt}"] = ops._agg_half_raw(g.csr, x.to(dt), D, spec(mk(N_, 1.0, 0.5)), _lib.REDUCE_MEAN, ss, ds,
                                                           seg_len)
        out["[E,1] normal"] = ops._agg_w1_raw(g.csr, x, D, spec(mk(N_, loc, ls, dn=1, p1_log=True, relu=True)), _lib.REDUCE_SUM,
                                              ss, ds, seg_len)
        out["[E,1] bernoulli"] = ops._agg_w1_raw(g.csr, x, D, spec(mk(B_, 0.6, dn=1)), _lib.REDUCE_MEAN, None, None, seg_len)
        out["[E] explicit"] = ops._agg_w1_raw(g.csr, x, D, ops._targs_or_c(ops._explicit_spec(w_one, relu=True)), _lib.REDUCE_SUM,
                                              None, None, seg_len)
        mx = ops._max_fwd_raw(g.csr, x, D, spec(mk(N_, 1.0, 0.5)), seg_len, True)
        out["max"], out["max cnt"] = mx[0], mx[1]
        out["max none"] = ops._max_fwd_raw(g.csr, x, D, ops._targs_or_c(ops._none_spec()), seg_len, False)[0]
        dx, t0, t1 = ops._agg_bwd_raw(g.csr_t, gout, D, ops._noise_spec(mk(N_, 1.0, 0.5, relu=True), in_norm=False), ds, ss, seg_len,
                                      True)
        out["bwd dx"], out["bwd dp0 rows"], out["bwd dp1 rows"] = dx, t0, t1
        out["bwd dx only"] = ops._agg_bwd_raw(g.csr_t, gout, D, ops._noise_spec(mk(U_, 0.2, 1.8), in_norm=False), None, None,
                                              seg_len, False)[0]
        got = ops._agg_bwd_edge_raw(g.csr_t, gout, x, D, ops._targs_or_c(ops._noise_spec(mk(N_, loc, ls, p1_log=True))), ds, ss,
                                    seg_len)
        for k, t in enumerate(got or ()):
            if t is not None:
                out[f"bwd edge {k}"] = t
    xg = x.clone().requires_grad_(True)
    ops.aggregate(g, xg, mk(N_, 1.0, 0.5, relu=True), reduce="mean", src_scale=ss, seg_len=seg_len).backward(gout)
    out["autograd dx"] = xg.grad
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,seg_len", [("skewed", 8), ("skewed", 64), ("five", 64)])
@pytest.mark.parametrize("D", [16, 128, 256])
def test_share_order_changes_no_bit(dev, name, seg_len, D):
    g0, g1 = _graph(dev, name, "0"), _graph(dev, name, "1")
    if name == "skewed":
        for view in (g1.csr, g1.csr_t):
            plan = view.plan(seg_len)
            assert view.share_units(plan) is plan["share"] and not torch.equal(plan["share"][:plan["n_units"]],
                                                                             plan["units"][:plan["n_units"]])
    assert g0.csr.share_units(g0.csr.plan(seg_len)) is None
    plain, shared = _launches(g0, D, seg_len, dev), _launches(g1, D, seg_len, dev)
    assert plain.keys() == shared.keys() and len(plain) >= 25
    for what in plain:
        assert torch.equal(plain[what], shared[what]), f"{name} seg_len={seg_len} D={D}: {what} differs under the share order"


def test_policy_switches_after_the_threshold_and_not_before(dev, monkeypatch):
    import stag_amd
    from stag_amd import _lib, ops
    gm = importlib.import_module("stag_amd.graph")
    monkeypatch.setattr(gm, "SHARE_ORDER", "auto")
    monkeypatch.setattr(gm, "XCD_ORDER", "auto")
    monkeypatch.setattr(gm, "SHARE_AFTER_LAUNCHES", 40)
    src, dst, n = _edges("skewed")
    x = torch.randn(n, 128, device=dev)
    new = lambda: stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    launch = lambda g: ops.aggregate(g, x, stag_amd.EdgeNoise(g, 128, _lib.NOISE_NORMAL, 1.0, 0.5, seed=2, offset=1))
    g = new()
    first = launch(g)
    plan = g.csr.plan(64)                                   # (a request of its own: it counts as a launch)
    while plan["share_uses"] < 40:
        assert torch.equal(launch(g), first) and "share" not in plan
    assert plan["share_uses"] == 40 and plan.get("xcd_declined") and g.csr.share_units(plan) is None
    assert torch.equal(launch(g), first)                    # the 41st request builds it and walks it
    assert plan.get("share") is not None and g.csr.share_units(plan) is plan["share"] and plan["share_decided"]
    assert torch.equal(launch(g), first)
    # (rows narrower than SHARE_MIN_WIDTH keep plan order unless the order was forced)
    assert g.csr.share_units(plan, gm.SHARE_MIN_WIDTH) is plan["share"] and g.csr.share_units(plan, gm.SHARE_MIN_WIDTH - 1) is None
    # an order the caller settled stays: plan order ...
    g = new()
    plan = g.csr.plan(64)
    plan["xcd_decided"] = True
    for _ in range(45):
        launch(g)
    assert "share" not in plan and plan["share_decided"]
    # ... and so does the XCD-aware order, whatever STAG_SHARE_ORDER says
    monkeypatch.setattr(gm, "SHARE_ORDER", "1")
    g = new()
    plan = g.csr.plan(64)
    assert plan.get("share") is not None
    g.csr._add_xcd_order(plan)
    assert g.csr.share_units(plan) is None
    assert torch.equal(launch(g), first)
    monkeypatch.setattr(gm, "SHARE_ORDER", "0")
    g = new()
    for _ in range(45):
        launch(g)
    assert "share" not in g.csr.plan(64)
