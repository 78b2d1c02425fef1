"""The noise kernels across the whole 64-bit counter space (run on the GPU box: -m gpu).

Every draw is Philox4x32-10 at ctr = {lo32(gpos), chunk | hi32(gpos) << 20, lo32(offset), hi32(offset)},
key = {lo32(seed), hi32(seed)} (include/stag_hip.h, "Noise stream"), and every entry point splits those 64-bit
values into 32-bit words, folds the device epoch in, and adds positions in 32 bits on its own.  The rest of the
suite draws at small seeds and offsets with pos_base = 0, where the high words are 0 and no addition carries.
Here each entry point runs in named counter regimes whose high words are not 0 and whose additions carry, against
the fp64 oracle at the equivalent counters (the oracle has no epoch: a launch at (offset O, epoch e) is the
oracle's at (O + e) mod 2^64), through both front ends (ctypes, torch.ops.stag.*) where a dispatcher op exists.
Normal draws come from the device's tables inside the oracle (util.hw_normals), so the weights agree bit for bit.
"""
import copy

import numpy as np
import pytest
import torch

from util import assert_close, assert_close_cond, assert_gat_grads_vs_oracle, hw_normals, oracle_graph, random_graph

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1

# id: (seed, offset, device epoch or None, pos_base); pos_base None: 5 * 2^32 - E, the last edge right below a
# 2^32 boundary of the position space (the launch is allowed)
REGIMES = {
    "low": (5, 3, None, 0),
    "seed_hi": (0xFEDCBA9876543210, 3, None, 0),
    "off_hi": (9, 2**32 + 7, None, 0),
    "off_top": (9, 2**63 + 11, None, 0),               # through the signed-int64 conversion of the dispatcher
    "epoch_carry": (9, 2**32 - 3, 5, 0),               # o0 + epoch carries into o1 inside the kernel
    "epoch_wrap": (9, 2**64 - 2, 7, 0),                # wraps mod 2^64
    "pos_hi": (9, 3, None, 3 * 2**32 + 17),            # hi32(gpos) != 0
    "pos_edge": (9, 3, None, None),
}
REGIME_IDS = list(REGIMES)


@pytest.fixture(params=["ctypes", "torch_ops"])
def front(request, monkeypatch):
    """The ctypes binding or the dispatcher ops (csrc/torch_ext.cpp) under ops.*: the same library, two argument paths."""
    if request.param == "torch_ops":
        monkeypatch.setenv("STAG_TORCH_OPS", "1")
        from stag_amd import _torch_ext
        assert _torch_ext.available()
    else:
        monkeypatch.delenv("STAG_TORCH_OPS", raising=False)
    return request.param


def _counters(regime, E, dev):
    """(device kwargs of EdgeNoise, the same launch as oracle kwargs, the same launch split differently between the
    host offset and the device epoch): (O, e) -> (O + e, none); (O, none) -> (O - 1, 1)."""
    seed, off, ep, pb = REGIMES[regime]
    pb = 5 * 2**32 - E if pb is None else pb
    epoch = None if ep is None else torch.tensor([ep], dtype=torch.int64, device=dev)
    kw = dict(seed=seed, offset=off, pos_base=pb, epoch=epoch)
    okw = dict(seed=seed, offset=(off + (ep or 0)) & M64, pos_base=pb)
    if ep is None:
        alt = dict(seed=seed, offset=(off - 1) & M64, pos_base=pb, epoch=torch.ones(1, dtype=torch.int64, device=dev))
    else:
        alt = dict(seed=seed, offset=(off + ep) & M64, pos_base=pb, epoch=None)
    return kw, okw, alt


def _noise(g, dn, kind, p0, p1=None, **kw):
    import stag_amd
    from stag_amd import _lib
    k = {"normal": _lib.NOISE_NORMAL, "uniform": _lib.NOISE_UNIFORM, "bernoulli": _lib.NOISE_BERNOULLI}[kind]
    return stag_amd.EdgeNoise(g, dn, k, p0, p1, **kw)


def _np(p):
    return p.detach().cpu().numpy() if torch.is_tensor(p) else p


def _ospec(O, g, dn, kind, p0, p1=None, **kw):
    return O.make_spec(kind, _np(p0), _np(p1), Dn=dn, n_edges=g.number_of_edges(), **kw)


def _params(mode, kind, E, D, rng, dev):
    """(p0, p1) of a parameter mode: scalar, [D], [E, 1], [E, D]; Bernoulli has p0 only."""
    shape = {"scalar": None, "per_channel": (D,), "per_edge1": (E, 1), "per_edge": (E, D)}[mode]
    if shape is None:
        return {"normal": (1.0, 0.5), "uniform": (0.4, 1.6), "bernoulli": (0.6, None)}[kind]
    a = rng.uniform(0.3, 0.9, shape).astype(np.float32)
    b = (a + rng.uniform(0.5, 1.0, shape)).astype(np.float32)
    t = lambda v: torch.from_numpy(v).to(dev)
    return (t(a), None) if kind == "bernoulli" else (t(a), t(b))


def _graph(dev, n=300, e=1500, hub=300, seed=4):
    """A few hundred rows and a hub row far longer than the segment length: segments and partial merges draw too."""
    return random_graph(n, e, seed=seed, hub=hub, device=dev)


# ---- stag_agg_fwd through ops.aggregate -----------------------------------------------------------------------
AGG_CASES = [("normal", "scalar", True, False), ("uniform", "per_channel", False, True),
             ("bernoulli", "per_edge1", False, True), ("normal", "per_edge", False, False),
             ("uniform", "per_edge1", True, False), ("bernoulli", "scalar", False, False)]


@pytest.mark.parametrize("D", [6, 128, 300])
@pytest.mark.parametrize("regime", REGIME_IDS)
def test_aggregate_counter_regimes(dev, oracle, front, regime, D):
    from stag_amd import ops
    rng = np.random.default_rng(D)
    g = _graph(dev)
    n, E = g.number_of_nodes(), g.number_of_edges()
    og = oracle_graph(oracle, g)
    kw, okw, alt = _counters(regime, E, dev)
    x = rng.standard_normal((n, D)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    for kind, mode, relu, norm in AGG_CASES:
        p0, p1 = _params(mode, kind, E, D, rng, dev)
        what = f"{regime} {front} D={D} {kind}/{mode} relu={relu} norm={norm}"
        got = ops.aggregate(g, xd, _noise(g, D, kind, p0, p1, relu=relu, in_norm=norm, **kw), seg_len=32)
        with hw_normals(oracle, dev):
            ref = oracle.agg_fwd(og, x, _ospec(oracle, g, D, kind, p0, p1, relu=relu, in_norm=norm, **okw))
        assert_close(got, ref, what=what)
        again = ops.aggregate(g, xd, _noise(g, D, kind, p0, p1, relu=relu, in_norm=norm, **alt), seg_len=32)
        assert torch.equal(got, again), f"{what}: (offset, epoch) split differently"


# ---- stag_agg_fwd_mc through ops.aggregate_mc ------------------------------------------------------------------
# id: (offset, offset_stride, epoch, in_norm)
MC_CASES = {
    "carry_in_pass": (2**32 - 2, 1, None, False),      # o1 changes between samples of one 4-sample pass
    "stride_hi": (3, 2**40 + 1, None, False),          # (o + 1) * stride needs 64 bits
    "wrap": (2**64 - 5, 1, None, False),
    "in_norm": (2**32 - 3, 2**33 + 1, None, True),     # 2 samples per pass
    "epoch": (2**32 - 6, 2**32 + 1, 3, False),         # the epoch, then key_plus, both carrying
}


@pytest.mark.parametrize("D", [6, 128, 300])
@pytest.mark.parametrize("case", list(MC_CASES))
def test_aggregate_mc_counter_regimes(dev, oracle, front, case, D):
    from stag_amd import ops
    off, stride, ep, norm = MC_CASES[case]
    S, seed, pb = 8, 0xFEDCBA9876543210, 2**32 + 5
    rng = np.random.default_rng(D + 1)
    g = _graph(dev)
    n = g.number_of_nodes()
    x = rng.standard_normal((n, D)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    p0 = torch.from_numpy(rng.uniform(0.4, 0.9, D).astype(np.float32)).to(dev)
    p1 = torch.from_numpy(rng.uniform(1.0, 1.6, D).astype(np.float32)).to(dev)
    kind = "uniform" if norm else "normal"
    epoch = None if ep is None else torch.tensor([ep], dtype=torch.int64, device=dev)
    noise = _noise(g, D, kind, p0, p1, relu=not norm, in_norm=norm, seed=seed, offset=off, pos_base=pb, epoch=epoch)
    got = ops.aggregate_mc(g, xd, noise, S, offset_stride=stride, reduce="mean", seg_len=32)
    assert got.shape == (S, n, D)
    og = oracle_graph(oracle, g)
    for s in range(S):
        o_s = (off + (ep or 0) + s * stride) & M64
        with hw_normals(oracle, dev):
            ref = oracle.agg_fwd(og, x, _ospec(oracle, g, D, kind, p0, p1, relu=not norm, in_norm=norm, seed=seed,
                                               offset=o_s, pos_base=pb), reduce=oracle.REDUCE_MEAN)
        assert_close(got[s], ref, what=f"mc {case} {front} D={D} sample {s}")
        one = copy.copy(noise)
        one.offset = (off + s * stride) & M64
        assert torch.equal(got[s], ops.aggregate(g, xd, one, reduce="mean", seg_len=32)), f"mc {case} sample {s} != one launch"
    # the twin of stag_agg_fwd_mc in the oracle, where its offsets stay below 2^64
    if (off + (ep or 0) + (S - 1) * stride) <= M64:
        with hw_normals(oracle, dev):
            twin = oracle.agg_fwd_mc(og, x, _ospec(oracle, g, D, kind, p0, p1, relu=not norm, in_norm=norm, seed=seed,
                                                   offset=(off + (ep or 0)) & M64, pos_base=pb),
                                     S, offset_stride=stride, reduce=oracle.REDUCE_MEAN)
        assert_close(got.cpu().numpy(), twin, what=f"mc {case} vs oracle.agg_fwd_mc")


# ---- the channel field: the last chunk_base a noise width allows -------------------------------------------------
@pytest.mark.parametrize("D", [6, 128, 300])
def test_chunk_field_top(dev, oracle, front, D):
    """chunk_base = 2^20 - ceil(D/4), set the way partition.ChannelShard sets it: the last chunk is 2^20 - 1."""
    from stag_amd import ops
    rng = np.random.default_rng(D + 2)
    g = _graph(dev)
    n, E = g.number_of_nodes(), g.number_of_edges()
    og = oracle_graph(oracle, g)
    cb = (1 << 20) - (D + 3) // 4
    x = rng.standard_normal((n, D)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    for kind, mode in (("normal", "per_channel"), ("uniform", "scalar"), ("bernoulli", "per_edge")):
        p0, p1 = _params(mode, kind, E, D, rng, dev)
        nz = _noise(g, D, kind, p0, p1, seed=9, offset=2**32 + 1, pos_base=2**33)
        nz.chunk_base = cb
        osp = _ospec(oracle, g, D, kind, p0, p1, seed=9, offset=2**32 + 1, pos_base=2**33, chunk_base=cb)
        with hw_normals(oracle, dev):
            ref = oracle.agg_fwd(og, x, osp)
            wref = oracle.noise_materialize(og, osp, D)
        assert_close(ops.aggregate(g, xd, nz, seg_len=32), ref, what=f"chunk top {kind} D={D}")
        assert_close(ops.materialize_noise(g, nz), wref, what=f"chunk top materialised {kind} D={D}")
        if mode != "per_edge":
            mc = ops.aggregate_mc(g, xd, nz, 4, offset_stride=3, seg_len=32)
            for s in range(4):
                with hw_normals(oracle, dev):
                    r = oracle.agg_fwd(og, x, _ospec(oracle, g, D, kind, p0, p1, seed=9, offset=2**32 + 1 + 3 * s,
                                                     pos_base=2**33, chunk_base=cb))
                assert_close(mc[s], r, what=f"chunk top mc {kind} D={D} sample {s}")
    # one chunk further is refused, not aliased
    nz = _noise(g, D, "normal", 1.0, 0.5, seed=9)
    nz.chunk_base = cb + 1
    with pytest.raises(RuntimeError, match="rc=-22"):
        ops.aggregate(g, xd, nz)


# ---- stag_noise_materialize ------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIME_IDS)
def test_materialize_counter_regimes(dev, oracle, regime):
    from stag_amd import ops
    rng = np.random.default_rng(3)
    g = _graph(dev)
    E = g.number_of_edges()
    og = oracle_graph(oracle, g)
    kw, okw, alt = _counters(regime, E, dev)
    for D in (6, 128, 300):
        for kind, mode, relu, norm in AGG_CASES:
            p0, p1 = _params(mode, kind, E, D, rng, dev)
            what = f"materialise {regime} D={D} {kind}/{mode} relu={relu} norm={norm}"
            got = ops.materialize_noise(g, _noise(g, D, kind, p0, p1, relu=relu, in_norm=norm, **kw))
            with hw_normals(oracle, dev):
                ref = oracle.noise_materialize(og, _ospec(oracle, g, D, kind, p0, p1, relu=relu, in_norm=norm, **okw), D)
            if kind == "normal" or norm:
                assert_close(got, ref, what=what)
            else:
                assert np.array_equal(got.cpu().numpy(), ref), what
            again = ops.materialize_noise(g, _noise(g, D, kind, p0, p1, relu=relu, in_norm=norm, **alt))
            assert torch.equal(got, again), f"{what}: (offset, epoch) split differently"


# ---- the backward kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIME_IDS)
def test_backward_counter_regimes(dev, oracle, front, regime):
    """stag_agg_bwd (dx and the two derivative aggregates), stag_agg_bwd_dp, stag_agg_bwd_edge and stag_agg_bwd_w
    (one and two derivatives) on the source-major CSR, whose nidx carries the forward positions, against the oracle's
    aggregation / weight gradient with spec.deriv = 0, 1, 2 at the same counters."""
    from stag_amd import ops
    rng = np.random.default_rng(11)
    g = _graph(dev)
    n, E = g.number_of_nodes(), g.number_of_edges()
    ogt, og = oracle_graph(oracle, g, transposed=True), oracle_graph(oracle, g)
    kw, okw, alt = _counters(regime, E, dev)
    with hw_normals(oracle, dev):
        for D in (6, 40, 300):
            for kind, relu in (("normal", True), ("uniform", False)):
                what = f"bwd {regime} {front} D={D} {kind} relu={relu}"
                x, gout = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((n, D)).astype(np.float32)
                gs, rs = rng.uniform(0.5, 1.5, n).astype(np.float32), rng.uniform(0.5, 1.5, n).astype(np.float32)
                xd, gd, gsd, rsd = (torch.from_numpy(a).to(dev) for a in (x, gout, gs, rs))
                p0 = rng.uniform(0.2, 1.0, D).astype(np.float32)
                p1 = (p0 + rng.uniform(0.6, 1.2, D)).astype(np.float32)
                noise = _noise(g, D, kind, torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev), relu=relu, **kw)
                osp = lambda dv, a=p0, b=p1: _ospec(oracle, g, D, kind, a, b, relu=relu, deriv=dv, **okw)
                T = [oracle.agg_fwd(ogt, gout, osp(dv), src_scale=gs, dst_scale=rs) for dv in (0, 1, 2)]
                A = [oracle.agg_fwd(ogt, np.abs(gout), oracle.make_spec("explicit", np.abs(oracle.noise_materialize(ogt, osp(dv), D))),
                                    src_scale=gs, dst_scale=rs) for dv in (0, 1, 2)]
                dx, t0, t1 = ops._agg_bwd_raw(g.csr_t, gd, D, ops._noise_spec(noise), gsd, rsd, 32, True)
                for got, ref, ab, nm in ((dx, T[0], A[0], "dx"), (t0, T[1], A[1], "T0"), (t1, T[2], A[2], "T1")):
                    assert_close_cond(got, ref, ab, what=f"{what} stag_agg_bwd {nm}")
                alt_noise = _noise(g, D, kind, torch.from_numpy(p0).to(dev), torch.from_numpy(p1).to(dev), relu=relu, **alt)
                adx, at0, at1 = ops._agg_bwd_raw(g.csr_t, gd, D, ops._noise_spec(alt_noise), gsd, rsd, 32, True)
                assert torch.equal(dx, adx) and torch.equal(t0, at0) and torch.equal(t1, at1), f"{what}: epoch split"
                # stag_agg_bwd_dp: the finished per-channel gradients
                dx2, c0, c1 = ops._agg_bwd_dp_raw(g.csr_t, gd, xd, D, ops._noise_spec(noise), gsd, rsd, 32)
                assert_close_cond(dx2, T[0], A[0], what=f"{what} stag_agg_bwd_dp dx")
                for got, Ti, Ai, nm in ((c0, T[1], A[1], "d p0"), (c1, T[2], A[2], "d p1")):
                    ref = (x.astype(np.float64) * Ti.astype(np.float64)).sum(0)
                    sc = max(1.0, float(np.abs(ref).max()))
                    assert_close_cond(got / sc, ref / sc, (np.abs(x).astype(np.float64) * Ai).sum(0) / sc,
                                      what=f"{what} stag_agg_bwd_dp {nm}")
                # stag_agg_bwd_w: the [E, D] derivative of one parameter, then both from one pass (ctypes only)
                sp = noise.spec()
                sp.deriv = 1
                w1 = ops._bwd_w_raw(g.csr, xd, gd, D, gsd, spec=sp)
                sp.deriv = 0
                b0, b1 = ops._bwd_w_raw(g.csr, xd, gd, D, gsd, spec=sp, both=True)
                for dv, got in ((1, w1), (1, b0), (2, b1)):
                    ref = oracle.agg_bwd_w(og, x, gout, src_scale=gs, spec=osp(dv))
                    assert_close(got, ref, what=f"{what} stag_agg_bwd_w deriv={dv}")
                # stag_agg_bwd_edge: [E, 1] parameters (one channel tile; ctypes only)
                if D <= 256:
                    q0 = rng.uniform(0.2, 1.0, (E, 1)).astype(np.float32)
                    q1 = (q0 + rng.uniform(0.6, 1.2, (E, 1))).astype(np.float32)
                    nz = _noise(g, D, kind, torch.from_numpy(q0).to(dev), torch.from_numpy(q1).to(dev), relu=relu, **kw)
                    dx3, e0, e1 = ops._agg_bwd_edge_raw(g.csr_t, gd, xd, D, nz.spec(), gsd, rsd, 32)
                    oq = lambda dv: _ospec(oracle, g, D, kind, q0, q1, relu=relu, deriv=dv, **okw)
                    ab = oracle.agg_fwd(ogt, np.abs(gout), oracle.make_spec("explicit", np.abs(oracle.noise_materialize(ogt, oq(0), D))),
                                        src_scale=gs, dst_scale=rs)
                    assert_close_cond(dx3, oracle.agg_fwd(ogt, gout, oq(0), src_scale=gs, dst_scale=rs), ab,
                                      what=f"{what} stag_agg_bwd_edge dx")
                    for dv, got in ((1, e0), (2, e1)):
                        ref = oracle.agg_bwd_w(og, x, gout * gs[:, None], src_scale=rs, spec=oq(dv)).astype(np.float64).sum(1, keepdims=True)
                        sc = max(1.0, float(np.abs(ref).max()))
                        assert_close(got / sc, ref / sc, what=f"{what} stag_agg_bwd_edge d p{dv - 1}")


# ---- GAT -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIME_IDS)
def test_gat_counter_regimes(dev, oracle, front, regime, monkeypatch):
    """ops.gat_aggregate forward with the attention (stag_gat_fwd + stag_gat_attn), its backward through the one-gather
    (stag_gat_bwd), two-pass (stag_gat_bwd_two_pass) and per-edge (stag_gat_bwd_edge + stag_agg_fwd) forms, the staged
    backward (stag_gat_bwd_stages) against the whole one, and a vi=True draw's parameter gradients (stag_gat_bwd_dp);
    attention dropout with its mask at the regime's counters."""
    import stag_amd
    from stag_amd import _lib, ops
    from stag_amd.random import ATTN_DROP_DOMAIN
    H, F = 4, 16
    rng = np.random.default_rng(5)
    g = _graph(dev, n=300, e=2500, hub=400, seed=6)
    n, E = g.number_of_nodes(), g.number_of_edges()
    og = oracle_graph(oracle, g)
    kw, okw, alt = _counters(regime, E, dev)
    el, er = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((n, H)).astype(np.float32)
    ft, G = rng.standard_normal((n, H, F)).astype(np.float32), rng.standard_normal((n, H, F)).astype(np.float32)
    Gd = torch.from_numpy(G).to(dev)
    t_ = lambda: [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (el, er, ft)]
    for kind, p0, p1, relu, norm in (("normal", 1.0, 0.5, True, False), ("bernoulli", 0.7, None, False, True)):
        what = f"gat {regime} {front} {kind}"
        spec = _ospec(oracle, g, H, kind, p0, p1, relu=relu, in_norm=norm, **okw)
        mk = lambda c: _noise(g, H, kind, p0, p1, relu=relu, in_norm=norm, **c)
        with torch.no_grad():
            out, attn = ops.gat_aggregate(g, *[torch.from_numpy(a).to(dev) for a in (el, er, ft)], 0.2, mk(kw), want_attn=True)
            out_a, attn_a = ops.gat_aggregate(g, *[torch.from_numpy(a).to(dev) for a in (el, er, ft)], 0.2, mk(alt), want_attn=True)
        with hw_normals(oracle, dev):
            ref, ref_attn = oracle.gat_fwd(og, el, er, ft, 0.2, spec, want_attn=True)
        assert_close(out, ref, what=f"{what} out")
        assert_close(attn, ref_attn, what=f"{what} attn")
        assert torch.equal(out, out_a) and torch.equal(attn, attn_a), f"{what}: epoch split"
        for form, one_gather, fused in (("one_gather", True, True), ("two_pass", False, True), ("edge", True, False)):
            monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", one_gather)
            monkeypatch.setattr(ops, "_GAT_BWD_FUSED", fused)
            t = t_()
            ops.gat_aggregate(g, *t, 0.2, mk(kw)).backward(Gd)
            assert_gat_grads_vs_oracle(oracle, og, el, er, ft, G, spec, [a.grad for a in t], what=f"{what} {form}", dev=dev)
        monkeypatch.setattr(ops, "_GAT_BWD_ONE_GATHER", True)
        monkeypatch.setattr(ops, "_GAT_BWD_FUSED", True)
        # the staged backward equals the whole one, bit for bit
        csrv, csrt = g.csr, g.csr_t
        nz = mk(kw)
        sp = nz.spec()
        nscale = ops._gat_norm_scale(csrv, nz, H, 64, dev) if norm else None
        ed, rd, fd = (torch.from_numpy(a).to(dev) for a in (el, er, ft))
        o2 = torch.empty(n, H, F, device=dev)
        stats = torch.empty(n, 2 * H, device=dev)
        ops._gat_fwd_into(csrv, csrv.plan(64, need=True), ed, rd, fd, H, F, 0.2, sp, nscale, None, o2, stats, dev)
        d_el, d_er, d_ft, _ = ops._gat_bwd_fused(csrv, csrt, ed, rd, fd, stats, Gd, o2, H, F, 0.2, sp, nscale, False, 64, dev, None,
                                                 spec_tensors=(nz.p0, nz.p1, nz.epoch))
        assert_gat_grads_vs_oracle(oracle, og, el, er, ft, G, spec, [d_el, d_er, d_ft], what=f"{what} whole", dev=dev)
        S_el, S_er, S_ft = torch.empty(n, H, device=dev), torch.empty(n, H, device=dev), torch.empty(n, H * F, device=dev)
        st = ops._GatBwdStages(csrv, csrt, ed, rd, fd, stats, Gd, o2, H, F, 0.2, sp, nscale, None, 64, S_el, S_er, S_ft, dev)
        st.rowdot()
        st.source()
        st.der()
        assert torch.equal(S_el, d_el) and torch.equal(S_er, d_er) and torch.equal(S_ft, d_ft.reshape(n, -1)), f"{what} stages"
    # attention dropout: the mask's own stream (seed ^ ATTN_DROP_DOMAIN) at the regime's offset and epoch
    seed, off, ep, _ = REGIMES[regime]
    dseed = seed ^ ATTN_DROP_DOMAIN
    p_drop = 0.4
    keep_prob = float(np.float32(1.0 - p_drop))
    keep = oracle.noise_materialize(og, oracle.make_spec("bernoulli", keep_prob, seed=dseed, offset=okw["offset"],
                                                         pos_base=okw["pos_base"], Dn=H, n_edges=E), H)
    assert abs(float(keep.mean()) - keep_prob) < 0.03
    drop = (p_drop, dseed, off) + (() if ep is None else (kw["epoch"],))
    spec = _ospec(oracle, g, H, "normal", 1.0, 0.5, relu=True, **okw)
    t = t_()
    out = ops.gat_aggregate(g, *t, 0.2, _noise(g, H, "normal", 1.0, 0.5, relu=True, **kw), attn_drop=drop)
    with hw_normals(oracle, dev):
        ref = oracle.gat_fwd(og, el, er, ft, 0.2, spec, keep=keep, keep_prob=keep_prob)
    assert_close(out, ref, what=f"gat {regime} {front} dropout forward")
    out.backward(Gd)
    assert_gat_grads_vs_oracle(oracle, og, el, er, ft, G, spec, [a.grad for a in t], keep=keep, keep_prob=keep_prob,
                               what=f"gat {regime} dropout", dev=dev)
    # vi=True: the parameters' gradients from the kernels (stag_gat_bwd_dp), against dL/dw of the oracle's backward
    p0h, p1h = np.float32(0.9), np.float32(0.6)
    q0 = torch.tensor(0.9, device=dev, requires_grad=True)
    q1 = torch.tensor(0.6, device=dev, requires_grad=True)
    nz = stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, q0, q1, differentiable=True, **kw)
    t = t_()
    ops.gat_aggregate(g, *t, 0.2, nz).backward(Gd)
    with hw_normals(oracle, dev):
        std = oracle.noise_materialize(og, _ospec(oracle, g, H, "normal", 0.0, 1.0, **okw), H).astype(np.float64)
    raw = p0h + p1h * std
    espec = oracle.make_spec("explicit", raw.astype(np.float32))
    d_el, d_er, d_ft, dw = oracle.gat_bwd(og, el, er, ft, G, 0.2, espec, want_dw=True)
    dw = dw.astype(np.float64)
    for got, ref, nm in ((q0.grad, dw.sum(), "d loc"), (q1.grad, (dw * std).sum(), "d scale")):
        sc = max(1.0, float(np.abs(ref)), float(np.abs(dw).max()))
        assert_close(got.cpu().numpy().reshape(()) / sc, np.float64(ref) / sc, what=f"gat {regime} vi {nm}")
    for got, ref, nm in ((t[0].grad, d_el, "d el"), (t[1].grad, d_er, "d er"), (t[2].grad, d_ft, "d ft")):
        sc = max(1.0, float(np.abs(ref).max()))
        assert_close(got / sc, ref.astype(np.float64) / sc, what=f"gat {regime} vi {nm}")


# ---- a dropped high word changes the result --------------------------------------------------------------------
def test_high_words_change_the_draws(dev, front):
    """A kernel and an oracle that both dropped a high word would agree with each other: these pairs differ only in
    one high word (seed, offset, position), so they must give different results."""
    from stag_amd import ops
    g = _graph(dev)
    n = g.number_of_nodes()
    x = torch.randn(n, 128, device=dev)
    el, er, ft = torch.randn(n, 4, device=dev), torch.randn(n, 4, device=dev), torch.randn(n, 4, 16, device=dev)
    pairs = [(dict(seed=9, offset=7), dict(seed=9, offset=2**32 + 7)),
             (dict(seed=0x76543210, offset=3), dict(seed=0xFEDCBA9876543210, offset=3)),
             (dict(seed=9, offset=3, pos_base=17), dict(seed=9, offset=3, pos_base=3 * 2**32 + 17))]
    for a, b in pairs:
        na, nb = (_noise(g, 128, "normal", 1.0, 0.5, **c) for c in (a, b))
        assert not torch.equal(ops.aggregate(g, x, na), ops.aggregate(g, x, nb)), (a, b)
        assert not torch.equal(ops.materialize_noise(g, na), ops.materialize_noise(g, nb)), (a, b)
        assert not torch.equal(ops.aggregate_mc(g, x, na, 4), ops.aggregate_mc(g, x, nb, 4)), (a, b)
        ga, gb = (_noise(g, 4, "normal", 1.0, 0.5, **c) for c in (a, b))
        with torch.no_grad():
            oa, aa = ops.gat_aggregate(g, el, er, ft, 0.2, ga, want_attn=True)
            ob, ab = ops.gat_aggregate(g, el, er, ft, 0.2, gb, want_attn=True)
        assert not torch.equal(oa, ob) and not torch.equal(aa, ab), (a, b)


# ---- Monte-Carlo offsets wrap mod 2^64 in the model ------------------------------------------------------------
def test_model_monte_carlo_offsets_wrap(dev):
    """A two-stochastic-layer model whose generator offset wraps past 2^64 inside one batched Monte-Carlo call: the
    batched first layer gives the plain loop's output bit for bit, batching stays on, and the generator ends at
    (start + S * L) mod 2^64."""
    import stag_amd
    from stag_amd.random import NoiseGenerator
    n, D, S = 300, 24, 4
    g = _graph(dev)
    x = torch.randn(n, D, device=dev)
    N, L, Z = torch.distributions.Normal, stag_amd.layers, stag_amd.zoo
    gen = NoiseGenerator(seed=5)
    torch.manual_seed(1)
    layers = torch.nn.ModuleList([
        L.StagLayer(Z.GCN(D, 16, activation=torch.relu), generator=gen, q_a=N(1.0, 0.5), relu=True),
        L.StagLayer(Z.GCN(16, 5, activation=lambda t: torch.softmax(t, -1)), generator=gen, q_a=N(1.0, 0.3))])
    model = stag_amd.models.StagModel(layers).to(dev).eval()
    per = sum(l.offsets_per_forward() for l in layers)
    assert per == 2
    start = 2**64 - 3
    calls = []
    orig = layers[0].forward_mc

    def counted(*a, **k):
        out = orig(*a, **k)
        calls.append(out is not None)
        return out
    layers[0].forward_mc = counted

    def run(batched):
        model._mc_batching_off = not batched
        gen.set_state({"seed": 5, "offset": start})
        with torch.no_grad():
            return model(g, x, n_samples=S, return_parameters=True)

    plain = run(False)
    assert gen.get_state()["offset"] == (start + S * per) & M64
    batched = run(True)
    assert calls and all(calls), "the batched first layer was not used"
    assert model._mc_batching_off is False
    assert gen.get_state()["offset"] == (start + S * per) & M64
    assert torch.equal(batched, plain)
