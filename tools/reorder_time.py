#!/usr/bin/env python
"""reorder_graph: what the renumbering costs and what it buys, on one large graph.

Two graphs at the arxiv shape (N = 169,343, E = 1,166,243):
    planted   a planted-partition multigraph, 40 communities, p_in = 0.85, a 13,000-edge hub row, ids scrambled — the
              structure of the graphs the reference trains on (communities, arbitrary ids);
    uniform   synthetic.arxiv_like(): uniform sources, where a reordering has nothing to find (reported as such).
For each: the cost of reorder_graph("locality") — its library part (stag_reorder_locality), the relabelled graph's two
CSR builds with their keying, the two plan builds — as host wall time around a device synchronisation (median of
--reps); the stripe locality before and after; then device time per call, median over --iters samples of --inner calls
between two device events, the routes INTERLEAVED in one process so that clocks and neighbours drift over all alike:
    (s)  the scrambled graph
    (o)  reordered, noise="original"   (csr.nidx set: the general kernel)
    (w)  reordered, noise="own"        (csr.nidx None: the plain launch stays eligible); (o) - (w) is the price of nidx
    (s') the scrambled graph again: the spread between two repeats of one route in the same run
for ops.aggregate at D = 128 and 256 without noise and with Normal noise, the GAT 8 x 32 forward, and one GCN
training step (two StagLayer(GCN) layers, loss, backward).  Every route is warmed past XCD_AFTER_LAUNCHES first, so a
graph that qualifies for the XCD-aware order has it.  Outputs of (o) are checked bit for bit against (s) before timing.

    python tools/reorder_time.py [--iters 20] [--inner 5] [--reps 5] [--out FILE] [--planted-only]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stag_amd  # noqa: E402
from stag_amd import _lib, ops, synthetic  # noqa: E402
gm = importlib.import_module("stag_amd.graph")  # (stag_amd.graph the attribute is the constructor function)

N_ARXIV, E_ARXIV = 169_343, 1_166_243


def planted_edges(n=N_ARXIV, e=E_ARXIV, k=40, p_in=0.85, hub=13_000, seed=0):
    """(src, dst): every node gets a community uniformly at random (ids carry no structure), every edge a uniform
    destination and, with probability p_in, a source from the destination's community, else a uniform one; the first
    `hub` edges are redirected into one row."""
    rng = np.random.default_rng(seed)
    comm = rng.integers(0, k, n)
    dst = rng.integers(0, n, e)
    src = rng.integers(0, n, e)
    inside = rng.random(e) < p_in
    for c in range(k):
        members = np.nonzero(comm == c)[0]
        sel = inside & (comm[dst] == c)
        if len(members) and sel.any():
            src[sel] = rng.choice(members, int(sel.sum()))
    dst[:hub] = int(rng.integers(0, n))
    return src, dst


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def interleaved(routes, iters, inner, warm):
    for fn in routes:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    samples = [[] for _ in routes]
    for _ in range(iters):
        for i, fn in enumerate(routes):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            samples[i].append(a.elapsed_time(b) * 1e3 / inner)
    return [float(np.median(s)) for s in samples]


def row(label, routes, args, inner=None):
    """One table line: (s), (o), (w) and (s) again — the spread between two repeats of one route in the same run."""
    ts, to, tw, ts2 = interleaved(list(routes) + [routes[0]], args.iters, inner or args.inner, gm.XCD_AFTER_LAUNCHES + 4)
    return f"  {label:<34s}{ts:14.1f}{to:14.1f}{tw:10.1f}{to / ts:7.2f}{to - tw:8.1f}{abs(ts - ts2):9.1f}"


def fresh(g):
    """g's edge list as a new graph: no views, no plans."""
    return stag_amd.Graph(g._src, g._dst, g.number_of_nodes(), _trusted=True)


def report(name, src, dst, n, dev, args, lines):
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    g.csr, g.csr_t                                             # the original's views exist before anything is timed
    out = lambda s: (lines.append(s), print(s, flush=True))
    out(f"{name}: N = {n}, E = {g.number_of_edges()}")
    stag_amd.reorder_graph(g, "locality")                       # warm-up: code objects, rocPRIM
    t_all = wall_ms(lambda: stag_amd.reorder_graph(g, "locality"), args.reps)
    t_lib = wall_ms(lambda: gm._locality_perm(g, 16, 8, 0), args.reps)
    g2 = stag_amd.reorder_graph(g, "locality")
    t_csr = wall_ms(lambda: gm._original_keying(g, fresh(g2)), args.reps)

    def plans():
        f = fresh(g2)
        f.csr.plan(gm.DEFAULT_SEG_LEN, need=True), f.csr_t.plan(gm.DEFAULT_SEG_LEN, need=True)
    t_views = wall_ms(plans, args.reps)
    out(f"  reorder_graph('locality', dims=16, rounds=8): {t_all:.2f} ms; stag_reorder_locality {t_lib:.2f} ms; the two CSR "
        f"builds with their keying {t_csr:.2f} ms; (CSR builds + both plans of a fresh graph: {t_views:.2f} ms)")
    own = stag_amd.reorder_graph(g, "locality", noise="own")
    out(f"  stripe locality: scrambled {g.csr.stripe_locality():.3f}; reordered csr {g2.csr.stripe_locality():.3f}, "
        f"csr_t {g2.csr_t.stripe_locality():.3f}")
    torch.manual_seed(0)
    graphs = (g, g2, own)
    with torch.no_grad():
        out(f"  {'launch (us per call)':<34s}{'(s) scrambled':>14s}{'(o) original':>14s}{'(w) own':>10s}{'o/s':>7s}{'o - w':>8s}{'|s - s|':>9s}")
        for D in (128, 256):
            x = torch.randn(n, D, device=dev)
            xs = (x, g2.rows_from_original(x).contiguous(), own.rows_from_original(x).contiguous())
            for kind in ("none", "normal"):
                ws = [None if kind == "none" else stag_amd.EdgeNoise(gr, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=5, offset=1)
                      for gr in graphs]
                routes = [(lambda gr=gr, xi=xi, w=w: ops.aggregate(gr, xi, w)) for gr, xi, w in zip(graphs, xs, ws)]
                outs = [fn() for fn in routes]
                assert torch.equal(g2.rows_to_original(outs[1]), outs[0]), "noise='original' must return the original's bits"
                del outs
                out(row('aggregate D=%d %s' % (D, kind), routes, args))
        H, F = 8, 32
        el, er, ft = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev), torch.randn(n, H, F, device=dev)
        routes = []
        for gr in graphs:
            to_ = (lambda t: t) if gr is g else (lambda t, gr=gr: gr.rows_from_original(t).contiguous())
            a = (to_(el), to_(er), to_(ft))
            w = stag_amd.EdgeNoise(gr, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=5, offset=1)
            routes.append(lambda gr=gr, a=a, w=w: ops.gat_aggregate(gr, a[0], a[1], a[2], 0.2, w))
        out(row('GAT 8 x 32 forward, Normal', routes, args))
        xcd = [bool(gr.csr._plans.get(gm.DEFAULT_SEG_LEN, {}).get("xcd_on")) for gr in graphs]
    # one GCN training step: two StagLayer(GCN) layers, softmax head, loss, backward
    L, Z = stag_amd.layers, stag_amd.zoo
    D, C = 128, 40
    torch.manual_seed(1)
    layers = torch.nn.ModuleList([
        L.StagLayer(Z.GCN(D, 128, activation=torch.relu), q_a=torch.distributions.Normal(1.0, 0.5)),
        L.StagLayer(Z.GCN(128, C), q_a=torch.distributions.Normal(1.0, 0.5)),
        L.FeatOnlyLayer(torch.nn.Softmax(dim=-1))])
    model = stag_amd.models.StagModel(layers).to(dev)
    x = torch.randn(n, D, device=dev)
    y = torch.randint(0, C, (n,), device=dev)
    routes = []
    for gr in graphs:
        xi = x if gr is g else gr.rows_from_original(x).contiguous()
        yi = y if gr is g else gr.rows_from_original(y).contiguous()

        def step(gr=gr, xi=xi, yi=yi):
            model.zero_grad(set_to_none=True)
            model.loss(gr, xi, yi, n_samples=1).backward()
        routes.append(step)
    out(row('GCN training step (2 layers)', routes, args, inner=max(1, args.inner // 2)))
    out(f"  XCD-aware order on (s, o, w): {xcd}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--planted-only", action="store_true", help="the planted graph only (a profiler capture)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reorder_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = [f"reorder_graph: cost and effect; device {torch.cuda.get_device_name(0)}; XCD_ORDER = {gm.XCD_ORDER!r}; launches "
             f"interleaved, median of {args.iters} samples of {args.inner} calls; costs: median of {args.reps} host wall times"]
    print(lines[0], flush=True)
    src, dst = planted_edges()
    report("planted (40 communities, p_in 0.85, 13,000-edge hub, scrambled ids)", src, dst, N_ARXIV, dev, args, lines)
    if not args.planted_only:
        src, dst = synthetic.arxiv_like()
        n = int(max(src.max(), dst.max())) + 1
        report("uniform sources (synthetic.arxiv_like): nothing for a reordering to find", src, dst, n, dev, args, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
