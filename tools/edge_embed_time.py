#!/usr/bin/env python
"""The wide edge embedding h = SiLU(p_src[src] + p_dst[dst]) of an AmortizedDistribution(in, out > 1): stag_edge_embed_fwd /
_bwd (ops.edge_embed) against the composed route (two gathers, an add, a SiLU; two aggregations of explicit rows behind
SiLU's backward), device time in one process, at the shapes the reference's citation_rec scripts run:
    Cora-sized (hidden 1433 and 16), Pubmed-sized (hidden 500), the PPI batch (hidden 50), arxiv-shaped (hidden 128)
For every shape:
    fwd        the forward alone, no grad                                                       us per call
    fwd+bwd    forward and backward with respect to both [N, hidden] tables                     us per call
    peak       the peak allocation of one forward + backward over what is resident              MiB
    layer      one training step of StagLayer(GCN(hidden, hidden), AmortizedDistribution(hidden, hidden), vi=True):
               forward, output gradient and KL, backward                                        ms per step
Each of (c) the composed route, (c') the composed route again — the spread between two repeats of one route in the same
run — (f) the fused route and (f') the fused route again; the routes are interleaved so that clock and neighbours drift
over all of them alike; a sample is `--inner` calls between two device events; the table gives the median over `--iters`
samples.  ops.EDGE_EMBED_FUSED may be True only if max(f, f') <= mean(c, c') + |c - c'| for every timed case.  The
outputs and gradients of (f) are checked against (c)'s first.

    python tools/edge_embed_time.py [--iters 20] [--inner 5] [--out FILE] [--shapes cora,arxiv]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stag_amd  # noqa: E402
from stag_amd import ops, synthetic  # noqa: E402


def timed(routes, iters, inner):
    """Median us per call of every route, interleaved."""
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


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def uniform_graph(n, e, seed, dev):
    """n nodes, e uniformly drawn edges and one self loop per node (the scripts' add_self_loop)."""
    gen = torch.Generator().manual_seed(seed)
    loop = torch.arange(n)
    return stag_amd.Graph(torch.cat([torch.randint(0, n, (e,), generator=gen), loop]),
                          torch.cat([torch.randint(0, n, (e,), generator=gen), loop]), n, device=dev)


def arxiv_graph(dev):
    src, dst = synthetic.arxiv_like(seed=1)
    n = int(max(src.max(), dst.max())) + 1
    return stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)


def ppi_graph(dev):
    s, d, sizes = synthetic.ppi_like()
    return stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                          batch_num_nodes=torch.from_numpy(sizes), device=dev)


SHAPES = [("cora", lambda dev: uniform_graph(2708, 10556, 1, dev), (1433, 16)),
          ("pubmed", lambda dev: uniform_graph(19717, 88648, 2, dev), (500,)),
          ("ppi", ppi_graph, (50,)),
          ("arxiv", arxiv_graph, (128,))]


def composed(g, ps, pd):
    return torch.nn.functional.silu(ops.gather_rows(g, ps, "src") + ops.gather_rows(g, pd, "dst"))


def scaled(a, b):
    s = max(1.0, float(b.abs().max()))
    return float(((a - b).abs() / s / (1.0 + b.abs() / s)).max())


def one_case(name, g, hidden, dev, iters, inner, lines):
    """Appends the row of one (shape, hidden); returns True when (f) meets the rule in every column."""
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(3)
    ps = torch.randn(n, hidden, generator=gen).to(dev).requires_grad_(True)
    pd = torch.randn(n, hidden, generator=gen).to(dev).requires_grad_(True)
    gout = torch.randn(E, hidden, generator=gen).to(dev)

    def fwd(fused):
        def fn():
            with torch.no_grad():
                return ops.edge_embed(g, ps, pd) if fused else composed(g, ps, pd)
        return fn

    def both(fused):
        def fn():
            ps.grad = pd.grad = None
            h = ops.edge_embed(g, ps, pd) if fused else composed(g, ps, pd)
            h.backward(gout)
            return h.detach(), ps.grad, pd.grad
        return fn

    torch.manual_seed(0)
    D = hidden
    layer = stag_amd.layers.StagLayer(
        stag_amd.zoo.GCN(D, D, allow_zero_in_degree=True),
        q_a=stag_amd.distributions.AmortizedDistribution(D, D, init_like=torch.distributions.Normal(1.0, 0.3)), vi=True).to(dev)
    x = torch.randn(n, D, generator=gen).to(dev)
    yout = torch.randn(n, D, generator=gen).to(dev)
    one = torch.ones((), device=dev)

    def step(fused):
        def fn():
            ops.EDGE_EMBED_FUSED = fused
            layer.zero_grad(set_to_none=True)
            stag_amd.manual_seed(7)
            y = layer(g, x)
            torch.autograd.backward([y, layer.kl_divergence()], [yout, one])
        return fn

    ref, got = both(False)(), both(True)()
    err = max(scaled(a, b) for a, b in zip(got, ref))
    assert err <= 1e-4, f"{name} hidden {hidden}: the fused route differs from the composed one by {err:.2e}"
    del ref, got
    cols, ok = [], True
    for make, unit in ((fwd, 1.0), (both, 1.0), (step, 1e-3)):
        routes = [make(False), make(False), make(True), make(True)]
        for fn in routes * 2:                                   # warm-up: plans, code objects, the allocator's blocks
            fn()
        torch.cuda.synchronize()
        peaks = (peak_of(routes[0]), peak_of(routes[2]))
        t = [v * unit for v in timed(routes, iters, inner if make is not step else max(1, inner // 2))]
        base, spread = 0.5 * (t[0] + t[1]), abs(t[0] - t[1])
        met = max(t[2], t[3]) <= base + spread
        ok = ok and met
        cols.append((t, spread, met, peaks))
    (tf, sf, mf, _), (tb, sb, mb, pb), (tl, sl, ml, pl) = cols
    lines.append(f"  {name:<7s}{n:>8d}{E:>9d}{hidden:>6d} |{tf[0]:8.1f}{tf[1]:8.1f}{tf[2]:8.1f}{tf[3]:8.1f} {'met' if mf else 'MISSED':<7s}|"
                 f"{tb[0]:8.1f}{tb[1]:8.1f}{tb[2]:8.1f}{tb[3]:8.1f} {'met' if mb else 'MISSED':<7s}|{pb[0]:8.1f}{pb[1]:8.1f} |"
                 f"{tl[0]:8.3f}{tl[1]:8.3f}{tl[2]:8.3f}{tl[3]:8.3f} {'met' if ml else 'MISSED':<7s}|{pl[0]:8.1f}{pl[1]:8.1f} | {err:.1e}")
    print(lines[-1], flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_embed_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    shipped = ops.EDGE_EMBED_FUSED
    lines = [f"wide edge embedding: stag_edge_embed_fwd / _bwd (f, f again) against the composed route (c, c again); device "
             f"{torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of {args.inner} calls",
             f"  {'shape':<7s}{'N':>8s}{'E':>9s}{'hid':>6s} |{'fwd c':>8s}{'c again':>8s}{'f':>8s}{'f again':>8s} {'us':<7s}|"
             f"{'f+b c':>8s}{'c again':>8s}{'f':>8s}{'f again':>8s} {'us':<7s}|{'peak c':>8s}{'f':>8s} |"
             f"{'layer c':>8s}{'c again':>8s}{'f':>8s}{'f again':>8s} {'ms':<7s}|{'peak c':>8s}{'f':>8s} | max scaled difference"]
    print("\n".join(lines), flush=True)
    ok = True
    wanted = args.shapes.split(",")
    for name, make, widths in SHAPES:
        if name not in wanted:
            continue
        g = make(dev)
        for hidden in widths:
            ok = one_case(name, g, hidden, dev, args.iters, args.inner, lines) and ok
        del g
        torch.cuda.empty_cache()
    ops.EDGE_EMBED_FUSED = shipped
    lines.append(f"rule for ops.EDGE_EMBED_FUSED = True (every case: max(f, f') <= mean(c, c') + |c - c'|): {'met' if ok else 'NOT met'}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
