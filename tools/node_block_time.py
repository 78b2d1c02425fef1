#!/usr/bin/env python
"""The node block between two layers — FeatOnlyLayer(Sequential(BatchNorm1d(D), ReLU(), Dropout(0.5))), training mode —
as fused HIP passes (ops.node_block: stag_node_norm_stats / _fwd / _bwd) against the torch route (the three modules),
device time in one process, at the shapes the reference's scripts run:
    arxiv [169,343, 128] and [169,343, 256], the PPI batch [56,944, 256], Cora-sized [2,708, 16]
For every shape:
    fwd        the training forward alone, no grad                                              us per call
    fwd+bwd    forward and backward with respect to x, gamma and beta                           us per call
    peak       the peak allocation of one forward + backward over what is resident              MiB
Each of (c) the torch route, (c') the torch route again — the spread between two repeats of one route in the same run —
(f) the fused route and (f') the fused route again; the routes are interleaved so that clock and neighbours drift over
all of them alike; a sample is `--inner` calls between two device events; the table gives the median over `--iters`
samples.  ops.NODE_BLOCK_FUSED may be True only if max(f, f') <= mean(c, c') + |c - c'| for every timed case.  The
outputs and gradients of (f) without dropout are checked against (c)'s first (the two routes draw different masks).

    python tools/node_block_time.py [--iters 20] [--inner 5] [--out FILE] [--shapes arxiv128,cora]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stag_amd  # noqa: E402
from stag_amd import ops  # noqa: E402

SHAPES = [("arxiv128", 169343, 128), ("arxiv256", 169343, 256), ("ppi", 56944, 256), ("cora", 2708, 16)]


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


def scaled(a, b):
    s = max(1.0, float(b.abs().max()))
    return float(((a - b).abs() / s / (1.0 + b.abs() / s)).max())


def make_layer(D, p, dev):
    torch.manual_seed(0)
    block = torch.nn.Sequential(torch.nn.BatchNorm1d(D), torch.nn.ReLU(), torch.nn.Dropout(p))
    with torch.no_grad():
        block[0].weight.uniform_(0.5, 1.5)
        block[0].bias.uniform_(-0.2, 0.2)
    return stag_amd.layers.FeatOnlyLayer(block).to(dev).train()


def one_case(name, n, D, dev, iters, inner, lines):
    """Appends the row of one shape; returns True when (f) meets the rule in every column."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, D, generator=gen).to(dev).requires_grad_(True)
    gout = torch.randn(n, D, generator=gen).to(dev)
    layer = make_layer(D, 0.5, dev)
    params = [x, layer.layer[0].weight, layer.layer[0].bias]

    def fwd(fused):
        def fn():
            ops.NODE_BLOCK_FUSED = fused
            with torch.no_grad():
                return layer(None, x)
        return fn

    def both(fused, lay=layer):
        def fn():
            ops.NODE_BLOCK_FUSED = fused
            for t in (x, lay.layer[0].weight, lay.layer[0].bias):
                t.grad = None
            y = lay(None, x)
            y.backward(gout)
            return y.detach(), x.grad, lay.layer[0].weight.grad, lay.layer[0].bias.grad
        return fn

    plain = make_layer(D, 0.0, dev)                        # the check: without a mask the two routes compute one function
    ref, got = both(False, plain)(), both(True, plain)()
    err = max(scaled(a, b) for a, b in zip(got, ref))
    assert err <= 1e-4, f"{name}: the fused route differs from the torch route by {err:.2e}"
    del ref, got, plain
    cols, ok = [], True
    for make in (fwd, both):
        routes = [make(False), make(False), make(True), make(True)]
        for fn in routes * 2:                                   # warm-up: code objects, the allocator's blocks
            fn()
        torch.cuda.synchronize()
        peaks = (peak_of(routes[0]), peak_of(routes[2]))
        t = timed(routes, iters, inner)
        base, spread = 0.5 * (t[0] + t[1]), abs(t[0] - t[1])
        met = max(t[2], t[3]) <= base + spread
        ok = ok and met
        cols.append((t, met, peaks))
    for t in params:
        t.grad = None
    (tf, mf, _), (tb, mb, pb) = cols
    lines.append(f"  {name:<9s}{n:>8d}{D:>5d} |{tf[0]:8.1f}{tf[1]:8.1f}{tf[2]:8.1f}{tf[3]:8.1f} {'met' if mf else 'MISSED':<7s}|"
                 f"{tb[0]:8.1f}{tb[1]:8.1f}{tb[2]:8.1f}{tb[3]:8.1f} {'met' if mb else 'MISSED':<7s}|{pb[0]:8.1f}{pb[1]:8.1f} | {err:.1e}")
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
        raise SystemExit("node_block_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    shipped = ops.NODE_BLOCK_FUSED
    lines = [f"node block BatchNorm1d + ReLU + Dropout(0.5), training: stag_node_norm_* (f, f again) against the torch route "
             f"(c, c again); device {torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of "
             f"{args.inner} calls",
             f"  {'shape':<9s}{'N':>8s}{'D':>5s} |{'fwd c':>8s}{'c again':>8s}{'f':>8s}{'f again':>8s} {'us':<7s}|"
             f"{'f+b c':>8s}{'c again':>8s}{'f':>8s}{'f again':>8s} {'us':<7s}|{'peak c':>8s}{'f':>8s} | max scaled difference"]
    print("\n".join(lines), flush=True)
    ok = True
    wanted = args.shapes.split(",")
    for name, n, D in SHAPES:
        if name in wanted:
            ok = one_case(name, n, D, dev, args.iters, args.inner, lines) and ok
            torch.cuda.empty_cache()
    ops.NODE_BLOCK_FUSED = shipped
    lines.append(f"rule for ops.NODE_BLOCK_FUSED = True (every case: max(f, f') <= mean(c, c') + |c - c'|): {'met' if ok else 'NOT met'}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
