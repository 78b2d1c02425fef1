#!/usr/bin/env python
"""The max reducer (DGL's fn.max; GraphSAGE 'pool'): the fused route (stag_agg_max_fwd / _bwd) against the composed one
(messages formed, scatter-amax; ops.FUSED_MAX = False), device time and peak allocated memory of
    fwd      ops.aggregate_max with x.requires_grad (cnt written, autograd node kept)
    fwd+bwd  the same and its backward
    step     a StagLayer(GraphSAGE(pool), Normal noise) training step (forward, backward, SGD)
at the arxiv shape (D = 128, Normal per edge per channel) and on the PPI batch of BASELINE configs[2] (D = 256, 50),
plus stag_agg_fwd (ops.aggregate, sum) at the same shape for scale.

    python tools/max_reducer_time.py [--iters 20] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stag_amd  # noqa: E402
from stag_amd import _lib, ops, synthetic  # noqa: E402


def timed(fn, iters):
    """(median device ms per call, peak allocated MB above the baseline)."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), peak


def shape_rows(name, g, D, dev, iters, lines, routes=(True, False)):
    N = g.number_of_nodes()
    torch.manual_seed(0)
    x = torch.randn(N, D, device=dev, requires_grad=True)
    noise = stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.3, seed=5, offset=1)
    gout = torch.randn(N, D, device=dev)
    base = stag_amd.zoo.GraphSAGE(D, D, aggregator_type="pool").to(dev)
    layer = stag_amd.layers.StagLayer(base, q_a=torch.distributions.Normal(1.0, 0.3)).to(dev)
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)
    xs = x.detach()

    def fwd():
        ops.aggregate_max(g, x, noise)

    def fwd_bwd():
        ops.aggregate_max(g, x, noise).backward(gout)

    def step():
        opt.zero_grad(set_to_none=True)
        layer(g, xs).square().mean().backward()
        opt.step()

    def agg_sum():
        with torch.no_grad():
            ops.aggregate(g, xs, noise)

    lines.append(f"{name}: N = {N}, E = {g.number_of_edges()}, D = {D}")
    t, m = timed(agg_sum, iters)
    lines.append(f"  stag_agg_fwd (sum, same noise, no grad)      {t:9.3f} ms  peak {m:9.1f} MB")
    for fused in routes:
        ops.FUSED_MAX = fused
        tag = "fused   " if fused else "composed"
        for what, fn in (("fwd", fwd), ("fwd+bwd", fwd_bwd), ("StagLayer(pool) step", step)):
            x.grad = None
            t, m = timed(fn, iters)
            lines.append(f"  {tag} {what:<36s}{t:9.3f} ms  peak {m:9.1f} MB")
    ops.FUSED_MAX = True
    print("\n".join(lines[-8:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused-only", action="store_true", help="the fused route at the arxiv shape only (a profiler capture)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"max reducer, fused vs composed; device {torch.cuda.get_device_name(0)}; median of {args.iters} calls"]
    src, dst = synthetic.arxiv_like()
    n = int(max(src.max(), dst.max())) + 1
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    if args.fused_only:
        shape_rows("arxiv", g, 128, dev, args.iters, lines, routes=(True,))
        return
    shape_rows("arxiv", g, 128, dev, args.iters, lines)
    s, d, sizes = synthetic.ppi_like()
    gp = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                        batch_num_nodes=torch.from_numpy(sizes), device=dev)
    for D in (256, 50):
        shape_rows("ppi batch", gp, D, dev, args.iters, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
