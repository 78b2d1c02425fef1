#!/usr/bin/env python
"""Half-typed feature rows: stag_agg_fwd_half against the routes it stands beside, device time per ops.aggregate call
(no grad) at the arxiv shape (D = 128) and on the PPI batch (D = 256), for no noise, Bernoulli, Uniform and Normal:
    (a)  fp32 rows                      stag_agg_fwd
    (b)  bf16 rows, the cast route      x.float() + stag_agg_fwd          (ops.HALF_ROWS = False)
    (b') the same again: the spread between two repeats of one route in the same run
    (c)  bf16 rows as they are          stag_agg_fwd_half                 (ops.HALF_ROWS = True)
    (c') fp16 rows as they are          stag_agg_fwd_half
One process; the routes are interleaved (a, b, b', c, c', a, ...) so that clock and neighbours drift over all of them
alike; a sample is `--inner` calls between two device events; the table gives the median over `--iters` samples.
The last column compares (c) with (b): ops.HALF_ROWS may default to True only if (c) is not slower than (b) by more
than |b - b'| for every kind at the arxiv shape.  Outputs of (c) are checked against (b)'s before anything is timed.

    python tools/half_rows_time.py [--iters 30] [--inner 10] [--out FILE] [--arxiv-only]
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

KINDS = (("none", None), ("bernoulli", (_lib.NOISE_BERNOULLI, 0.7, None)), ("uniform", (_lib.NOISE_UNIFORM, 0.2, 1.8)),
         ("normal", (_lib.NOISE_NORMAL, 1.0, 0.5)))


def shape_rows(name, g, D, dev, iters, inner, lines):
    """Appends the table of one shape; returns True when (c) meets the rule for every kind."""
    N = g.number_of_nodes()
    torch.manual_seed(0)
    x32 = torch.randn(N, D, device=dev)
    xb, xh = x32.to(torch.bfloat16), x32.to(torch.float16)
    lines.append(f"{name}: N = {N}, E = {g.number_of_edges()}, D = {D}; us per call")
    lines.append(f"  {'kind':<10s}{'(a) fp32':>10s}{'(b) cast':>10s}{'(b) again':>10s}{'(c) bf16':>10s}{'(c) fp16':>10s}"
                 f"{'c/a':>7s}{'c - b':>8s}{'|b - b|':>8s}  rule")
    all_ok = True
    for kname, par in KINDS:
        noise = None if par is None else stag_amd.EdgeNoise(g, D, par[0], par[1], par[2], seed=5, offset=1)

        def route(x, half):
            def fn():
                ops.HALF_ROWS = half
                return ops.aggregate(g, x, noise)
            return fn
        routes = [route(x32, False), route(xb, False), route(xb, False), route(xb, True), route(xh, True)]
        with torch.no_grad():
            outs = [fn() for fn in routes]                     # warm-up of every route: plans, code objects
            outs = [fn() for fn in routes]
            torch.cuda.synchronize()
            # same result before any timing: the half kernel against the cast route on the same rows and draws
            err = float(((outs[3] - outs[1]).abs() / (1 + outs[1].abs())).max())
            assert err <= 1e-5, f"{name} {kname}: stag_agg_fwd_half differs from the cast route by {err:.2e}"
            del outs
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
        ta, tb, tb2, tc, tch = (float(np.median(s)) for s in samples)
        spread = abs(tb - tb2)
        ok = tc <= 0.5 * (tb + tb2) + spread               # (b) = the mean of its two repeats
        all_ok = all_ok and ok
        lines.append(f"  {kname:<10s}{ta:10.1f}{tb:10.1f}{tb2:10.1f}{tc:10.1f}{tch:10.1f}{tc / ta:7.2f}"
                     f"{tc - 0.5 * (tb + tb2):8.1f}{spread:8.1f}"
                     f"  {'met' if ok else 'MISSED'}   (max scaled difference of (c) from (b): {err:.1e})")
        print(lines[-1], flush=True)
    ops.HALF_ROWS = False
    return all_ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--arxiv-only", action="store_true", help="the arxiv shape only (a profiler capture)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("half_rows_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = [f"half-typed rows: stag_agg_fwd_half against fp32 rows and the cast route; device "
             f"{torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of {args.inner} calls"]
    src, dst = synthetic.arxiv_like()
    n = int(max(src.max(), dst.max())) + 1
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    ok = shape_rows("arxiv", g, 128, dev, args.iters, args.inner, lines)
    lines.append(f"rule for ops.HALF_ROWS = True at the arxiv shape (every kind: (c) <= (b) + |b - b'|): "
                 f"{'met' if ok else 'NOT met'}")
    if not args.arxiv_only:
        s, d, sizes = synthetic.ppi_like()
        gp = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                            batch_num_nodes=torch.from_numpy(sizes), device=dev)
        shape_rows("ppi batch", gp, 256, dev, args.iters, args.inner, lines)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
