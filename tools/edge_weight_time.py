#!/usr/bin/env python
"""One weight per edge (noise width 1 on rows of width D): stag_agg_fwd_w1 against the routes it stands beside, device
time per ops.aggregate call (no grad) at the arxiv shape (D = 128) and on the PPI batch (D = 256):
    stag_agg_fwd without noise, with a per-channel Normal draw, with a per-channel Bernoulli(0.5) draw   (the scale)
    for Normal, Uniform, Bernoulli at keep 0.9 / 0.5 / 0.1 and explicit [E, 1] weights:
      (t)  the two-launch route: stag_noise_materialize at width 1, stag_agg_fwd EXPLICIT with group = D — the baseline
      (t') the same again: the spread between two repeats of one route in the same run
      (f)  stag_agg_fwd_w1
      further columns: stag_agg_fwd_w1 of build variants of the library (--lib NAME=PATH, tools/ab_bench.py build), e.g.
           noskip = -DSTAG_W1_NO_SKIP=1, which multiplies by zero weights instead of skipping their rows
    explicit [E, 1] weights expanded to a contiguous [E, D] copy, the copy included                      (the old route)
    one StagLayer(GCN 128 -> 128) training step, Bernoulli(0.5) + norm=True, at sample_dimension 128 and 1
One process; the routes of a kind are interleaved so that clock and neighbours drift over all of them alike; a sample is
`--inner` calls between two device events; the table gives the median over `--iters` samples.  ops.EDGE_WEIGHT_FUSED may
be True only if (f) <= mean(t, t') + |t - t'| for every kind timed.  Outputs of (f) are checked against (t)'s first.

    python tools/edge_weight_time.py [--iters 30] [--inner 10] [--out FILE] [--lib noskip=tools/_bin/libstag_w1noskip.so]
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

KINDS = (("normal", (_lib.NOISE_NORMAL, 1.0, 0.5)), ("uniform", (_lib.NOISE_UNIFORM, 0.2, 1.8)),
         ("bern 0.9", (_lib.NOISE_BERNOULLI, 0.9, None)), ("bern 0.5", (_lib.NOISE_BERNOULLI, 0.5, None)),
         ("bern 0.1", (_lib.NOISE_BERNOULLI, 0.1, None)), ("explicit", None))


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


def shape_rows(name, g, D, dev, iters, inner, lines, variants):
    """Appends the tables of one shape; returns True when (f) meets the rule for every kind."""
    N, E = g.number_of_nodes(), g.number_of_edges()
    torch.manual_seed(0)
    x = torch.randn(N, D, device=dev)
    w1 = torch.rand(E, 1, device=dev)
    shipped = _lib.lib()

    def route(weight, fused=False, tensors=True, lib=None):
        def fn():
            ops.EDGE_WEIGHT_FUSED, ops.EDGE_WEIGHT_TENSORS = fused, tensors
            _lib._lib = lib if lib is not None else shipped
            try:
                return ops.aggregate(g, x, weight)
            finally:
                _lib._lib = shipped
        return fn

    lines.append(f"{name}: N = {N}, E = {E}, D = {D}; us per call")
    with torch.no_grad():
        scale = [route(None), route(stag_amd.EdgeNoise(g, D, _lib.NOISE_NORMAL, 1.0, 0.5, seed=5, offset=1)),
                 route(stag_amd.EdgeNoise(g, D, _lib.NOISE_BERNOULLI, 0.5, None, seed=5, offset=1)),
                 route(w1, tensors=False)]
        for fn in scale * 2:
            fn()
        torch.cuda.synchronize()
        t = timed(scale, iters, inner)
        lines.append(f"  stag_agg_fwd: no noise {t[0]:.1f}; per-channel Normal {t[1]:.1f}; per-channel Bernoulli(0.5) {t[2]:.1f}; "
                     f"[E, 1] weights expanded to [E, D], copy included {t[3]:.1f}")
        print(lines[-1], flush=True)
        lines.append(f"  {'kind':<10s}{'(t) two':>10s}{'(t) again':>10s}{'(f) fused':>10s}"
                     + "".join(f"{nm:>10s}" for nm, _ in variants) + f"{'f - t':>8s}{'|t - t|':>8s}  rule")
        all_ok = True
        for kname, par in KINDS:
            weight = w1 if par is None else stag_amd.EdgeNoise(g, 1, par[0], par[1], par[2], seed=5, offset=1)
            routes = [route(weight), route(weight), route(weight, fused=True)]
            routes += [route(weight, fused=True, lib=lb) for _, lb in variants]
            outs = [fn() for fn in routes]                     # warm-up of every route: plans, code objects
            outs = [fn() for fn in routes]
            torch.cuda.synchronize()
            err = float(((outs[2] - outs[0]).abs() / (1 + outs[0].abs())).max())
            # (two fp32 sums of up to 13,000 terms in different block orders, each held to 1e-5 of the exact sum)
            assert err <= 2e-5, f"{name} {kname}: stag_agg_fwd_w1 differs from the two-launch route by {err:.2e}"
            for (nm, _), o in zip(variants, outs[3:]):      # (the skip, the rows in flight: no bit changes on finite rows)
                assert torch.equal(o, outs[2]), f"{name} {kname}: build variant {nm} gives other bits"
            del outs
            t = timed(routes, iters, inner)
            spread = abs(t[0] - t[1])
            base = 0.5 * (t[0] + t[1])
            ok = t[2] <= base + spread
            all_ok = all_ok and ok
            ns = "".join(f"{v:10.1f}" for v in t[3:])
            lines.append(f"  {kname:<10s}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}{ns}{t[2] - base:8.1f}{spread:8.1f}"
                         f"  {'met' if ok else 'MISSED'}   (max scaled difference of (f) from (t): {err:.1e})")
            print(lines[-1], flush=True)
    return all_ok


def layer_rows(g, dev, iters, lines):
    """One training step of StagLayer(GCN 128 -> 128), Bernoulli(0.5) + norm=True: forward, loss, backward; ms per step."""
    from stag_amd import layers, zoo
    torch.manual_seed(0)
    x = torch.randn(g.number_of_nodes(), 128, device=dev)

    def step_of(sd, fused):
        layer = layers.StagLayer(zoo.GCN(128, 128), q_a=torch.distributions.Bernoulli(0.5), norm=True).to(dev)
        if sd is not None:
            layer.base_layer.sample_dimension = sd

        def fn():
            ops.EDGE_WEIGHT_FUSED = fused
            layer.zero_grad(set_to_none=True)
            layer(g, x).square().mean().backward()
        return fn
    steps = [step_of(None, False), step_of(1, False), step_of(1, False), step_of(1, True)]
    stag_amd.manual_seed(7)
    for fn in steps * 2:
        fn()
    torch.cuda.synchronize()
    peaks = []
    for fn in steps:
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks.append((torch.cuda.max_memory_allocated() - torch.cuda.memory_allocated()) / 2 ** 20)
    t = [v / 1e3 for v in timed(steps, iters, 3)]
    lines.append("StagLayer(GCN 128 -> 128), Bernoulli(0.5) + norm=True, arxiv: one training step, ms (peak MiB over the resident set)")
    lines.append(f"  sample_dimension 128: {t[0]:.3f} ({peaks[0]:.0f}); sample_dimension 1, two-launch route: {t[1]:.3f}, again "
                 f"{t[2]:.3f} ({peaks[1]:.0f}); sample_dimension 1, stag_agg_fwd_w1: {t[3]:.3f} ({peaks[3]:.0f})")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH",
                    help="a build variant of the library whose stag_agg_fwd_w1 is timed beside the shipped one (tools/ab_bench.py build)")
    ap.add_argument("--arxiv-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_weight_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    shipped_switch = (ops.EDGE_WEIGHT_FUSED, ops.EDGE_WEIGHT_TENSORS)
    variants = [(v.partition("=")[0], _lib.bind(v.partition("=")[2])) for v in args.lib]
    lines = [f"one weight per edge: stag_agg_fwd_w1 against the two-launch route; device {torch.cuda.get_device_name(0)}; "
             f"interleaved, median of {args.iters} samples of {args.inner} calls"]
    src, dst = synthetic.arxiv_like()
    n = int(max(src.max(), dst.max())) + 1
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    ok = shape_rows("arxiv", g, 128, dev, args.iters, args.inner, lines, variants)
    if not args.arxiv_only:
        s, d, sizes = synthetic.ppi_like()
        gp = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                            batch_num_nodes=torch.from_numpy(sizes), device=dev)
        ok = shape_rows("ppi batch", gp, 256, dev, args.iters, args.inner, lines, variants) and ok
    lines.append(f"rule for ops.EDGE_WEIGHT_FUSED = True (every kind at every shape: (f) <= mean(t, t') + |t - t'|): "
                 f"{'met' if ok else 'NOT met'}")
    layer_rows(g, dev, args.iters, lines)
    ops.EDGE_WEIGHT_FUSED, ops.EDGE_WEIGHT_TENSORS = shipped_switch
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
