#!/usr/bin/env python
"""The sample-based KL fallback against a mixture prior (stag/layers.py:141-143): stag_sample_kl against the composed
route (EdgeNoise.materialize(), both log_probs as eager torch, autograd through the [E, D] sample).

    StagLayer(zoo.GCN(128, 128), q_a, p_a = a 2-component MixtureSameFamily of Normals, vi=True)
on the arxiv-shaped graph of bench.py (N = 169,343, E = 1,166,243), for q_a = Normal(1, 0.5) (learned scalars, a
per-channel row in the kernels) and q_a = AmortizedDistribution(128, 1) ([E, 1] heads, log-scale).  A step is
forward + kl_divergence() + backward of (out.square().mean() + kl).  Per configuration:
    (a)  ops.SAMPLED_KL_FUSED = False      the composed route: what the parent of this change ran
    (a') the same again: the spread between two repeats of one route in the same run
    (b)  ops.SAMPLED_KL_FUSED = True       stag_sample_kl
One process; the routes are interleaved (a, a', b, a, ...) so that clock and neighbours drift over all of them alike; a
sample is `--inner` steps between two device events; the table gives the median over `--iters` samples, and the peak of
torch.cuda.max_memory_allocated over one step of each route (above what is allocated before the step); `kl call` is the
stag_sample_kl call alone (value and both gradients, us) on the descriptor of one forward.  Before timing,
the two routes' values and parameter gradients are compared.  If the composed route does not fit in memory at the full
graph, that is recorded and both are timed on the first quarter of the edges.  The last line applies the rule for the
default of the switch: True unless (b) measures slower than (a).

    python tools/sample_kl_time.py [--iters 20] [--inner 5] [--out FILE]
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

D = 128


def timed(routes, iters, inner):
    """Median device time (us per step) of every route, interleaved."""
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


def mixture(dev):
    M = torch.distributions
    return M.MixtureSameFamily(M.Categorical(torch.tensor([0.3, 0.7], device=dev)),
                               M.Normal(torch.tensor([0.0, 1.0], device=dev), torch.tensor([0.5, 0.8], device=dev)))


def make_layer(which, dev):
    torch.manual_seed(0)
    q_a = (torch.distributions.Normal(1.0, 0.5) if which == "normal"
           else stag_amd.distributions.AmortizedDistribution(D, 1))
    return stag_amd.layers.StagLayer(stag_amd.zoo.GCN(D, D), q_a=q_a, p_a=mixture(dev), vi=True).to(dev)


def make_step(layer, g, x, fused):
    def fn():
        ops.SAMPLED_KL_FUSED = fused
        for p in layer.parameters():
            p.grad = None
        stag_amd.manual_seed(7)            # the same draw on every route: the values can be compared
        out = layer(g, x)
        kl = layer.kl_divergence()
        (out.square().mean() + kl).backward()
        layer._edge_weight_handle = None   # (the composed route leaves its [E, D] sample there)
        return kl.detach()
    return fn


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def one_config(which, g, x, dev, iters, inner, lines):
    """One row of the table; None if the composed route ran out of memory."""
    layer = make_layer(which, dev)
    off, off2, on = make_step(layer, g, x, False), make_step(layer, g, x, False), make_step(layer, g, x, True)
    try:
        kl_off = off()
        g_off = [p.grad.clone() for p in layer.parameters() if p.grad is not None]
        kl_on = on()
        g_on = [p.grad.clone() for p in layer.parameters() if p.grad is not None]
        for fn in (off, off2, on):
            fn()
        torch.cuda.synchronize()
        mem_off, mem_on = peak_of(off), peak_of(on)
        t_off, t_off2, t_on = timed([off, off2, on], iters, inner)
        # the stag_sample_kl call alone (value and both gradients), on the descriptor of one forward
        ops.SAMPLED_KL_FUSED = True
        with torch.no_grad():
            layer(g, x)
        h = layer._edge_weight_handle
        t_call, = timed([lambda: ops._sample_kl_raw(h, layer.p_a, True)], iters, inner)
        layer._edge_weight_handle = None
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None
    err = max(float(((a - b).abs() / (1.0 + b.abs())).max()) for a, b in zip([kl_on] + g_on, [kl_off] + g_off))
    mean_off, spread = 0.5 * (t_off + t_off2), abs(t_off - t_off2)
    lines.append(f"  {which:<10s}{t_off:10.1f}{t_off2:10.1f}{t_on:10.1f}{t_on / mean_off:8.2f}{spread:9.1f}"
                 f"{mem_off:11.1f}{mem_on:11.1f}{t_call:9.1f}   {err:.1e}")
    print(lines[-1], flush=True)
    return t_on <= mean_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_kl_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    default = ops.SAMPLED_KL_FUSED
    lines = [f"sample-based KL against a 2-component mixture prior: stag_sample_kl against the composed route; device "
             f"{torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of {args.inner} steps"]
    src, dst = synthetic.arxiv_like(seed=1)
    n = int(max(src.max(), dst.max())) + 1
    results = []
    for frac in (1, 4):
        E = len(src) // frac
        g = stag_amd.Graph(torch.from_numpy(src[:E]), torch.from_numpy(dst[:E]), n, device=dev)
        torch.manual_seed(1)
        x = torch.randn(n, D, device=dev)
        lines.append(f"StagLayer(zoo.GCN({D}, {D}), vi=True), N = {n}, E = {E}" + (" (the first quarter of the edges)" if frac > 1 else "")
                     + f"; one [E, D] fp32 tensor is {E * D * 4 / 2 ** 20:.0f} MiB; step = forward + kl_divergence() + backward")
        lines.append(f"  {'q_a':<10s}{'(a) off':>10s}{'(a) again':>10s}{'(b) on':>10s}{'b / a':>8s}{'|a - a|':>9s}"
                     f"{'peak a MiB':>11s}{'peak b MiB':>11s}{'kl call':>9s}   max scaled |b - a| of kl and parameter gradients")
        print("\n".join(lines[-2:]), flush=True)
        results = [one_config(which, g, x, dev, args.iters, args.inner, lines) for which in ("normal", "amortized")]
        if None not in results:
            break
        lines.append("  the composed route ran out of memory at this size")
        del g, x
        torch.cuda.empty_cache()
    ops.SAMPLED_KL_FUSED = default
    if None in results:
        lines.append("the composed route did not fit at either size: nothing to compare")
    else:
        lines.append("rule for ops.SAMPLED_KL_FUSED = True (the fused step not slower than the composed one, every q_a): "
                     + ("met" if all(results) else "NOT met"))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
