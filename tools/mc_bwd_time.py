#!/usr/bin/env python
"""The backward of a Monte-Carlo batch with respect to amortised per-edge parameters: stag_agg_bwd_w_mc (one pass over the
rows and the parameter tables for the gradients of all S samples) against the per-sample loop it replaces, device time per
backward of S samples at the arxiv shape (D = 128), on the PPI batch (D = 50, 256) and on a Cora-sized synthetic graph
(2,708 nodes, 10,556 edges, D = 1433):
    for Normal with loc / log_scale (p1_log) and Uniform with low / high, S in {2, 4}, heads [E, 1] (_AggregateMCEdge) and
    [E, D] (_AggregateMCPEdge), both parameters live, x without a gradient (the first layer of a model: its input is data):
      (t)  the loop (ops.MC_BWD_FUSED = False): per sample stag_agg_bwd_edge on csr_t ([E, 1], D <= 256), or a g * dvec
           pass + stag_agg_bwd_w + two additions ([E, D]; [E, 1] past D = 256) — the baseline
      (t') the same again: the spread between two repeats of one route in the same run
      (f)  the batched call (ops.MC_BWD_FUSED = True), (f') the same again
One process; the forward runs once per case and its graph is kept, so a sample times the backward alone
(torch.autograd.grad with retain_graph); the routes of a case are interleaved so that clock and neighbours drift over all of
them alike; a sample is `--inner` backward passes between two device events; the table gives the median over `--iters`
samples, and the peak allocation of one backward above what was allocated before it.  ops.MC_BWD_FUSED may be True only if
max(f, f') <= mean(t, t') + |t - t'| for every case timed.  Gradients of (f) are checked against (t)'s first.

    python tools/mc_bwd_time.py [--iters 12] [--inner 2] [--out FILE]
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

SAMPLES = (2, 4)
STRIDE = 2          # offsets per sample of a two-layer model
CORA_NODES, CORA_EDGES, CORA_FEATURES = 2708, 10556, 1433


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


def peak_mb(fn):
    """MB allocated at the peak of one call above what was allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kinds(E, W, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    r = lambda: torch.rand(E, W, generator=gen, device=dev)
    return (("normal log", lambda: dict(kind=_lib.NOISE_NORMAL, p0=0.5 + r(), p1=-1.5 + r(), p1_log=True)),
            ("uniform", lambda: dict(kind=_lib.NOISE_UNIFORM, p0=0.2 * r(), p1=1.5 + r(), p1_log=False)))


def shape_rows(name, g, D, dev, iters, inner, lines):
    """Appends the table of one shape; returns the names of the cases that miss the rule."""
    N, E = g.number_of_nodes(), g.number_of_edges()
    torch.manual_seed(0)
    x = torch.randn(N, D, device=dev)
    lines.append(f"{name}: N = {N}, E = {E}, D = {D}; us per backward of S samples, MB at the peak of one")
    lines.append(f"  {'heads':<8s}{'kind':<12s}{'S':>3s}{'(t) loop':>10s}{'(t) again':>10s}{'(f) fused':>10s}{'(f) again':>10s}"
                 f"{'f - t':>9s}{'|t - t|':>8s}{'MB (t)':>9s}{'MB (f)':>9s}  rule")
    missed = []
    for heads, W, mode in (("[E, 1]", 1, _lib.PARAM_PER_EDGE1), ("[E, D]", D, _lib.PARAM_PER_EDGE)):
        for kname, make in kinds(E, W, dev):
            kw = make()                                        # (one kind's two tables at a time)
            p0, p1 = kw["p0"].requires_grad_(True), kw["p1"].requires_grad_(True)
            noise = stag_amd.EdgeNoise(g, D, kw["kind"], p0, p1, p1_log=kw["p1_log"], differentiable=True, seed=5, offset=1)
            assert noise.param_mode == mode
            for S in SAMPLES:
                out = ops.aggregate_mc(g, x, noise, S, STRIDE)
                assert "_AggregateMC" in type(out.grad_fn).__name__, "the forward did not take the batched node"
                G = torch.randn_like(out)

                def route(fused):
                    def fn():
                        ops.MC_BWD_FUSED = fused
                        return torch.autograd.grad(out, (p0, p1), G, retain_graph=True)
                    return fn
                routes = [route(False), route(False), route(True), route(True)]
                outs = [fn() for fn in routes]                 # warm-up of every route: plans, code objects
                outs = [fn() for fn in routes]
                torch.cuda.synchronize()
                err = 0.0
                for i in range(2):                             # against the loop, relative to the largest gradient
                    sc = max(1.0, float(outs[0][i].abs().max()))
                    err = max(err, float((outs[2][i] - outs[0][i]).abs().max()) / sc)
                    assert torch.equal(outs[2][i], outs[3][i]), f"{name} {heads} {kname} S={S}: two calls, different bits"
                assert err <= 2e-5, f"{name} {heads} {kname} S={S}: stag_agg_bwd_w_mc differs from the loop by {err:.2e}"
                del outs
                mb = [peak_mb(routes[0]), peak_mb(routes[2])]
                t = timed(routes, iters, inner)
                spread = abs(t[0] - t[1])
                base = 0.5 * (t[0] + t[1])
                f = max(t[2], t[3])
                ok = f <= base + spread
                if not ok:
                    missed.append(f"{name} D = {D} {heads} {kname} S = {S}")
                lines.append(f"  {heads:<8s}{kname:<12s}{S:3d}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}{t[3]:10.1f}{f - base:9.1f}{spread:8.1f}"
                             f"{mb[0]:9.1f}{mb[1]:9.1f}  {'met' if ok else 'MISSED'}   (max difference of (f) from (t), "
                             f"scaled by the largest gradient: {err:.1e})")
                print(lines[-1], flush=True)
                del out, G, routes
            del noise, kw, p0, p1
    return missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--arxiv-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mc_bwd_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    shipped_switch = ops.MC_BWD_FUSED
    lines = [f"Parameter gradients of a Monte-Carlo batch: stag_agg_bwd_w_mc against the per-sample loop; device "
             f"{torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of {args.inner} backward passes"]
    src, dst = synthetic.arxiv_like()
    n = int(max(src.max(), dst.max())) + 1
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    missed = shape_rows("arxiv", g, 128, dev, args.iters, args.inner, lines)
    del g
    if not args.arxiv_only:
        s, d, sizes = synthetic.ppi_like()
        gp = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                            batch_num_nodes=torch.from_numpy(sizes), device=dev)
        for D in (50, 256):
            missed += shape_rows("ppi batch", gp, D, dev, args.iters, args.inner, lines)
        del gp
        src, dst = synthetic.arxiv_like(n_nodes=CORA_NODES, n_edges=CORA_EDGES, max_in_degree=168, n_hubs=20, seed=4)
        gc = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), CORA_NODES, device=dev)
        missed += shape_rows("cora-sized", gc, CORA_FEATURES, dev, args.iters, args.inner, lines)
    lines.append(f"rule for ops.MC_BWD_FUSED = True (every case: max(f, f') <= mean(t, t') + |t - t'|): "
                 f"{'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    ops.MC_BWD_FUSED = shipped_switch
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
