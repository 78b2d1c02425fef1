#!/usr/bin/env python
"""The backward of an aggregation with amortised [E, D] edge noise when the input needs a gradient too: stag_agg_bwd_pedge
(dx and both [E, D] gradient tables from one pass over the source-major CSR) against the route it replaces, device time per
backward at the arxiv shape (D = 128), on the PPI batch (D = 50, 256), on a Cora-sized synthetic graph (2,708 nodes, 10,556
edges, D = 1433 and 16) and on a Pubmed-sized one (19,717 nodes, 88,648 edges, D = 500):
    for Normal with loc / log_scale (p1_log) and Uniform with low / high, with GCN's two degree scalings,
      (c)  stag_agg_bwd on csr_t + the [N, D] product g * dvec + stag_agg_bwd_w on csr (both gradient tables) — the baseline,
           whose device code this change leaves as it was
      (c') the same again: the spread between two repeats of one route in the same run
      (f)  stag_agg_bwd_pedge, (f') the same again
    and the training step (forward + backward) of StagLayer(GCN(in, in), AmortizedDistribution(in, in), vi=True) on an input
    that needs a gradient, with ops.PEDGE_BWD_FUSED off (c, c') and on (f, f').
One process; the routes of a case are interleaved so that clock and neighbours drift over all of them alike; a sample is
`--inner` calls between two device events; the table gives the median over `--iters` samples, and the peak allocation of one
call above what was allocated before it.  ops.PEDGE_BWD_FUSED may be True only if max(f, f') <= mean(c, c') + |c - c'| for
every case timed.  The outputs of (f) are checked against (c)'s first.

    python tools/pedge_bwd_time.py [--iters 12] [--inner 2] [--out FILE]
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

CORA_NODES, CORA_EDGES = 2708, 10556
PUBMED_NODES, PUBMED_EDGES = 19717, 88648
SEG = ops.DEFAULT_SEG_LEN


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


def rule_row(lines, missed, label, t, mb, extra=""):
    spread, base, f = abs(t[0] - t[1]), 0.5 * (t[0] + t[1]), max(t[2], t[3])
    ok = f <= base + spread
    if not ok:
        missed.append(label.strip())
    lines.append(f"  {label:<34s}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}{t[3]:10.1f}{f - base:9.1f}{spread:8.1f}{mb[0]:9.1f}{mb[1]:9.1f}"
                 f"  {'met' if ok else 'MISSED'}{extra}")
    print(lines[-1], flush=True)


def call_rows(name, g, D, dev, iters, inner, lines, missed):
    """The entry point against the three launches it replaces."""
    N, E = g.number_of_nodes(), g.number_of_edges()
    torch.manual_seed(0)
    x, G = torch.randn(N, D, device=dev), torch.randn(N, D, device=dev)
    ss = g.csr_t.degrees.clamp(min=1).to(torch.float32).pow(-0.5)
    dvec = g.csr.degrees.clamp(min=1).to(torch.float32).pow(-0.5)
    for kname, make in kinds(E, D, dev):
        kw = make()
        noise = stag_amd.EdgeNoise(g, D, kw["kind"], kw["p0"], kw["p1"], p1_log=kw["p1_log"], seed=5, offset=1)
        noise.param_mode, noise.p0, noise.p1 = _lib.PARAM_PER_EDGE, kw["p0"], kw["p1"]     # (whatever E and D are)
        spec = ops._noise_spec(noise, in_norm=0)
        spec_c = ops._targs_or_c(spec)

        def two_passes():
            dx, _, _ = ops._agg_bwd_raw(g.csr_t, G, D, spec, dvec, ss, SEG, False)
            gg = (G * dvec.unsqueeze(1)).contiguous()
            e0, e1 = ops._bwd_w_raw(g.csr, x, gg, D, ss, spec=spec_c, both=True, seg_len=SEG)
            return dx, e0, e1

        def one_pass():
            return ops._agg_bwd_pedge_raw(g.csr_t, G, x, D, spec_c, dvec, ss, SEG)
        routes = [two_passes, two_passes, one_pass, one_pass]
        outs = [fn() for fn in routes]                         # warm-up of every route: plans, code objects
        outs = [fn() for fn in routes]
        torch.cuda.synchronize()
        err = 0.0
        for i in range(3):                                     # against the two passes, relative to the largest value
            sc = max(1.0, float(outs[0][i].abs().max()))
            err = max(err, float((outs[2][i] - outs[0][i]).abs().max()) / sc)
            assert torch.equal(outs[2][i], outs[3][i]), f"{name} {kname}: two calls, different bits"
        assert err <= 2e-5, f"{name} D = {D} {kname}: stag_agg_bwd_pedge differs from the two passes by {err:.2e}"
        del outs
        mb = [peak_mb(routes[0]), peak_mb(routes[2])]
        t = timed(routes, iters, inner)
        rule_row(lines, missed, f"{name} D = {D} call {kname}", t, mb, f"   (max scaled difference of (f) from (c): {err:.1e})")
        del noise, kw, spec, spec_c


def step_row(name, g, D, dev, iters, inner, lines, missed):
    """The training step of one amortised GCN layer, the switch off and on."""
    from stag_amd import distributions, layers, zoo
    torch.manual_seed(1)
    layer = layers.StagLayer(zoo.GCN(D, D), q_a=distributions.AmortizedDistribution(D, D), vi=True).to(dev).train()
    feat = torch.randn(g.number_of_nodes(), D, device=dev, requires_grad=True)

    def route(fused):
        def fn():
            ops.PEDGE_BWD_FUSED = fused
            layer.zero_grad(set_to_none=True)
            feat.grad = None
            out = layer(g, feat)
            (out.square().mean() + layer.kl_divergence()).backward()
            return feat.grad
        return fn
    routes = [route(False), route(False), route(True), route(True)]
    for fn in routes * 2:
        fn()
    torch.cuda.synchronize()
    mb = [peak_mb(routes[0]), peak_mb(routes[2])]
    t = timed(routes, iters, inner)
    rule_row(lines, missed, f"{name} D = {D} layer step", t, mb)
    del layer, feat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--arxiv-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pedge_bwd_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    shipped_switch = ops.PEDGE_BWD_FUSED
    lines = [f"dx and both [E, D] parameter gradients from one pass: stag_agg_bwd_pedge against stag_agg_bwd + g * dvec + "
             f"stag_agg_bwd_w; device {torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of "
             f"{args.inner} calls; us per call, MB at the peak of one",
             f"  {'case':<34s}{'(c)':>10s}{'(c) again':>10s}{'(f)':>10s}{'(f) again':>10s}{'f - c':>9s}{'|c - c|':>8s}"
             f"{'MB (c)':>9s}{'MB (f)':>9s}  rule"]
    missed = []
    shapes = []
    src, dst = synthetic.arxiv_like()
    n = int(max(src.max(), dst.max())) + 1
    shapes.append(("arxiv", lambda: stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev), (128,)))
    if not args.arxiv_only:
        def ppi():
            s, d, sizes = synthetic.ppi_like()
            return stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                                  batch_num_nodes=torch.from_numpy(sizes), device=dev)

        def small(nodes, edges, seed):
            def make():
                s, d = synthetic.arxiv_like(n_nodes=nodes, n_edges=edges, max_in_degree=168, n_hubs=20, seed=seed)
                return stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), nodes, device=dev)
            return make
        shapes += [("ppi batch", ppi, (50, 256)), ("cora-sized", small(CORA_NODES, CORA_EDGES, 4), (1433, 16)),
                   ("pubmed-sized", small(PUBMED_NODES, PUBMED_EDGES, 6), (500,))]
    for name, make, widths in shapes:
        g = make()
        lines.append(f"{name}: N = {g.number_of_nodes()}, E = {g.number_of_edges()}")
        for D in widths:
            call_rows(name, g, D, dev, args.iters, args.inner, lines, missed)
            step_row(name, g, D, dev, args.iters, args.inner, lines, missed)
            torch.cuda.empty_cache()
        del g
    lines.append(f"rule for ops.PEDGE_BWD_FUSED = True (every case: max(f, f') <= mean(c, c') + |c - c'|): "
                 f"{'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    ops.PEDGE_BWD_FUSED = shipped_switch
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
