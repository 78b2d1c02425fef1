#!/usr/bin/env python
"""The contrastive NLL of amortised edge noise (stag/models.py:7-25): stag_contrastive_nll against the composed route
(an [E, 2 in] concatenation of the fake endpoints' features, the MLP over its E rows, two Normal objects).

The model of scripts/citation_rec_contrastive/gcn/run.py without its dropout layers:
    StagModelContrastive([StagLayer(GCN(in, 16, relu),     q_a=AmortizedDistribution(in, 1), p_a=Normal(0.5, 1), vi=True),
                          StagLayer(GCN(16, classes, softmax), q_a=AmortizedDistribution(16, 1), p_a=Normal(0.5, 1), vi=True)])
on synthetic graphs of three shapes: Cora-sized (N 2708, E 13264, in 1433), Pubmed-sized (N 19717, E 108365, in 500) and
the arxiv-shaped CSR of bench.py at in = 128.  A step is loss_terms + backward of (nll + reg).  Per shape:
    (a)  ops.CONTRASTIVE_FUSED = False     the composed route: what the parent of this change ran
    (a') the same again: the spread between two repeats of one route in the same run
    (b)  ops.CONTRASTIVE_FUSED = True      stag_contrastive_nll
One process; the routes are interleaved (a, a', b, a, ...) after warm-up, so that clock and neighbours drift over all of
them alike; a sample is `--inner` steps between two device events; the table gives the median over `--iters` samples and
the peak of torch.cuda.max_memory_allocated over one step of each route (above what is allocated before the step).  The
model differentiates the LAST layer's term only (in = 16), and computes the first layer's (in = the features') forward
and discards it, as the reference does; so a second table times the term alone at the first layer's width — condition()
+ nll_contrastive + backward with the features as data, both routes — next to the stag_contrastive_nll call alone (value
and all five gradients), the two CSR views of the fake graph alone, and d P from d pre (those builds, their plans and the
two aggregations: what the backward adds when P needs a gradient).  Before timing, the two routes' values and parameter
gradients are compared.  The last line applies the rule for the default of the switch: True unless, at some shape, (b)
measures slower than (a) by more than |a - a'|.

    python tools/contrastive_time.py [--iters 20] [--inner 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stag_amd  # noqa: E402
from stag_amd import models, ops, synthetic  # noqa: E402

HIDDEN = 16


def timed(routes, iters, inner):
    """Median device time (us per call) of every route, interleaved."""
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
    gen = torch.Generator().manual_seed(seed)
    return stag_amd.Graph(torch.randint(0, n, (e,), generator=gen), torch.randint(0, n, (e,), generator=gen), n, device=dev)


def arxiv_graph(dev):
    src, dst = synthetic.arxiv_like(seed=1)
    n = int(max(src.max(), dst.max())) + 1
    return stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)


SHAPES = [("cora", lambda dev: uniform_graph(2708, 13264, 1, dev), 1433, 7),
          ("pubmed", lambda dev: uniform_graph(19717, 108365, 2, dev), 500, 3),
          ("arxiv", arxiv_graph, 128, 40)]


def make_model(in_features, classes, dev):
    L, Z, Dist = stag_amd.layers, stag_amd.zoo, stag_amd.distributions
    torch.manual_seed(0)
    layers = torch.nn.ModuleList([
        L.StagLayer(Z.GCN(in_features, HIDDEN, activation=torch.nn.functional.relu, allow_zero_in_degree=True),
                    q_a=Dist.AmortizedDistribution(in_features, 1), p_a=torch.distributions.Normal(0.5, 1.0), vi=True),
        L.StagLayer(Z.GCN(HIDDEN, classes, activation=lambda x: torch.nn.functional.softmax(x, dim=-1),
                          allow_zero_in_degree=True),
                    q_a=Dist.AmortizedDistribution(HIDDEN, 1), p_a=torch.distributions.Normal(0.5, 1.0), vi=True)])
    return models.StagModelContrastive(layers=layers, kl_scaling=1.0).to(dev)


def make_step(model, g, x, y, mask, fused):
    def fn():
        ops.CONTRASTIVE_FUSED = fused
        model.zero_grad(set_to_none=True)
        torch.manual_seed(7)               # the same fake edges and the same draw on every route
        stag_amd.manual_seed(7)
        nll, reg = model.loss_terms(g, x, y, mask=mask)
        (nll + reg).backward()
        return (nll + reg).detach()
    return fn


def make_term(q, g, x, fused):
    def fn():
        ops.CONTRASTIVE_FUSED = fused
        q.zero_grad(set_to_none=True)
        torch.manual_seed(7)
        q.condition(g, x)
        val = models.nll_contrastive(q, g, x)
        val.backward()
        return val.detach()
    return fn


def grads_of(module):
    return [p.grad.clone() for p in module.parameters() if p.grad is not None]


def max_err(a, b):
    sc = lambda r: max(1.0, float(r.abs().max()))
    return max(float(((x - r).abs() / sc(r) / (1.0 + r.abs() / sc(r))).max()) for x, r in zip(a, b))


def one_shape(name, g, K, classes, dev, iters, inner):
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, K, generator=gen).to(dev)
    y = torch.randint(0, classes, (n,), generator=gen).to(dev)
    mask = (torch.rand(n, generator=gen) < 0.3).to(dev)
    model = make_model(K, classes, dev)
    off, off2, on = (make_step(model, g, x, y, mask, f) for f in (False, False, True))
    v_off = off()
    g_off = grads_of(model)
    v_on = on()
    g_on = grads_of(model)
    err = max_err([v_on] + g_on, [v_off] + g_off)
    for fn in (off, off2, on, off, off2, on):
        fn()
    torch.cuda.synchronize()
    mem_off, mem_on = peak_of(off), peak_of(on)
    t_off, t_off2, t_on = timed([off, off2, on], iters, inner)
    mean_off, spread = 0.5 * (t_off + t_off2), abs(t_off - t_off2)
    step = (f"  {name:<8s}{n:>8d}{E:>9d}{K:>6d}{t_off:10.1f}{t_off2:10.1f}{t_on:10.1f}{t_on / mean_off:8.2f}{spread:9.1f}"
            f"{mem_off:11.1f}{mem_on:11.1f}   {err:.1e}")

    # the term alone at the first layer's width, the features as data
    q = model.layers[0].q_a
    toff, toff2, ton = (make_term(q, g, x, f) for f in (False, False, True))
    w_off = toff()
    gq_off = grads_of(q)
    w_on = ton()
    gq_on = grads_of(q)
    terr = max_err([w_on] + gq_on, [w_off] + gq_off)
    for fn in (toff, toff2, ton):
        fn()
    tm_off, tm_on = peak_of(toff), peak_of(ton)
    tt_off, tt_off2, tt_on = timed([toff, toff2, ton], iters, inner)
    # the launch alone, the fake graph's two CSR views alone, d P from d pre
    ops.CONTRASTIVE_FUSED = True
    with torch.no_grad():
        q.condition(g, x)
        P, wh, bh = q._narrow_tables(x)
        P, wh, bh = P.contiguous(), wh.contiguous(), bh.contiguous()
        loc, ls = (q.new_parameters[k].reshape(E).contiguous() for k in ("loc", "log_scale"))
        fs = torch.randint(high=n, size=[E], device=dev).to(torch.int32)
        fd = torch.randint(high=n, size=[E], device=dev).to(torch.int32)
        hidden = wh.shape[0]
        call = lambda: ops._contrastive_raw(loc, ls, fs, fd, P, hidden, wh, bh, (True,) * 5)
        dpre = call()[3]

        def views():
            fake = stag_amd.Graph(fs, fd, n, _trusted=True)
            return fake.csr, fake.csr_t
        dP = lambda: torch.cat(ops._pre_grad_tables(stag_amd.Graph(fs, fd, n, _trusted=True), dpre), 1)
        for fn in (call, views, dP):
            fn()
        t_call, t_views, t_dp = timed([call, views, dP], iters, inner)
    term = (f"  {name:<8s}{tt_off:10.1f}{tt_off2:10.1f}{tt_on:10.1f}{tt_on / (0.5 * (tt_off + tt_off2)):8.2f}"
            f"{abs(tt_off - tt_off2):9.1f}{tm_off:11.1f}{tm_on:11.1f}{t_call:9.1f}{t_views:10.1f}{t_dp:9.1f}   {terr:.1e}")
    return step, term, t_on <= mean_off + spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrastive_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    default = ops.CONTRASTIVE_FUSED
    head = [f"contrastive NLL of amortised edge noise: stag_contrastive_nll against the composed route; device "
            f"{torch.cuda.get_device_name(0)}; interleaved after warm-up, median of {args.iters} samples of {args.inner} "
            f"calls; times in us, memory in MiB above what is allocated before the call",
            f"training step of StagModelContrastive (two StagLayer(GCN), hidden {HIDDEN}): loss_terms + backward",
            f"  {'shape':<8s}{'N':>8s}{'E':>9s}{'in':>6s}{'(a) off':>10s}{'(a) again':>10s}{'(b) on':>10s}{'b / a':>8s}{'|a - a|':>9s}"
            f"{'peak a':>11s}{'peak b':>11s}   max scaled |b - a| of the loss and parameter gradients"]
    print("\n".join(head), flush=True)
    steps, terms, ok = [], [], []
    for name, make, K, classes in SHAPES:
        g = make(dev)
        step, term, met = one_shape(name, g, K, classes, dev, args.iters, args.inner)
        print(step, flush=True)
        steps.append(step), terms.append(term), ok.append(met)
        del g
        torch.cuda.empty_cache()
    mid = ["the term alone at the first layer's width (condition() + nll_contrastive + backward, features as data); `call`: "
           "stag_contrastive_nll alone, value and five gradients; `2 csr`: both CSR views of the fake graph; `d P`: those, "
           "their plans and the two aggregations of d pre",
           f"  {'shape':<8s}{'(a) off':>10s}{'(a) again':>10s}{'(b) on':>10s}{'b / a':>8s}{'|a - a|':>9s}{'peak a':>11s}"
           f"{'peak b':>11s}{'call':>9s}{'2 csr':>10s}{'d P':>9s}   max scaled |b - a| of the term and q_a's gradients"]
    lines = head + steps + mid + terms
    lines.append("rule for ops.CONTRASTIVE_FUSED = True (at every shape the fused step not slower than the composed one by more "
                 "than |a - a|): " + ("met" if all(ok) else "NOT met at " + ", ".join(s[0] for s, m in zip(SHAPES, ok) if not m)))
    print("\n".join(mid + terms + lines[-1:]), flush=True)
    ops.CONTRASTIVE_FUSED = default
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
