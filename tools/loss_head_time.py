#!/usr/bin/env python
"""The likelihood end of model.loss — Likelihood.mean_nll(out, y, mask): -log_prob, then the masked mean — as fused HIP
passes (ops.nll_mean: stag_nll_categorical_fwd / _bwd, stag_nll_bernoulli_fwd / _bwd) against the composed torch route
(the same build with ops.NLL_FUSED = False), in one process, at the shapes the reference's scripts run:
    Categorical  arxiv [169,343, 40] with a 0.54 mask and without one, Cora [2,708, 7] with 140 masked rows,
                 Pubmed [19,717, 3] with 60 masked rows, a readout batch [128, 10] without a mask
    Bernoulli    the PPI batch [56,944, 121] without a mask
For every case:
    fwd        the value alone, no grad                                                         us per call
    fwd+bwd    the value and its gradient with respect to the probabilities                     us per call
    peak       the peak allocation of one forward + backward over what is resident              MiB
Each of (c) the composed route, (c') the composed route again — the spread between two repeats of one route in the same
run — (f) the fused route and (f') the fused route again; the routes are interleaved so that clock and neighbours drift
over all of them alike; a sample is `--inner` calls between two device events; the table gives the median over `--iters`
samples.  ops.NLL_FUSED may be True only if max(f, f') <= mean(c, c') + |c - c'| for every timed case.  Value and gradient
of (f) are checked against (c)'s first.  Then two whole training steps with the switch off and on, alternating: the
arxiv GCN epoch of tools/arxiv_epoch.py and a Cora-sized two-layer GCN step.

    python tools/loss_head_time.py [--iters 20] [--inner 5] [--out FILE] [--cases arxiv,cora] [--no-steps]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stag_amd  # noqa: E402
from stag_amd import likelihoods, ops, synthetic  # noqa: E402

# (name, likelihood, N, C, masked rows: a fraction, a count, or None)
CASES = [("arxiv", "categorical", 169343, 40, 0.54), ("arxiv-all", "categorical", 169343, 40, None),
         ("cora", "categorical", 2708, 7, 140), ("pubmed", "categorical", 19717, 3, 60),
         ("readout", "categorical", 128, 10, None), ("ppi", "bernoulli", 56944, 121, None)]


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
    return float(((a - b).abs() / (1.0 + b.abs())).max())


def one_case(name, kind, n, C, masked, dev, iters, inner, lines):
    """Appends the row of one case; returns True when (f) meets the rule in every column."""
    gen = torch.Generator().manual_seed(3)
    if kind == "categorical":
        lk = likelihoods.CategoricalLikelihood()
        feat = torch.softmax(2.0 * torch.randn(n, C, generator=gen), -1).to(dev).requires_grad_(True)
        y = torch.randint(0, C, (n,), generator=gen).to(dev)
    else:
        lk = likelihoods.BernoulliLikelihood()
        feat = torch.sigmoid(2.0 * torch.randn(n, C, generator=gen)).to(dev).requires_grad_(True)
        y = (torch.rand(n, C, generator=gen) < 0.5).float().to(dev)
    if masked is None:
        mask = None
    elif isinstance(masked, float):
        mask = (torch.rand(n, generator=gen) < masked).to(dev)
    else:
        mask = torch.zeros(n, dtype=torch.bool)
        mask[torch.randperm(n, generator=gen)[:masked]] = True
        mask = mask.to(dev)

    def fwd(fused):
        def fn():
            ops.NLL_FUSED = fused
            with torch.no_grad():
                return lk.mean_nll(feat, y, mask)
        return fn

    def both(fused):
        def fn():
            ops.NLL_FUSED = fused
            feat.grad = None
            v = lk.mean_nll(feat, y, mask)
            v.backward()
            return v.detach(), feat.grad
        return fn

    ops.NLL_FUSED = True
    assert ops.nll_why_not(lk, feat, y, mask) is None
    ref, got = both(False)(), both(True)()
    count = n if mask is None else int(mask.sum())
    err = max(scaled(got[0], ref[0]), scaled(got[1] * count, ref[1] * count))
    assert err <= 1e-4, f"{name}: the fused route differs from the composed route by {err:.2e}"
    del ref, got
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
    feat.grad = None
    (tf, mf, _), (tb, mb, pb) = cols
    rows = "all" if masked is None else (f"{masked:.2f}" if isinstance(masked, float) else str(masked))
    lines.append(f"  {name:<10s}{kind[:4]:<5s}{n:>7d}{C:>4d}{rows:>6s} |{tf[0]:8.1f}{tf[1]:8.1f}{tf[2]:8.1f}{tf[3]:8.1f} "
                 f"{'met' if mf else 'MISSED':<7s}|{tb[0]:8.1f}{tb[1]:8.1f}{tb[2]:8.1f}{tb[3]:8.1f} {'met' if mb else 'MISSED':<7s}|"
                 f"{pb[0]:8.2f}{pb[1]:8.2f} | {err:.1e}")
    print(lines[-1], flush=True)
    return ok


def step_times(tag, step, lines, runs=4, epochs=30):
    """`runs` alternating runs of `epochs` steps per setting of the switch, 5 warm-up steps before each."""
    res = {False: [], True: []}
    for fused in [False, True, True, False] * (runs // 2):
        ops.NLL_FUSED = fused
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(epochs):
            loss = step()
        e1.record()
        torch.cuda.synchronize()
        wall, devt = (time.perf_counter() - t0) / epochs * 1e3, e0.elapsed_time(e1) / epochs
        res[fused].append((wall, devt))
        lines.append(f"{tag} switch {'on ' if fused else 'off'}: step {wall:.3f} ms wall, {devt:.3f} ms device, loss {loss.item():.4f}")
        print(lines[-1], flush=True)
    for fused in (False, True):
        w, d = np.median([r[0] for r in res[fused]]), np.median([r[1] for r in res[fused]])
        lines.append(f"{tag} switch {'on ' if fused else 'off'}: median {w:.3f} ms wall, {d:.3f} ms device over {runs} alternating "
                     f"runs of {epochs} steps")
        print(lines[-1], flush=True)


def arxiv_step(dev):
    import arxiv_epoch
    src, dst = synthetic.arxiv_like(seed=1)
    n = synthetic.ARXIV_NODES
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    g = stag_amd.add_reverse_edges(stag_amd.add_self_loop(stag_amd.remove_self_loop(g)))
    x = torch.randn(n, 128, device=dev)
    y = torch.randint(0, 40, (n,), device=dev)
    mask = torch.rand(n, device=dev) < 0.54
    model = arxiv_epoch.build(dev, "Bernoulli")
    return _step_of(model, g, x, y, mask)


def cora_step(dev):
    """A two-layer GCN on a Cora-sized graph (scripts/citation_*/gcn: 2,708 nodes, 1,433 features, 16 hidden, 7 classes,
    140 training rows)."""
    n, E = 2708, 10556
    gen = torch.Generator().manual_seed(5)
    g = stag_amd.Graph(torch.randint(0, n, (E,), generator=gen), torch.randint(0, n, (E,), generator=gen), n, device=dev)
    g = stag_amd.add_self_loop(g)
    x = torch.randn(n, 1433, generator=gen).to(dev)
    y = torch.randint(0, 7, (n,), generator=gen).to(dev)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=gen)[:140]] = True
    SL, Z = stag_amd.layers.StagLayer, stag_amd.zoo
    q_a = torch.distributions.Normal(1.0, 0.3, validate_args=False)
    layers = torch.nn.ModuleList([
        SL(Z.GCN(1433, 16, activation=torch.relu), q_a=q_a),
        SL(Z.GCN(16, 7, activation=lambda t: torch.nn.functional.softmax(t, dim=-1)), q_a=q_a)])
    model = stag_amd.models.StagModel(layers=layers).to(dev)
    return _step_of(model, g, x, y, mask.to(dev))


def _step_of(model, g, x, y, mask):
    opt = torch.optim.Adam(model.parameters(), 1e-2)

    def step():
        model.train()
        opt.zero_grad()
        loss = model.loss(g, x, y, mask=mask)
        loss.backward()
        opt.step()
        return loss
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--no-steps", action="store_true", help="the head cases only, not the two whole training steps")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_head_time.py measures on the GPU: no device found")
    torch.distributions.Distribution.set_default_validate_args(False)
    dev = torch.device("cuda:0")
    shipped = ops.NLL_FUSED
    lines = [f"likelihood head Likelihood.mean_nll: stag_nll_* (f, f again) against the composed torch route, ops.NLL_FUSED = False "
             f"(c, c again); device {torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of "
             f"{args.inner} calls",
             f"  {'case':<10s}{'lik':<5s}{'N':>7s}{'C':>4s}{'rows':>6s} |{'fwd c':>8s}{'c again':>8s}{'f':>8s}{'f again':>8s} {'us':<7s}|"
             f"{'f+b c':>8s}{'c again':>8s}{'f':>8s}{'f again':>8s} {'us':<7s}|{'peak c':>8s}{'f':>8s} | max scaled difference"]
    print("\n".join(lines), flush=True)
    ok = True
    wanted = args.cases.split(",")
    for name, kind, n, C, masked in CASES:
        if name in wanted:
            ok = one_case(name, kind, n, C, masked, dev, args.iters, args.inner, lines) and ok
            torch.cuda.empty_cache()
    lines.append(f"rule for ops.NLL_FUSED = True (every case: max(f, f') <= mean(c, c') + |c - c'|): {'met' if ok else 'NOT met'}")
    print(lines[-1], flush=True)
    if not args.no_steps:
        lines.append("")
        lines.append("whole training steps with ops.NLL_FUSED off / on, alternating in one process (5 warm-up steps, then 30 timed ones per run):")
        step_times("arxiv GCN Bernoulli epoch (tools/arxiv_epoch.py)", arxiv_step(dev), lines)
        torch.cuda.empty_cache()
        step_times("Cora-sized two-layer GCN step", cora_step(dev), lines)
    ops.NLL_FUSED = shipped
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
