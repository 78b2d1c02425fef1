#!/usr/bin/env python
"""Monte-Carlo samples of amortised [E, D] edge noise: stag_agg_fwd_mc_pedge (one pass over the rows and both parameter
tables for S samples) against the loop it replaces, device time per S samples (no grad) at the arxiv shape (D = 128), on
the PPI batch (D = 50, 256) and on a Cora-sized synthetic graph (2,708 nodes, 10,556 edges, D = 1433):
    for Normal with [E, D] loc / log_scale (p1_log) and Uniform with [E, D] low / high, S in {2, 4, 8, 16}:
      (t)  the loop: S launches of stag_agg_fwd with the same PER_EDGE spec at offset + s * stride — the baseline
      (t') the same again: the spread between two repeats of one route in the same run
      (f)  stag_agg_fwd_mc_pedge, (f') the same again
    an inference StagModel.forward(n_samples = 16) of a citation_rec/gcn-shaped model on the Cora-sized graph (Dropout,
    StagLayer(GCN, AmortizedDistribution(in, in)), Dropout, StagLayer(GCN, AmortizedDistribution(hidden, hidden)), eval()),
    batching on and off (model._mc_batching_off), each twice
One process; the routes of a case are interleaved so that clock and neighbours drift over all of them alike; a sample is
`--inner` calls between two device events; the table gives the median over `--iters` samples.  ops.MC_PEDGE_FUSED may be
True only if max(f, f') <= mean(t, t') + |t - t'| for every case timed.  Outputs of (f) are checked against (t)'s first.

    python tools/mc_pedge_time.py [--iters 20] [--inner 3] [--out FILE]
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

SAMPLES = (2, 4, 8, 16)
STRIDE = 2          # offsets per sample of a two-layer model
CORA_NODES, CORA_EDGES, CORA_FEATURES, CORA_CLASSES = 2708, 10556, 1433, 7


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


def kinds(E, D, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    r = lambda: torch.rand(E, D, generator=gen, device=dev)
    return (("normal log", lambda: dict(kind=_lib.NOISE_NORMAL, p0=0.5 + r(), p1=-1.5 + r(), p1_log=True)),
            ("uniform", lambda: dict(kind=_lib.NOISE_UNIFORM, p0=0.2 * r(), p1=1.5 + r(), p1_log=False)))


def shape_rows(name, g, D, dev, iters, inner, lines):
    """Appends the table of one shape; returns True when (f) meets the rule for every case."""
    N, E = g.number_of_nodes(), g.number_of_edges()
    torch.manual_seed(0)
    x = torch.randn(N, D, device=dev)

    def route(noise, S, fused):
        def fn():
            ops.MC_PEDGE_FUSED = fused
            return ops.aggregate_mc(g, x, noise, S, STRIDE)
        return fn

    lines.append(f"{name}: N = {N}, E = {E}, D = {D}; us per S samples")
    lines.append(f"  {'kind':<12s}{'S':>3s}{'(t) loop':>10s}{'(t) again':>10s}{'(f) fused':>10s}{'(f) again':>10s}"
                 f"{'f - t':>9s}{'|t - t|':>8s}  rule")
    all_ok = True
    with torch.no_grad():
        for kname, make in kinds(E, D, dev):
            kw = make()                                        # (one kind's two [E, D] tables at a time)
            noise = stag_amd.EdgeNoise(g, D, kw["kind"], kw["p0"], kw["p1"], p1_log=kw["p1_log"], seed=5, offset=1)
            assert noise.param_mode == _lib.PARAM_PER_EDGE
            for S in SAMPLES:
                routes = [route(noise, S, False), route(noise, S, False), route(noise, S, True), route(noise, S, True)]
                outs = [fn() for fn in routes]                 # warm-up of every route: plans, code objects
                outs = [fn() for fn in routes]
                torch.cuda.synchronize()
                # two fp32 sums of up to 13,000 terms in different block orders.  Each rounds its running block sums, so
                # they differ by about 2^-24 sqrt(deg) |term| whatever the sum comes to, and among S * D sums of a hub
                # row some cancel to almost nothing: the difference is held against the row's largest sum (what was
                # summed), not against the sum that happens to cancel.  (tests/test_gpu_mc_pedge.py holds the values to
                # the oracle at the project's bar.)
                scale = 1 + outs[0].abs().amax(dim=2, keepdim=True)
                err = float(((outs[2] - outs[0]).abs() / scale).max())
                assert err <= 2e-5, f"{name} {kname} S={S}: stag_agg_fwd_mc_pedge differs from the loop by {err:.2e}"
                assert torch.equal(outs[2], outs[3]), f"{name} {kname} S={S}: two launches, different bits"
                del outs
                t = timed(routes, iters, inner)
                spread = abs(t[0] - t[1])
                base = 0.5 * (t[0] + t[1])
                f = max(t[2], t[3])
                ok = f <= base + spread
                all_ok = all_ok and ok
                lines.append(f"  {kname:<12s}{S:3d}{t[0]:10.1f}{t[1]:10.1f}{t[2]:10.1f}{t[3]:10.1f}{f - base:9.1f}{spread:8.1f}"
                             f"  {'met' if ok else 'MISSED'}   (max difference of (f) from (t), scaled by the row's largest sum: {err:.1e})")
                print(lines[-1], flush=True)
            del noise, kw
    return all_ok


def model_rows(g, dev, iters, lines):
    """Inference StagModel.forward(n_samples = 16) of a citation_rec/gcn-shaped model on the Cora-sized graph; ms per call.
    True when batching meets the rule."""
    from stag_amd import distributions, layers, models
    torch.manual_seed(0)
    D, H, C_ = CORA_FEATURES, 16, CORA_CLASSES
    p_a = torch.distributions.Normal(1.0, 0.5, validate_args=False)
    x = torch.randn(g.number_of_nodes(), D, device=dev)
    model = models.StagModel(torch.nn.ModuleList([
        layers.FeatOnlyLayer(torch.nn.Dropout(0.5)),
        layers.StagLayer(stag_amd.zoo.GCN(D, H, activation=torch.nn.ReLU()),
                         q_a=distributions.AmortizedDistribution(D, D, init_like=p_a), p_a=p_a),
        layers.FeatOnlyLayer(torch.nn.Dropout(0.5)),
        layers.StagLayer(stag_amd.zoo.GCN(H, C_), q_a=distributions.AmortizedDistribution(H, H, init_like=p_a), p_a=p_a),
    ])).to(dev).eval()

    def call(off):
        def fn():
            model._mc_batching_off = off
            return model.forward(g, x, n_samples=16, return_parameters=True)
        return fn
    routes = [call(True), call(True), call(False), call(False)]
    with torch.no_grad():
        outs = []
        for fn in routes * 2:
            stag_amd.manual_seed(7)
            outs.append(fn())
        torch.cuda.synchronize()
        assert not model._mc_batching_off, "the model fell back to the loop"
        err = float(((outs[2] - outs[0]).abs() / (1 + outs[0].abs())).max())
        assert err <= 1e-4, f"model: batched forward differs from the loop by {err:.2e}"
        del outs
        t = [v / 1e3 for v in timed(routes, iters, 2)]
    spread = abs(t[0] - t[1])
    base = 0.5 * (t[0] + t[1])
    ok = max(t[2], t[3]) <= base + spread
    lines.append(f"StagModel.forward(n_samples = 16), citation_rec/gcn-shaped model ({D} -> {H} -> {C_}, leading Dropout), "
                 f"eval(), Cora-sized graph: ms per call")
    lines.append(f"  loop (_mc_batching_off): {t[0]:.3f}, again {t[1]:.3f}; first stochastic layer batched "
                 f"(stag_agg_fwd_mc_pedge): {t[2]:.3f}, again {t[3]:.3f}"
                 f"  rule {'met' if ok else 'MISSED'}   (max scaled difference of the outputs: {err:.1e})")
    print(lines[-1], flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--arxiv-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mc_pedge_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    shipped_switch = ops.MC_PEDGE_FUSED
    lines = [f"Monte-Carlo samples of [E, D] edge noise: stag_agg_fwd_mc_pedge against the loop of stag_agg_fwd; device "
             f"{torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of {args.inner} calls"]
    src, dst = synthetic.arxiv_like()
    n = int(max(src.max(), dst.max())) + 1
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    ok = shape_rows("arxiv", g, 128, dev, args.iters, args.inner, lines)
    del g
    src, dst = synthetic.arxiv_like(n_nodes=CORA_NODES, n_edges=CORA_EDGES, max_in_degree=168, n_hubs=20, seed=4)
    gc = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), CORA_NODES, device=dev)
    if not args.arxiv_only:
        s, d, sizes = synthetic.ppi_like()
        gp = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                            batch_num_nodes=torch.from_numpy(sizes), device=dev)
        for D in (50, 256):
            ok = shape_rows("ppi batch", gp, D, dev, args.iters, args.inner, lines) and ok
        del gp
        ok = shape_rows("cora-sized", gc, CORA_FEATURES, dev, args.iters, args.inner, lines) and ok
    ops.MC_PEDGE_FUSED = True      # (the model rows compare batching on and off through the model's own switch)
    ok = model_rows(gc, dev, args.iters, lines) and ok
    lines.append(f"rule for ops.MC_PEDGE_FUSED = True (every case: max(f, f') <= mean(t, t') + |t - t'|): "
                 f"{'met' if ok else 'NOT met'}")
    ops.MC_PEDGE_FUSED = shipped_switch
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
