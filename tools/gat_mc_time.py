#!/usr/bin/env python
"""Device time of the Monte-Carlo GAT forward: S samples from one gather of the ft rows per pass (ops.gat_aggregate_mc
-> stag_gat_fwd_mc) against S separate launches (ops.gat_aggregate at offset + s), for S in {1, 2, 4, 8}, at
  cfg5     the arxiv-shaped graph, H = 8, F = 32
  arxiv    the first layer of scripts/arxiv_mle/gat/run.py: H = 8, F = 8, with self loops
  ppi      the first layer of scripts/ppi_mle/gat/run.py: H = 4, F = 256, synthetic.ppi_like batch, XCD-local plan
and the reference's arxiv GAT evaluation block (model.eval(), no_grad, model.loss + model.forward at n_samples = 8;
the model of tools/arxiv_gat_epoch.py), batched against model._mc_batching_off = True, with peak memory.

    python tools/gat_mc_time.py [--only cfg5,arxiv,ppi,eval] [--samples 1,2,4,8] [--steps 20] [--json out.json]

The A/B of samples per pass runs a build variant through STAG_HIP_SO (tools/ab_bench.py build sp3=-DSTAG_GAT_MC_SP=3).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stag_amd  # noqa: E402
from stag_amd import _lib, ops, synthetic  # noqa: E402


def timeit(fn, steps, warmup):
    """Median device time (us) of fn() between events, one event pair per call."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warmup + i)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def shape(name, dev):
    if name == "cfg5":
        src, dst = synthetic.arxiv_like(seed=1)
        g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), synthetic.ARXIV_NODES, device=dev)
        return g, 8, 32
    if name == "arxiv":
        src, dst = synthetic.arxiv_like(seed=1)
        g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), synthetic.ARXIV_NODES, device=dev)
        return stag_amd.add_self_loop(stag_amd.remove_self_loop(g)), 8, 8
    import importlib
    importlib.import_module("stag_amd.graph").XCD_ORDER = "1"
    src, dst, sizes = synthetic.ppi_like()
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), int(sizes.sum()),
                       batch_num_nodes=torch.from_numpy(sizes).to(dev), device=dev)
    return g, 4, 256


def layer_rows(name, samples, steps, warmup, dev):
    g, H, F = shape(name, dev)
    n = g.number_of_nodes()
    el, er = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev)
    ft = torch.randn(n, H, F, device=dev)
    noise = lambda i: stag_amd.EdgeNoise(g, H, _lib.NOISE_NORMAL, 1.0, 0.5, seed=1, offset=100 * i)
    rows = []
    with torch.no_grad():
        g.csr.plan(64, need=True)
        for S in samples:
            tb = timeit(lambda i: ops.gat_aggregate_mc(g, el, er, ft, 0.2, noise(i), S, 1), steps, warmup)

            def loop(i):
                nz = noise(i)
                for s in range(S):
                    nz.offset = 100 * i + s
                    ops.gat_aggregate(g, el, er, ft, 0.2, nz)
            tl = timeit(loop, steps, warmup)
            rows.append(dict(shape=name, H=H, F=F, nodes=n, edges=g.number_of_edges(), S=S, batched_us=round(tb[0], 1),
                             batched_min_max=[round(tb[1], 1), round(tb[2], 1)], separate_us=round(tl[0], 1),
                             separate_min_max=[round(tl[1], 1), round(tl[2], 1)], ratio=round(tb[0] / tl[0], 3)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def eval_block(steps, warmup, dev):
    torch.distributions.Distribution.set_default_validate_args(False)
    src, dst = synthetic.arxiv_like(seed=1)
    n = synthetic.ARXIV_NODES
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    g = stag_amd.add_self_loop(stag_amd.remove_self_loop(g))
    x = torch.randn(n, 128, device=dev)
    y = torch.randint(0, 40, (n,), device=dev)
    N = torch.distributions.Normal
    SL, Z = stag_amd.layers.StagLayer, stag_amd.zoo
    layers = torch.nn.ModuleList([
        SL(Z.GAT(128, 8, num_heads=8, feat_drop=0.6, attn_drop=0.6, activation=torch.nn.functional.elu), q_a=N(1.0, 0.3)),
        SL(Z.GAT(64, 40, num_heads=8, last=True, feat_drop=0.6, attn_drop=0.6,
                 activation=lambda t: torch.nn.functional.softmax(t, dim=-1)), q_a=N(1.0, 0.3))])
    model = stag_amd.models.StagModel(layers=layers).to(dev)
    model.eval()

    def block(_):
        with torch.no_grad():
            model.loss(g, x, y, n_samples=8)
            model(g, x, n_samples=8)

    out = {}
    for name, off in (("batched", False), ("loop", True)):
        model._mc_batching_off = off
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t = timeit(block, steps, warmup)
        out[name] = dict(us=round(t[0], 1), min_max=[round(t[1], 1), round(t[2], 1)],
                         peak_mb=round(torch.cuda.max_memory_allocated() / 2**20, 1))
    out["ratio"] = round(out["batched"]["us"] / out["loop"]["us"], 3)
    row = dict(shape="arxiv_gat_eval_block", **out)
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="cfg5,arxiv,eval,ppi")
    ap.add_argument("--samples", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gat_mc_time.py times the GPU"
    dev = torch.device("cuda:0")
    samples = [int(s) for s in args.samples.split(",")]
    rows = []
    for name in args.only.split(","):
        if name == "eval":
            rows += eval_block(max(args.steps // 4, 3), 1, dev)
        else:
            rows += layer_rows(name, samples, args.steps, args.warmup, dev)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(lib=os.environ.get("STAG_HIP_SO", "libstag_hip.so"), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
