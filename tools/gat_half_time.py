#!/usr/bin/env python
"""Half-typed GAT feature rows: stag_gat_fwd_half against the routes it stands beside, device time per
ops.gat_aggregate call (no grad), for no noise, Normal, and Normal + attention dropout 0.6:
    (a)  fp32 ft                        stag_gat_fwd
    (b)  bf16 ft, the cast route        ft.float() + stag_gat_fwd         (ops.GAT_HALF_ROWS = False)
    (b') the same again: the spread between two repeats of one route in the same run
    (c)  bf16 ft as it is               stag_gat_fwd_half                 (ops.GAT_HALF_ROWS = True)
    (c') fp16 ft as it is               stag_gat_fwd_half
Shapes: cfg5 (the arxiv-shaped CSR, 8 heads x 32), the PPI batch (4 x 64, XCD-local batches), and one shard of eight
of cfg5 (the first eighth of the destination rows, every source row: the entry points called directly).
Then zoo.GAT(128 -> 8 x 32) on the cfg5 graph under bf16 autocast, forward and training step, ops.GAT_HALF_FT off / on.
One process; the routes are interleaved (a, b, b', c, c', a, ...) so that clock and neighbours drift over all of them
alike; a sample is `--inner` calls between two device events; the table gives the median over `--iters` samples.
(c) is asserted torch.equal to (b) before anything is timed.  The last column applies the rule for the default of
ops.GAT_HALF_ROWS: (c) not slower than (b) by more than |b - b'|, for every kind at cfg5.

    python tools/gat_half_time.py [--iters 30] [--inner 10] [--out FILE] [--cfg5-only] [--no-layer]
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
from stag_amd.graph import CsrView  # noqa: E402

KINDS = (("none", None, None), ("normal", (_lib.NOISE_NORMAL, 1.0, 0.5), None),
         ("normal+drop", (_lib.NOISE_NORMAL, 1.0, 0.5), (0.6, 0xD00D, 4)))


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


def table(name, head, make_routes, iters, inner, lines):
    """One shape: make_routes(kind) -> the five routes.  Returns True when (c) meets the rule for every kind."""
    lines.append(f"{name}: {head}; us per call")
    lines.append(f"  {'kind':<12s}{'(a) fp32':>10s}{'(b) cast':>10s}{'(b) again':>10s}{'(c) bf16':>10s}{'(c) fp16':>10s}"
                 f"{'c/a':>7s}{'c - b':>8s}{'|b - b|':>8s}  rule")
    all_ok = True
    for kname, par, drop in KINDS:
        routes = make_routes(par, drop)
        with torch.no_grad():
            outs = [fn() for fn in routes]                     # warm-up of every route: plans, code objects
            outs = [fn() for fn in routes]
            torch.cuda.synchronize()
            assert torch.equal(outs[3], outs[1]), f"{name} {kname}: stag_gat_fwd_half differs from the cast route"
            del outs
            ta, tb, tb2, tc, tch = timed(routes, iters, inner)
        spread = abs(tb - tb2)
        ok = tc <= 0.5 * (tb + tb2) + spread               # (b) = the mean of its two repeats
        all_ok = all_ok and ok
        lines.append(f"  {kname:<12s}{ta:10.1f}{tb:10.1f}{tb2:10.1f}{tc:10.1f}{tch:10.1f}{tc / ta:7.2f}"
                     f"{tc - 0.5 * (tb + tb2):8.1f}{spread:8.1f}  {'met' if ok else 'MISSED'}   ((c) torch.equal (b))")
        print(lines[-1], flush=True)
    ops.GAT_HALF_ROWS = False
    return all_ok


def graph_routes(g, H, F, dev):
    N = g.number_of_nodes()
    torch.manual_seed(0)
    el, er = torch.randn(N, H, device=dev), torch.randn(N, H, device=dev)
    f32 = torch.randn(N, H, F, device=dev)
    fb, fh = f32.to(torch.bfloat16), f32.to(torch.float16)

    def make(par, drop):
        noise = None if par is None else stag_amd.EdgeNoise(g, H, par[0], par[1], par[2], seed=5, offset=1)

        def route(ft, half):
            def fn():
                ops.GAT_HALF_ROWS = half
                return ops.gat_aggregate(g, el, er, ft, 0.2, noise, attn_drop=drop)
            return fn
        return [route(f32, False), route(fb, False), route(fb, False), route(fb, True), route(fh, True)]
    return make


def shard_routes(g, H, F, dev, parts=8):
    """The first of `parts` equal ranges of destination rows with every source row: a shard-sized launch (its time is
    the longest unit's chain of round trips, not the fabric's)."""
    full = g.csr
    N = full.n_dst
    nd = N // parts
    cut = int(full.indptr[nd])
    csrv = CsrView(nd, N, full.indptr[:nd + 1].contiguous(), full.indices[:cut].contiguous())
    plan_t = csrv.plan(ops.DEFAULT_SEG_LEN, need=True)
    torch.manual_seed(0)
    el, er = torch.randn(N, H, device=dev), torch.randn(nd, H, device=dev)
    f32 = torch.randn(N, H, F, device=dev)
    fb, fh = f32.to(torch.bfloat16), f32.to(torch.float16)

    def make(par, drop):
        if par is None:
            spec = ops._targs_or_c(ops._none_spec())
        else:
            spec = _lib.NoiseSpec()
            spec.kind, spec.p0_scalar, spec.p1_scalar, spec.seed, spec.offset = par[0], par[1], par[2], 5, 1
        d = ops._gat_drop_struct(drop)

        def route(ft, half, cast):
            out = torch.empty(nd, H, F, device=dev)        # (a buffer per route: the comparison before timing is real)

            def fn():
                if half:
                    ops._gat_fwd_half_raw(csrv, plan_t, el, er, ft, H, F, 0.2, spec, None, d, out, None, ops.DEFAULT_SEG_LEN, dev)
                else:
                    ops._gat_fwd_into(csrv, plan_t, el, er, ft.float() if cast else ft, H, F, 0.2, spec, None, d, out, None, dev)
                return out
            return fn
        return [route(f32, False, False), route(fb, False, True), route(fb, False, True), route(fb, True, False),
                route(fh, True, False)]
    return make, (nd, cut)


def layer_rows(g, dev, iters, inner, lines):
    """zoo.GAT(128 -> 8 x 32) with Normal edge noise and attention dropout 0.6 under bf16 autocast: forward (no grad)
    and a training step, ops.GAT_HALF_FT off (ft in fp32, as always) and on (ft from a bf16 GEMM, gathered as it is)."""
    N = g.number_of_nodes()
    torch.manual_seed(0)
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GAT(128, 32, num_heads=8, attn_drop=0.6),
                                      q_a=torch.distributions.Normal(1.0, 0.5)).to(dev)
    layer.train()
    x = torch.randn(N, 128, device=dev)

    def fwd(on):
        def fn():
            ops.GAT_HALF_FT = ops.GAT_HALF_ROWS = on
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return layer(g, x)
        return fn

    def step(on):
        def fn():
            ops.GAT_HALF_FT = ops.GAT_HALF_ROWS = on
            for p in layer.parameters():
                p.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = layer(g, x)
            out.square().mean().backward()
        return fn
    lines.append(f"zoo.GAT(128 -> 8 x 32) under bf16 autocast, N = {N}, Normal noise, attn_drop 0.6; us per call "
                 f"(off, off again, on)")
    for name, mk in (("forward", fwd), ("training step", step)):
        routes = [mk(False), mk(False), mk(True)]
        for fn in routes + routes:
            fn()
        torch.cuda.synchronize()
        t0, t1, t2 = timed(routes, iters, max(inner // 2, 1))
        lines.append(f"  {name:<14s}{t0:10.1f}{t1:10.1f}{t2:10.1f}   on / off {t2 / (0.5 * (t0 + t1)):.2f}")
        print(lines[-1], flush=True)
    ops.GAT_HALF_FT = ops.GAT_HALF_ROWS = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cfg5-only", action="store_true", help="the cfg5 table only (a profiler capture, an A/B build)")
    ap.add_argument("--no-layer", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_half_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = [f"half-typed GAT rows: stag_gat_fwd_half against fp32 ft and the cast route; device "
             f"{torch.cuda.get_device_name(0)}; interleaved, median of {args.iters} samples of {args.inner} calls"]
    src, dst = synthetic.arxiv_like()
    n = int(max(src.max(), dst.max())) + 1
    g = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
    ok = table("cfg5", f"N = {n}, E = {g.number_of_edges()}, 8 x 32", graph_routes(g, 8, 32, dev), args.iters, args.inner, lines)
    lines.append(f"rule for ops.GAT_HALF_ROWS = True at cfg5 (every kind: (c) <= (b) + |b - b'|): {'met' if ok else 'NOT met'}")
    if not args.cfg5_only:
        s, d, sizes = synthetic.ppi_like()
        gp = stag_amd.Graph(torch.from_numpy(s), torch.from_numpy(d), int(sizes.sum()),
                            batch_num_nodes=torch.from_numpy(sizes), device=dev)
        table("ppi batch", f"N = {gp.number_of_nodes()}, E = {gp.number_of_edges()}, 4 x 64", graph_routes(gp, 4, 64, dev),
              args.iters, args.inner, lines)
        make, (nd, cut) = shard_routes(g, 8, 32, dev)
        table("cfg5, one shard of eight", f"{nd} destination rows, {cut} edges, 8 x 32 (entry points called directly)",
              make, args.iters, args.inner, lines)
        if not args.no_layer:
            layer_rows(g, dev, args.iters, args.inner, lines)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
