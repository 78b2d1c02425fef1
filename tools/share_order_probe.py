#!/usr/bin/env python
"""The share order (stag_plan_share_device) on the arxiv-shaped graph, in ONE process:

  python tools/share_order_probe.py [--rounds 7] [--steps 200] [--out FILE]

  - how long the device builder takes (events around whole builds, after a first one that loads the kernels);
  - how many repeated sources per aligned block of 2 / 4 / 8 units it finds, beside plan order and the sequential greedy
    (stag_plan_share on the host);
  - the launch time in plan order and in share order, interleaved rounds on two Graph objects of the same edges, for the
    shapes the order must not lose on; every pair of outputs is compared bit for bit;
  - the launch count after which building the order has paid for itself: build time / saving of the headline launch."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seg-len", type=int, default=64)
    ap.add_argument("--shapes", default="normal:128,uniform:128,bernoulli:128,none:128,normal:256,normal:64",
                    help="noise:D pairs to time; the first is the headline the threshold is formed from")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stag_amd
    import bench
    from stag_amd import _lib, ops, synthetic
    from stag_amd.graph import repeated_sources
    gm = importlib.import_module("stag_amd.graph")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    src, dst = synthetic.arxiv_like(seed=1)
    n = synthetic.ARXIV_NODES
    graphs = {}
    for order in ("plan", "share"):
        gm.SHARE_ORDER, gm.XCD_ORDER = ("1" if order == "share" else "0"), "0"
        g = graphs[order] = stag_amd.Graph(torch.from_numpy(src), torch.from_numpy(dst), n, device=dev)
        for view in (g.csr, g.csr_t):
            view.plan(args.seg_len)
    gm.SHARE_ORDER = "0"        # (what is built stays; the plan-order graph never gets one)
    g = graphs["share"]
    plan = g.csr.plan(args.seg_len)
    assert g.csr.share_units(plan) is not None and graphs["plan"].csr.share_units(graphs["plan"].csr.plan(args.seg_len)) is None

    # build time
    torch.cuda.synchronize()
    times, wall = [], []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        again = g.csr._build_share_units(plan)
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        times.append(e0.elapsed_time(e1))
    assert torch.equal(again, plan["share"])
    build_ms = float(np.median(times))
    say(f"device builder, {plan['n_units']} units ({plan['n_seg']} segments), {g.csr.n_edges} edges: median {build_ms:.3f} ms on "
        f"the stream (min {min(times):.3f}, max {max(times):.3f}), {np.median(wall):.3f} ms wall with the allocation, 10 builds")

    # what it found
    nu, n_seg = plan["n_units"], plan["n_seg"]
    units_h, idx_h = plan["units"][:nu].cpu().numpy(), g.csr.indices.cpu().numpy()
    greedy = np.zeros_like(units_h)
    t0 = time.perf_counter()
    _lib.check(_lib.lib().stag_plan_share(units_h.ctypes.data, nu, n_seg, plan["n_heavy"], args.seg_len, idx_h.ctypes.data,
                                          len(idx_h), greedy.ctypes.data), "stag_plan_share")
    say(f"sequential greedy on the host: {(time.perf_counter() - t0) * 1e3:.0f} ms")
    share_h = plan["share"][:nu].cpu().numpy()
    found = {}
    for block in (2, 4, 8):
        found[block] = [repeated_sources(a, n_seg, idx_h, block) for a in (units_h, share_h, greedy)]
        say(f"repeated sources inside an aligned block of {block} units: plan order {found[block][0]}, device builder "
            f"{found[block][1]}, sequential greedy {found[block][2]}")
    say(f"device builder / sequential greedy at 8: {found[8][1] / max(found[8][2], 1):.3f}; "
        f"{found[8][1]} x 512 B = {found[8][1] * 512 / 1e6:.1f} MB of row fetches a workgroup could share at D = 128")

    # launch times
    shapes = [(p.split(":")[0], int(p.split(":")[1])) for p in args.shapes.split(",")]
    saving = None
    for noise, D in shapes:
        x = torch.randn(n, D, device=dev)
        one = lambda gr, i: ops.aggregate(gr, x, bench.make_noise(stag_amd, gr, D, noise, i), seg_len=args.seg_len)
        assert torch.equal(one(graphs["plan"], 3), one(graphs["share"], 3)), (noise, D)
        t = {k: [] for k in graphs}
        for r in range(args.rounds + 1):
            for name, gr in graphs.items():
                for i in range(10):
                    one(gr, i)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.steps):
                    one(gr, i)
                e1.record()
                torch.cuda.synchronize()
                if r > 0:
                    t[name].append(e0.elapsed_time(e1) / args.steps * 1e3)
        mp, ms = float(np.median(t["plan"])), float(np.median(t["share"]))
        say(f"{noise:9s} D={D:3d}: plan order median {mp:7.2f} us (min {min(t['plan']):7.2f}, max {max(t['plan']):7.2f}) | share "
            f"order median {ms:7.2f} us (min {min(t['share']):7.2f}, max {max(t['share']):7.2f}) | {ms - mp:+6.2f} us "
            f"({(ms - mp) / mp * 100:+5.2f} %), {args.rounds} rounds x {args.steps} launches, outputs bit-identical")
        if (noise, D) == shapes[0]:
            saving = mp - ms
    if saving and saving > 0:
        say(f"threshold: {build_ms * 1e3:.0f} us build / {saving:.2f} us saved per headline launch = "
            f"{int(np.ceil(build_ms * 1e3 / saving))} launches")
    else:
        say(f"threshold: none — the headline launch saves {saving if saving is None else round(saving, 2)} us")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
