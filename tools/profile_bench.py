#!/usr/bin/env python
"""Regenerate the profiles/<round>/ files for the bench workload into gpurun_out/profiles/<round>/
(run on the GPU box, from the repo root; copy them into profiles/<round>/ afterwards):

    python tools/profile_bench.py --round r01 [--noise normal] [--feat 128]

Passes (each its own process; counters never share a run with a trace domain):
  1. rocprofv3 --kernel-trace --stats   -> bench_n1_kernel_stats.csv + the bench line (bench_n1.json)
  2. rocprofv3 --pmc FETCH_SIZE         |
  3. rocprofv3 --pmc WRITE_SIZE         |-> bench_n1_pmc_summary.json (per-dispatch averages of the
  4. rocprofv3 --pmc <SQ counters>      |   aggregation kernel, gfx950 FETCH_SIZE correction spelled out)
This script never touches the GPU itself; the profiled program is `python3 bench.py ...` directly
after `--`.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = None      # --lib: a build variant (tools/_bin/libstag_<name>.so) instead of stag_amd/libstag_hip.so
# Two SQ passes, each with its OWN cycle counter: a ratio is formed from counters of one pass only (round 3 divided
# counters of one replay by the cycles of another, at another clock: "VALU busy" 1.049 — VERDICT r03)
SQ_A = ["SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "GRBM_GUI_ACTIVE"]
SQ_B = ["SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_INSTS_VMEM_RD", "GRBM_GUI_ACTIVE"]


def derived(a, b):
    """Ratios from the two SQ passes (a: SQ_A's per-dispatch averages, b: SQ_B's), each normalised by the cycles counted
    in ITS pass.  GRBM_GUI_ACTIVE is summed over the 8 XCDs; SQ_ACTIVE_INST_VALU counts quad-cycles (x4 = SIMD cycles
    issuing VALU; 1024 SIMDs).  A busy fraction cannot exceed 1: a raw value above it (counter granularity, the replay's
    clock) is reported as 1.0 with `valu_saturated`."""
    out = {}
    if b.get("GRBM_GUI_ACTIVE"):
        cyc = b["GRBM_GUI_ACTIVE"] / 8.0
        raw = b["SQ_ACTIVE_INST_VALU"] * 4.0 / (1024.0 * cyc)
        out.update({"valu_busy_frac": min(raw, 1.0), "valu_busy_frac_raw": raw, "valu_saturated": raw >= 0.995,
                    "cycles_per_valu_inst": b["SQ_ACTIVE_INST_VALU"] * 4.0 / max(b["SQ_INSTS_VALU"], 1.0),
                    "xcd_cycles_valu_pass": cyc})
    if a.get("GRBM_GUI_ACTIVE"):
        cyc = a["GRBM_GUI_ACTIVE"] / 8.0
        out.update({"avg_waves_per_simd": a["SQ_WAVE_CYCLES"] * 4.0 / (1024.0 * cyc),
                    "wait_frac_of_wave_life": a["SQ_WAIT_ANY"] / max(a["SQ_WAVE_CYCLES"], 1.0),
                    "xcd_cycles_wave_pass": cyc})
    if a.get("SQ_WAVES") and b.get("SQ_INSTS_VALU"):
        out["valu_insts_per_wave"] = b["SQ_INSTS_VALU"] / max(a["SQ_WAVES"], 1.0)    # (both are counts: no clock in it)
    return out


def run_prof(tag, prof_args, bench_args, scratch):
    out = os.path.join(scratch, tag)
    cmd = ["rocprofv3", *prof_args, "-d", out, "-o", tag, "--output-format", "csv", "--",
           "python3", "bench.py", *bench_args]
    print("+", " ".join(cmd), flush=True)
    env = dict(os.environ, TMPDIR="/tmp", **({"STAG_HIP_SO": LIB} if LIB else {}))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{tag}: rocprofv3 exited {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    return out, (json.loads(line[-1]) if line else None)


def find(out, suffix):
    hits = glob.glob(os.path.join(out, "**", f"*{suffix}"), recursive=True)
    if not hits:
        raise SystemExit(f"no *{suffix} under {out}")
    return hits[0]


def counters(out, kernel_sub):
    """Per-dispatch averages of each counter for dispatches of the aggregation kernel."""
    f = find(out, "counter_collection.csv")
    per = {}
    disp = set()
    name = None
    for row in csv.DictReader(open(f)):
        if not any(s in row["Kernel_Name"] for s in kernel_sub):
            continue
        name = row["Kernel_Name"]
        disp.add(row["Dispatch_Id"])
        per.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    n = max(len(disp), 1)
    # a counter can appear once per dimension instance (XCD, SE ...): sum instances, average dispatches
    return name, len(disp), {k: sum(v) / n for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--round", default="r01")
    ap.add_argument("--noise", default="normal")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--graph", default="arxiv")
    ap.add_argument("--seg-len", type=int, default=64)
    ap.add_argument("--workload", default="agg", choices=["agg", "gat"])
    ap.add_argument("--tag", default="n1", help="file-name tag: bench_<tag>.json, bench_<tag>_kernel_stats.csv, ...")
    ap.add_argument("--lib", default=None, help="profile a build variant: path of its libstag_*.so")
    ap.add_argument("--summarize-only", action="store_true",
                    help="rebuild the summaries from the CSVs already under gpurun_out/prof/ (no GPU needed)")
    args = ap.parse_args()
    global LIB
    LIB = os.path.abspath(args.lib) if args.lib else None
    if args.summarize_only:
        global run_prof
        run_prof = lambda tag, prof_args, bench_args, scratch: (os.path.join(scratch, tag), None)
    scratch = os.path.join(ROOT, "gpurun_out", "prof" if args.tag == "n1" else f"prof_{args.tag}")
    # only gpurun_out/ travels back from the GPU box: copy the result into profiles/<round>/ afterwards
    dst = os.path.join(ROOT, "gpurun_out", "profiles", args.round)
    os.makedirs(dst, exist_ok=True)
    common = ["--noise", args.noise, "--feat", str(args.feat), "--graph", args.graph,
              "--seg-len", str(args.seg_len), "--workload", args.workload, "--no-cpu-baseline", "--no-variants"]   # one workload per profile
    # (the plain forward launch of a kind that draws runs agg_plain_kernel: csrc/agg_plain.hpp)
    kernel_sub = ("gat_fwd",) if args.workload == "gat" else ("agg_kernel", "agg_plain_kernel")

    out, line = run_prof("stats", ["--kernel-trace", "--stats"], ["--steps", "200", "--warmup", "20", *common], scratch)
    stats = find(out, "kernel_stats.csv")
    rows = list(csv.DictReader(open(stats)))
    with open(os.path.join(dst, f"bench_{args.tag}_kernel_stats.csv"), "w") as f:
        f.write(open(stats).read())
    agg = [r for r in rows if any(s in r["Name"] for s in kernel_sub)]
    print("kernel stats:", [(r["Name"][:60], r["Calls"], r["AverageNs"]) for r in agg])
    if line:
        with open(os.path.join(dst, f"bench_{args.tag}.json"), "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")

    summary = {}
    short = ["--steps", "20", "--warmup", "5", "--settle-ms", "0", *common]     # counters do not need warm clocks
    for tag, ctrs in (("pmc_fetch", ["FETCH_SIZE"]), ("pmc_write", ["WRITE_SIZE"]), ("pmc_sq_a", SQ_A), ("pmc_sq_b", SQ_B)):
        out, _ = run_prof(tag, ["--pmc", *ctrs], short, scratch)
        name, nd, avg = counters(out, kernel_sub)
        summary[tag] = {"kernel": name, "dispatches": nd, "counters_avg_per_dispatch": avg}
    fetch_kb = summary["pmc_fetch"]["counters_avg_per_dispatch"]["FETCH_SIZE"]
    write_kb = summary["pmc_write"]["counters_avg_per_dispatch"]["WRITE_SIZE"]
    summary["traffic"] = {
        "workload": (f"{args.graph}/{args.noise}/D{args.feat}/seg{args.seg_len}" if args.workload == "agg" else
                     f"{args.graph}/gat8x32/{args.noise}/seg{args.seg_len}"),
        "fetch_size_kb": fetch_kb, "write_size_kb": write_kb,
        "correction": "gfx950: FETCH_SIZE counts 128-B fabric read requests at 64 B => x2 for 16-B-per-lane "
                      "loads (MI355X_MICROARCH.md HBM); WRITE_SIZE exact for 16-B-per-lane stores",
        "traffic_bytes_per_launch": (2.0 * fetch_kb + write_kb) * 1024.0,
        "note": "counters sit on the fabric side of L2 and include Infinity-Cache hits: x (86.7 MB) stays "
                "resident in the 256 MB Infinity Cache (an nt gather, which bypasses it, is 36 % slower), so "
                "this is L2-miss traffic, an upper bound on HBM bytes"}
    d = derived(summary["pmc_sq_a"]["counters_avg_per_dispatch"], summary["pmc_sq_b"]["counters_avg_per_dispatch"])
    if agg and d:
        dur_us = float(agg[0]["AverageNs"]) / 1e3
        d["kernel_avg_us_from_stats_pass"] = dur_us
        summary["derived"] = d
    with open(os.path.join(dst, f"bench_{args.tag}_pmc_summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps(summary["traffic"], indent=1))


if __name__ == "__main__":
    main()
