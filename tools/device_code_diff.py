#!/usr/bin/env python
"""Is the device code of one source tree still that of another?  Host-only: hipcc cross-compiles, no GPU is used.

  python tools/device_code_diff.py PARENT_TREE BRANCH_TREE [--rename OLD=NEW ...] [--only gat.hip ...] [--jobs 8]

Every .hip of the Makefile's SRCS is compiled in both trees with the Makefile's CXXFLAGS plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`.  Each .s is split into its functions (`.type <sym>,@function`
up to `.end_amdhsa_kernel`) and compared function by function, by name, and so are the resource lines of each kernel.
Left aside: lines naming `__hip_cuid_` (a hash of the source text) and the numbers in local labels (.LBB<n>_<m>,
.Lfunc_end<n>, .Ltmp<n>: <n> counts functions or labels in emission order, which moves when a template is reordered or
a launch site instantiates its kernels in another order), the same <n> where a loop note names a block (`; in Loop:
Header=BB<n>_<m>`, `; Child Loop BB<n>_<m>`) and the padding in front of a comment, whose column moves with the width of <n>.
--rename rewrites mangled-name fragments of PARENT_TREE's output (all pairs in one pass) for a refactor that renames
kernels.  The texts are hashed and compared; nothing in them is interpreted.  Exit status 1 when anything differs."""
import argparse
import concurrent.futures as cf
import hashlib
import os
import re
import subprocess
import sys
import tempfile

EXTRA = ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


def make_var(csrc, name):
    out = subprocess.run(["make", "-s", "-C", csrc, "--no-print-directory", "--eval", f"_show: ; @echo $({name})", "_show"],
                         check=True, capture_output=True, text=True).stdout
    return out.split()


def compile_one(cmd, csrc, src, outdir):
    s, rem = os.path.join(outdir, src[:-4] + ".s"), os.path.join(outdir, src[:-4] + ".remarks")
    with open(rem, "w") as err:
        rc = subprocess.run([*cmd, src, "-o", s], cwd=csrc, stderr=err).returncode
    if rc:
        sys.exit(f"{csrc}/{src} does not compile:\n" + open(rem).read()[-4000:])
    return open(s).read(), open(rem).read()


def renamer(pairs):
    if not pairs:
        return lambda text: text
    table = dict(p.split("=", 1) for p in pairs)
    rx = re.compile("|".join(re.escape(k) for k in sorted(table, key=len, reverse=True)))
    return lambda text: rx.sub(lambda m: table[m.group(0)], text)


def functions(asm):
    """{symbol: hash of its normalised text}, from `.type <sym>,@function` to `.end_amdhsa_kernel` (or the next function)"""
    out, cur, body = {}, None, []

    def close():
        if cur is None:
            return
        tmp = {}
        text = "\n".join(body)
        text = re.sub(r"(\.L|\b)BB\d+_(\d+)", r"\1BB#_\2", text)
        text = re.sub(r"[ \t]+;", " ;", text)
        text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", text)
        text = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp#%d" % tmp.setdefault(m.group(0), len(tmp)), text)
        out[cur] = hashlib.sha256(text.encode()).hexdigest()

    for line in asm.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            close()
            cur, body = m.group(1), []
        if cur is not None and "__hip_cuid_" not in line:
            body.append(line)
        if cur is not None and line.strip() == ".end_amdhsa_kernel":
            close()
            cur = None
    close()
    return out


def resources(remarks):
    """{kernel: its resource lines}, source positions left aside"""
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = []
            continue
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if m and cur:
            res[cur].append(m.group(1))
    return res


def differing(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--rename", nargs="*", default=[], metavar="OLD=NEW")
    ap.add_argument("--only", nargs="*", default=None, metavar="X.hip")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    csrc = [os.path.join(os.path.abspath(t), "stag_amd", "csrc") for t in (args.parent, args.branch)]
    srcs = args.only or make_var(csrc[1], "SRCS")
    rename = renamer(args.rename)
    print("flags:", " ".join(make_var(csrc[1], "CXXFLAGS") + EXTRA))
    for pair in args.rename:
        print("rename (parent's symbols):", pair.replace("=", " -> "))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(args.jobs) as pool:
        jobs = {}
        for i, side in enumerate(("parent", "branch")):
            os.makedirs(os.path.join(tmp, side))
            cmd = make_var(csrc[i], "HIPCC") + make_var(csrc[i], "CXXFLAGS") + EXTRA
            for src in srcs:
                if os.path.exists(os.path.join(csrc[i], src)):
                    jobs[side, src] = pool.submit(compile_one, cmd, csrc[i], src, os.path.join(tmp, side))
        for src in srcs:
            if ("parent", src) not in jobs or ("branch", src) not in jobs:
                print(f"{src:26s} only in one tree")
                bad += 1
                continue
            (pa, pr), (ba, br) = jobs["parent", src].result(), jobs["branch", src].result()
            fp, fb = functions(rename(pa)), functions(ba)
            rp, rb = resources(rename(pr)), resources(br)
            df, dr = differing(fp, fb), differing(rp, rb)
            print(f"{src:26s} {len(fb):4d} functions, {len(df)} differ   {len(rb):4d} resource reports, {len(dr)} differ")
            for k in df + [k for k in dr if k not in df]:
                print("    differs:", k)
            bad += len(df) + len(dr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
