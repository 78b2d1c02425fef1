"""Compiled resources of agg_plain_kernel (csrc/agg_plain.hpp), from the compiler's report that the Makefile keeps
next to the objects: every instantiation is built for the occupancy the kernel asks for (amdgpu_waves_per_eu, both
bounds: STAG_PLAIN_WAVES = 7 waves per SIMD), within the 72 VGPRs that leaves, without scratch."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_WAVES = 7


def test_plain_kernel_resources():
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    hpp = open(os.path.join(csrc, "agg_plain.hpp")).read()
    assert re.search(r"#define STAG_PLAIN_WAVES (\d+)", hpp).group(1) == str(PLAIN_WAVES)
    seen = set()
    for kind, code in (("normal", 2), ("uniform", 3), ("bernoulli", 4)):
        text = open(os.path.join(csrc, "_obj", f"agg_plain_{kind}.remarks")).read()
        for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                             r"Occupancy \[waves/SIMD\]: (\d+)", text, re.S):
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            if "agg_plain_kernel<" not in name:
                continue
            vgprs, scratch, occ = (int(m.group(i)) for i in (2, 3, 4))
            assert occ == PLAIN_WAVES and vgprs <= 72 and scratch == 0, f"{name}: {vgprs} VGPRs, {scratch} B scratch, {occ} waves/SIMD"
            seen.add(name)
        # 32 and 64 lanes per row x relu x the plan-order kernel and its walk twin
        for lpe in (32, 64):
            for relu in ("false", "true"):
                for walk in ("false", "true"):
                    assert f"void stag::agg_plain_kernel<{code}, {lpe}, {relu}, {walk}>(stag::AggArgs)" in seen
    assert len(seen) == 24
