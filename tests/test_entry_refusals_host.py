"""The return code of every entry point that takes a csr, a plan and a noise spec, for a base call, every single fault of
a fixed list and every pair of them, against the codes recorded from the parent of the change that moved these checks
into stag_amd/csrc/entry_args.hpp (tests/golden/entry_refusals.json).  Nothing is dereferenced: a small real indptr,
dummy values for device pointers.  Cases that get past the checks reach a launch, so they are replayed only where no
device is present.

Recording (by hand, against a library built from the parent commit, on a machine without a GPU):
    STAG_HIP_SO=<parent libstag_hip.so> python tests/test_entry_refusals_host.py record <parent commit id>
and, once the branch's library is built, the list of tightenings:
    python tests/test_entry_refusals_host.py tightened
"""
import ctypes as C
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "entry_refusals.json")
OK, EINVAL, ENOMEM, ENOSYS = 0, -22, -12, -38
LETTER = {OK: "k", EINVAL: "I", ENOSYS: "S", ENOMEM: "M"}     # anything else ("L"): the call reached a launch
P = 16                       # a non-null, 16-byte aligned dummy "device pointer"
NORMAL, UNIFORM, EXPLICIT = 2, 3, 1
D, H, F = 8, 8, 4            # two chunks of 4 channels (D, and H for the GAT draws); H * F = 32
GAT_ROW = ((H * F + 2 * H + 3) & ~3) * 4

_INDPTR = np.array([0, 1, 2], np.int32)
_UNITS = np.zeros((4, 4), np.int32)

CSR0 = dict(n_dst=2, n_src=2, n_edges=2, indptr=_INDPTR.ctypes.data, indices=P, eid=P, nidx=P)
SPEC0 = dict(kind=NORMAL, param_mode=0, p0=None, p1=None, p0_scalar=1.0, p1_scalar=0.5, relu=0, in_norm=0, deriv=0, group=0,
             seed=1, offset=2, pos_base=0, chunk_base=0, p1_log=0, epoch=None)
# a plan with one long row of one segment, an XCD order and a block plan: every field a check reads is there
PLAN0 = dict(seg_len=64, n_units=3, n_long=1, n_seg=1, units=_UNITS.ctypes.data, long_rows=P, long_seg_ptr=P, seg_counters=P,
             workspace=P, workspace_bytes=0, n_heavy=1, n_blocks=1, block_ptr=P, xcd_order=P, xcd_stride_heavy=1,
             xcd_stride_light=2)
DROP0 = dict(keep_prob=1.0, seed=3, offset=4, epoch=None)

PE1 = dict(param_mode=2, p0=P, p1=P)
_GAT_BWD = ["csr", "plan", "csr_t", "plan_t", "el", "er", "ft", "stats", "g", "out", "H", "F", "neg_slope", "spec", "norm_scale",
            "drop", "d_el", "d_er", "d_ft"]
_GAT_BWD_WS = max(H, H * F + H) * 4

# name -> (argument names in order, values of the base call that differ from the defaults below, exact workspace bytes)
ENTRIES = {
    "stag_agg_fwd": ("csr plan x ldx D spec reduce src_scale dst_scale out ldo norm_scale stream".split(), {}, D * 4),
    "stag_agg_fwd_mc": ("csr plan x ldx D spec n_samples offset_stride reduce src_scale dst_scale out ldo sample_stride stream".split(),
                        dict(n_samples=3, sample_stride=2 * D), 2 * D * 4),
    "stag_agg_bwd": ("csr plan x ldx D spec src_scale dst_scale out dp0 dp1 ldo stream".split(), {}, 3 * D * 4),
    "stag_agg_bwd_edge": ("csr plan g ldg D spec src_scale dst_scale x ldx out ldo dp0 dp1 stream".split(), dict(spec=PE1), D * 4),
    "stag_agg_bwd_dp": ("csr plan g ldg D spec src_scale dst_scale x ldx out ldo dp0 dp1 workspace workspace_bytes stream".split(),
                        dict(workspace_bytes=1 << 20), D * 4),
    "stag_noise_materialize": ("csr plan spec D out ldo norm_scale stream".split(), {}, 2 * D * 4),
    "stag_agg_bwd_w": ("csr plan x ldx g ldg D src_scale spec reduce_k out dw1 ldo stream".split(), dict(dw1=None), 32),
    "stag_agg_max_fwd": ("csr plan x ldx D spec out ldo cnt ldc stream".split(), {}, 2 * D * 4),
    "stag_agg_max_bwd": ("csr plan x ldx out cnt g ldg D spec dx dw ldw dp0 dp1 ldd scratch scratch_bytes stream".split(),
                         dict(dw=None, dp0=None, dp1=None, scratch_bytes=1 << 20), D * 4),
    "stag_agg_fwd_half": ("csr plan x x_dtype ldx D spec reduce src_scale dst_scale out ldo stream".split(), {}, D * 4),
    "stag_gat_fwd": ("csr plan el er ft H F neg_slope spec norm_scale drop out stats stream".split(), {}, GAT_ROW),
    "stag_gat_fwd_mc": ("csr plan el er ft H F neg_slope spec n_samples offset_stride out out_stride stats stats_stride stream".split(),
                        dict(n_samples=2, out_stride=2 * H * F, stats_stride=2 * 2 * H), 2 * GAT_ROW),
    "stag_gat_attn": ("csr plan el er H neg_slope spec norm_scale stats attn_out stream".split(), {}, 32),
    "stag_gat_bwd_edge": ("csr plan el er ft stats g out H F neg_slope spec norm_scale de dw attn_out stream".split(), {}, 32),
    "stag_gat_bwd_two_pass": (_GAT_BWD + ["dw", "scratch", "stream"], {}, _GAT_BWD_WS),
    "stag_gat_bwd": (_GAT_BWD + ["dw", "scratch", "stream"], {}, _GAT_BWD_WS),
    "stag_gat_bwd_stages": (_GAT_BWD + ["scratch", "stages", "stream"], {}, _GAT_BWD_WS),
    "stag_gat_bwd_dp": (_GAT_BWD + ["dp0", "dp1", "scratch", "workspace", "workspace_bytes", "stream"],
                        dict(workspace_bytes=1 << 20), _GAT_BWD_WS),
}
STRUCTS = dict(csr=CSR0, csr_t=CSR0, spec=SPEC0, plan=PLAN0, plan_t=PLAN0, drop=DROP0)
SCALARS = dict(ldx=D, ldg=D, ldo=D, ldw=D, ldc=D, ldd=D, D=D, H=H, F=F, neg_slope=0.2, reduce=0, reduce_k=0, x_dtype=2,
               n_samples=1, offset_stride=1, stages=7, stream=None)
LDS = ("ldx", "ldg", "ldo", "ldw", "ldc", "ldd", "sample_stride", "out_stride", "stats_stride")
ALIGNED = ("x", "ft", "g", "out")          # pointers whose misalignment the fault list asks for


def base_call(name):
    names, over, ws = ENTRIES[name]
    call = {}
    for n in names:
        if n in STRUCTS:
            call[n] = dict(STRUCTS[n])
            if n in ("plan", "plan_t"):
                call[n]["workspace_bytes"] = ws
        else:
            call[n] = SCALARS.get(n, P)     # every other argument is a pointer
    for n, v in over.items():
        if isinstance(v, dict):
            call[n].update(v)
        else:
            call[n] = v
    return call


def _set(arg, **fields):
    def apply(call):
        if not isinstance(call.get(arg), dict):
            return False
        call[arg].update(fields)
        return True
    return apply


def _arg(arg, value):
    def apply(call):
        if arg not in call:
            return False
        call[arg] = value(call[arg]) if callable(value) else value
        return True
    return apply


def _in_norm(with_factor):
    def apply(call):
        if not isinstance(call.get("spec"), dict):
            return False
        call["spec"]["in_norm"] = 1
        if "norm_scale" in call:
            call["norm_scale"] = P if with_factor else None
        return True
    return apply


def _short(plan):
    def apply(call):
        if not isinstance(call.get(plan), dict):
            return False
        call[plan]["workspace_bytes"] -= 1
        return True
    return apply


SPEC_FAULTS = [
    ("kind=9", dict(kind=9)), ("param_mode=9", dict(param_mode=9)), ("deriv=1", dict(deriv=1)), ("deriv=3", dict(deriv=3)),
    ("p1_log,uniform", dict(kind=UNIFORM, p1_log=1)), ("p1_log,per-channel", dict(param_mode=1, p0=P, p1=P, p1_log=1)),
    ("chunk_base=-1", dict(chunk_base=-1)), ("chunk_base=2^20", dict(chunk_base=1 << 20)),
    ("chunk_base=2^20-1", dict(chunk_base=(1 << 20) - 1)),
    ("pos_base=-1", dict(pos_base=-1)), ("pos_base=2^44-1", dict(pos_base=(1 << 44) - 1)),
    ("pos_base=2^32-1", dict(pos_base=(1 << 32) - 1)),
    ("per-channel,p0=NULL", dict(param_mode=1, p0=None, p1=P)), ("per-channel,p1=NULL", dict(param_mode=1, p0=P, p1=None)),
    ("per-edge,p0=NULL", dict(param_mode=3, p0=None, p1=P)), ("per-edge,p1=NULL", dict(param_mode=3, p0=P, p1=None)),
    ("explicit,p0=NULL", dict(kind=EXPLICIT, p0=None)), ("explicit,group=3", dict(kind=EXPLICIT, p0=P, group=3)),
]
PLAN_FAULTS = [
    ("units=NULL", dict(units=None)), ("units=misaligned", dict(units=_UNITS.ctypes.data + 8)),
    ("long_rows=NULL", dict(long_rows=None)), ("long_seg_ptr=NULL", dict(long_seg_ptr=None)),
    ("workspace=NULL", dict(workspace=None)), ("seg_counters=NULL", dict(seg_counters=None)),
    ("n_heavy>n_units", dict(n_heavy=4)), ("n_seg=-1", dict(n_seg=-1)), ("n_long=-1", dict(n_long=-1)),
    ("xcd_order=misaligned", dict(xcd_order=24)), ("xcd_sh=-1", dict(xcd_stride_heavy=-1)), ("xcd_sl=-1", dict(xcd_stride_light=-1)),
    ("xcd_sh>n_heavy", dict(xcd_stride_heavy=2)), ("xcd_sl>n_units", dict(xcd_stride_light=4)),
    ("xcd_strides_short", dict(xcd_stride_heavy=0, xcd_stride_light=0)),
    ("xcd_strides_overflow", dict(n_units=(1 << 31) - 1, n_heavy=(1 << 31) - 1, xcd_stride_heavy=1 << 28, xcd_stride_light=1 << 28)),
    ("block_ptr=NULL", dict(block_ptr=None)), ("seg_len=257", dict(seg_len=257)),
]


def fault_list(name):
    """(fault name, function that applies it to a call) for every fault of the fixed list that names an argument of `name`."""
    names = ENTRIES[name][0]
    out = []
    for n in names:                                       # NULL for each pointer argument
        if n not in SCALARS and n not in LDS and not n.endswith("_bytes"):
            out.append((n + "=NULL", _arg(n, None)))
    out += [(n + "=misaligned", _arg(n, 24)) for n in names if n in ALIGNED]
    for c in ("csr", "csr_t"):
        if c in names:
            out += [("%s.%s=%s" % (c, k, t), _set(c, **{k: v})) for k, t, v in (
                ("n_dst", "-1", -1), ("n_dst", "0", 0), ("n_src", "-1", -1), ("n_edges", "-1", -1), ("n_edges", "2^31", 1 << 31),
                ("indptr", "NULL", None), ("indices", "NULL", None))]
    for n in ("D", "H", "F"):
        if n in names:
            out += [(n + "=0", _arg(n, 0)), (n + "=-4", _arg(n, -4))]
    out += [(n + "=width-1", _arg(n, lambda v: v - 1)) for n in names if n in LDS]
    if "reduce" in names:
        out.append(("reduce=2", _arg("reduce", 2)))
    if "x_dtype" in names:
        out.append(("x_dtype=0", _arg("x_dtype", 0)))
    out += [("spec." + t, _set("spec", **kw)) for t, kw in SPEC_FAULTS]
    out += [("spec.in_norm,no_factor", _in_norm(False)), ("spec.in_norm,factor", _in_norm(True))]
    for p in ("plan", "plan_t"):
        if p in names:
            out += [("%s.%s" % (p, t), _set(p, **kw)) for t, kw in PLAN_FAULTS]
            out.append((p + ".workspace_bytes-1", _short(p)))
    return out


def cases(name):
    """(case id, call) in the fixed order: the base call, every single fault, every pair (the first applied first)."""
    faults = fault_list(name)
    yield name + ":base", base_call(name)
    for t, f in faults:
        call = base_call(name)
        f(call)
        yield "%s:%s" % (name, t), call
    for (t1, f1), (t2, f2) in itertools.combinations(faults, 2):
        call = base_call(name)
        f1(call)
        f2(call)
        yield "%s:%s+%s" % (name, t1, t2), call


def run(lib, _lib, name, call):
    types = dict(csr=_lib.Csr, csr_t=_lib.Csr, spec=_lib.NoiseSpec, plan=_lib.Plan, plan_t=_lib.Plan, drop=_lib.GatDrop)
    keep, args = [], []
    for n in ENTRIES[name][0]:
        v = call[n]
        if isinstance(v, dict):
            s = types[n]()
            for k, x in v.items():
                setattr(s, k, x)
            keep.append(s)
            v = C.byref(s)
        args.append(v)
    return getattr(lib, name)(*args)


def letters(lib, _lib, name):
    return "".join(LETTER.get(run(lib, _lib, name, call), "L") for _, call in cases(name))


# The only way a call that reached a launch may now be refused: a GAT entry point given n_src < 0 or n_edges > 2^31 - 1,
# which the rest of check_csr refuses after every refusal the entry point had (so no refusal changed its code).
_GAT = ("stag_gat_fwd", "stag_gat_fwd_mc", "stag_gat_attn", "stag_gat_bwd_edge", "stag_gat_bwd_two_pass", "stag_gat_bwd",
        "stag_gat_bwd_stages", "stag_gat_bwd_dp")
TIGHTENING_SHAPES = [
    (_GAT, ("csr.n_src=-1", "csr_t.n_src=-1", "csr.n_edges=2^31", "csr_t.n_edges=2^31"),
     "GAT entry point: n_src < 0 or n_edges > 2^31 - 1 is now refused by the shared check_csr"),
]


def _reason(case_id):
    name, faults = case_id.split(":", 1)
    for names, shape, reason in TIGHTENING_SHAPES:
        if name in names and any(f in shape for f in faults.split("+")):
            return reason
    return None


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def replay():
    """(case id, recorded letter, the branch's letter or None where the case was not run) for every case."""
    from stag_amd import _lib
    lib, gold, device = _lib.lib(), _golden(), torch.cuda.is_available()
    tightened = {t["case"] for t in gold["tightened"]}
    rows = []
    for name in ENTRIES:
        rec = gold["codes"][name]
        ids = list(cases(name))
        assert len(rec) == len(ids), name
        for (cid, call), r in zip(ids, rec):
            # a recorded refusal (or OK before any device work) must come back; a tightened case must be refused now,
            # so with the branch's library neither runs a kernel.  Everything else launches on dummy pointers.
            safe = r in "kISM" or cid in tightened
            rows.append((cid, r, LETTER.get(run(lib, _lib, name, call), "L") if (safe or not device) else None))
    return rows, gold


def test_every_entry_point_and_fault_is_enumerated():
    gold = _golden()
    assert set(gold["codes"]) == set(ENTRIES) and len(ENTRIES) == 18
    assert re.fullmatch(r"[0-9a-f]{40}", gold["parent"])
    for name in ENTRIES:
        n = len(fault_list(name))
        assert len(gold["codes"][name]) == 1 + n + n * (n - 1) // 2, name
        assert gold["codes"][name][0] == "L", name            # the base call passes every check


def test_recorded_refusals_are_returned_unchanged(replay):
    rows, gold = replay
    tightened = {t["case"] for t in gold["tightened"]}
    wrong = [(cid, r, got) for cid, r, got in rows if r in "kISM" and got != r]
    assert not wrong, wrong[:20]
    # nothing that is not listed as tightened may have become a refusal (checked where the launches can be replayed)
    wrong = [(cid, r, got) for cid, r, got in rows if r == "L" and got is not None and got != "L" and cid not in tightened]
    assert not wrong, wrong[:20]


def test_tightenings_are_listed_and_of_the_allowed_kind(replay):
    rows, gold = replay
    by_id = {cid: (r, got) for cid, r, got in rows}
    for t in gold["tightened"]:
        assert t["parent"] == "reached a launch" and t["new"] == EINVAL, t
        assert t["reason"] == _reason(t["case"]), t                       # one of the three allowed shapes
        assert by_id[t["case"]] == ("L", "I"), (t, by_id[t["case"]])


def test_two_pass_checks_the_transposed_plan_before_any_launch(replay):
    rows, _ = replay
    by_id = {cid: (r, got) for cid, r, got in rows}
    for f in ("units=NULL", "units=misaligned", "long_rows=NULL", "long_seg_ptr=NULL"):
        assert by_id["stag_gat_bwd_two_pass:plan_t." + f] == ("I", "I"), f
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "gat.hip")).read()
    body = src[src.index('extern "C" int stag_gat_bwd_two_pass('):]
    body = body[:body.index('extern "C" size_t stag_gat_bwd_scratch_bytes')]
    first_launch = body.index("hipLaunchKernelGGL")
    assert "return STAG_E" not in body[first_launch:].replace("STAG_EIO", "")     # every refusal comes before it
    assert "plan_t" in body[:first_launch]


@pytest.mark.skipif(torch.cuda.is_available(), reason="cases that pass every check launch on dummy pointers: no device may be present")
def test_cases_that_reached_a_launch_are_still_not_refused(replay):
    rows, gold = replay
    tightened = {t["case"] for t in gold["tightened"]}
    wrong = [(cid, got) for cid, r, got in rows if r == "L" and cid not in tightened and got in "ISM"]
    assert not wrong, wrong[:20]


def _record(parent):
    from stag_amd import _lib
    assert not torch.cuda.is_available(), "record where no device is present: the accepted cases launch on dummy pointers"
    gold = dict(parent=parent, legend="k: STAG_OK, I: STAG_EINVAL, S: STAG_ENOSYS, M: STAG_ENOMEM, L: reached a launch; "
                "one letter per case, in the order of cases()", codes={n: letters(_lib.lib(), _lib, n) for n in ENTRIES},
                tightened=[])
    with open(GOLDEN, "w") as fh:
        json.dump(gold, fh, indent=0)


def _list_tightened():
    from stag_amd import _lib
    assert not torch.cuda.is_available()
    gold = _golden()
    gold["tightened"] = []
    for name in ENTRIES:
        for (cid, _), r, got in zip(cases(name), gold["codes"][name], letters(_lib.lib(), _lib, name)):
            if r == "L" and got == "I":
                gold["tightened"].append(dict(case=cid, parent="reached a launch", new=EINVAL, reason=_reason(cid)))
    with open(GOLDEN, "w") as fh:
        json.dump(gold, fh, indent=0)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "record":
        _record(sys.argv[2])
    elif sys.argv[1] == "tightened":
        _list_tightened()
