"""stag_edge_embed_fwd / _bwd (the wide edge embedding of an AmortizedDistribution) on the host: ABI surface, every refusal
before any device work, the compiler's resource report of the new kernels, the routing predicate of
AmortizedDistribution.condition, and the timing tool."""
import ctypes as C
import os
import py_compile
import re
import subprocess
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ENOSYS = -22, -12, -38


def test_header_declares_and_library_exports_the_entries():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    fwd = re.search(r"int stag_edge_embed_fwd\s*\(([^;]*)\);", header)
    bwd = re.search(r"int stag_edge_embed_bwd\s*\(([^;]*)\);", header)
    assert fwd and bwd, "prototypes"
    assert re.sub(r"\s+", " ", fwd.group(1)) == (
        "const int32_t* src, const int32_t* dst, int64_t n_edges, const float* ps, int64_t ldps, const float* pd, "
        "int64_t ldpd, int32_t hidden, float* h, int64_t ldh, void* stream")
    assert re.sub(r"\s+", " ", bwd.group(1)) == (
        "const stag_csr* view, const stag_plan* plan, const float* own, int64_t ld_own, const float* other, "
        "int64_t ld_other, int32_t hidden, const float* g, int64_t ldg, float* d_own, int64_t ldd, void* stream")
    assert hasattr(_lib.lib(), "stag_edge_embed_fwd") and hasattr(_lib.lib(), "stag_edge_embed_bwd")
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19      # additive
    para = header[:fwd.start()].rsplit("/* ----", 1)[1]
    for word in ("SiLU'", "expf", "summed from", "segment order", "STAG_EINVAL", "STAG_ENOMEM", "written as zeros"):
        assert word in para, word


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, indptr.ctypes.data, None, None)   # never dereferenced
    return _lib, _lib.lib(), indptr, csr, C.c_void_p(16)     # f: a non-null, 16-B aligned dummy "device pointer"


# argument positions
SRC, DST, NE, PS, LDPS, PD, LDPD, HID, H, LDH, FSTREAM = range(11)
VIEW, PLAN, OWN, LDOWN, OTHER, LDOTHER, BHID, G, LDG, DOWN, LDD, BSTREAM = range(12)


def _fwd_ok(f):
    return [f, f, 2, f, 8, f, 8, 8, f, 8, None]


def _bwd_ok(csr, f):
    return [C.byref(csr), None, f, 8, f, 8, 8, f, 8, f, 8, None]


def test_forward_entry_refuses_invalid_arguments_without_gpu():
    _lib, lib, _keep, _csr, f = _fixture()
    call = lambda a: lib.stag_edge_embed_fwd(*a)
    for pos in (SRC, DST, PS, PD, H):                                      # a NULL ids / table / output with edges
        a = _fwd_ok(f); a[pos] = None
        assert call(a) == EINVAL, pos
    for hid in (0, -4):                                                    # hidden <= 0
        a = _fwd_ok(f); a[HID] = hid
        assert call(a) == EINVAL
    for pos in (LDPS, LDPD, LDH):                                          # a row stride smaller than hidden
        a = _fwd_ok(f); a[pos] = 7
        assert call(a) == EINVAL, pos
        a = _fwd_ok(f); a[pos] = 0
        assert call(a) == EINVAL, pos
    a = _fwd_ok(f); a[NE] = -1
    assert call(a) == EINVAL
    a = _fwd_ok(f); a[NE] = 1 << 31                                        # int32 edge ids
    assert call(a) == EINVAL
    # no edges: nothing to do, whatever the pointers — but the shape is still checked
    a = _fwd_ok(f); a[NE] = 0
    for pos in (SRC, DST, PS, PD, H):
        a[pos] = None
    assert call(a) == 0
    a[HID] = 0
    assert call(a) == EINVAL


def test_backward_entry_refuses_invalid_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_edge_embed_bwd(*a)
    for pos in (VIEW, OWN, OTHER, G, DOWN):                                # a NULL view / table / gradient / output
        a = _bwd_ok(csr, f); a[pos] = None
        assert call(a) == EINVAL, pos
    for hid in (0, -4):
        a = _bwd_ok(csr, f); a[BHID] = hid
        assert call(a) == EINVAL
    for pos in (LDOWN, LDOTHER, LDG, LDD):                                 # a row stride smaller than hidden
        a = _bwd_ok(csr, f); a[pos] = 7
        assert call(a) == EINVAL, pos
    # the csr checks of entry_args.hpp
    for bad in (_lib.Csr(2, 2, 2, None, _keep.ctypes.data, None, None),           # no indptr
                _lib.Csr(-1, 2, 2, _keep.ctypes.data, _keep.ctypes.data, None, None),
                _lib.Csr(2, -1, 2, _keep.ctypes.data, _keep.ctypes.data, None, None),
                _lib.Csr(2, 2, -1, _keep.ctypes.data, _keep.ctypes.data, None, None),
                _lib.Csr(2, 2, 1 << 31, _keep.ctypes.data, _keep.ctypes.data, None, None),
                _lib.Csr(2, 2, 2, _keep.ctypes.data, None, None, None)):          # edges without indices
        a = _bwd_ok(csr, f); a[VIEW] = C.byref(bad)
        assert call(a) == EINVAL
    # the plan checks
    plan = _lib.Plan(64, 2, 1, 2, None, None, None, None, None, 0, 0, 0, None)
    a = _bwd_ok(csr, f); a[PLAN] = C.byref(plan)                           # plan without units
    assert call(a) == EINVAL
    units = np.zeros((4, 4), np.int32)
    plan = _lib.Plan(64, 2, -1, 0, units.ctypes.data, None, None, None, None, 0, 0, 0, None)
    a = _bwd_ok(csr, f); a[PLAN] = C.byref(plan)                           # negative counts
    assert call(a) == EINVAL
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, None, None, f.value, 1 << 20, 0, 0, None)
    a = _bwd_ok(csr, f); a[PLAN] = C.byref(plan)                           # segments without long_seg_ptr
    assert call(a) == EINVAL
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, None, f.value, None, f.value, 1 << 20, 0, 0, None)
    a = _bwd_ok(csr, f); a[PLAN] = C.byref(plan)                           # ... without long_rows
    assert call(a) == EINVAL
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, None, 1 << 20, 0, 0, None)
    a = _bwd_ok(csr, f); a[PLAN] = C.byref(plan)                           # ... without a workspace
    assert call(a) == EINVAL
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, f.value, 2 * 8 * 4 - 1, 0, 0, None)
    a = _bwd_ok(csr, f); a[PLAN] = C.byref(plan)                           # workspace one byte short of 2 segments x 8
    assert call(a) == ENOMEM
    # an invalid argument is reported before the workspace
    a[BHID] = 0
    assert call(a) == EINVAL
    # no rows: nothing to do, whatever the pointers
    empty = _lib.Csr(0, 2, 0, _keep.ctypes.data, None, None, None)
    a = _bwd_ok(csr, f); a[VIEW] = C.byref(empty)
    for pos in (OWN, OTHER, G, DOWN):
        a[pos] = None
    assert call(a) == 0


def test_every_refusal_comes_before_the_launch():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "edge_embed.hip")).read()
    for entry, launch in (("stag_edge_embed_fwd(", "embed_fwd_launch("), ("stag_edge_embed_bwd(", "embed_bwd_launch(")):
        body = src[src.index('extern "C" int ' + entry):]
        body = body[:body.index("\n}\n") + 3]
        at = body.index(launch)
        assert "return STAG_E" not in body[at:].replace("STAG_EIO", "")
        assert "hipLaunchKernelGGL" not in body and "hipMemset" not in body    # the entry points themselves touch no device


def test_edge_embed_kernels_use_no_scratch():
    """The forward, backward and merge kernels of edge_embed.hip keep their state in registers: 0 scratch bytes in every one."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "edge_embed.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    for kernel in ("edge_embed_fwd_kernel", "edge_embed_bwd_kernel", "edge_embed_merge_kernel"):
        assert sum(kernel in n for n in names) == 5, kernel                # lanes per row: 64, 32, 16, 8, 4
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import ops
    monkeypatch.setattr(ops, "EDGE_EMBED_FUSED", True)
    why = ops.edge_embed_why_not
    graph = types.SimpleNamespace(_src=None)
    mods = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.SiLU())
    meta = torch.zeros(6, 16, device="meta")
    cpu = torch.zeros(6, 16)

    class _OnDevice:
        """A stand-in that passes the device clause (no device is present here)."""

        def __init__(self, t):
            self.t = t
            self.is_cuda = True

        def __getattr__(self, k):
            return getattr(self.t, k)

    p = _OnDevice(cpu)
    assert why(graph, p, p, mods) is None
    assert why(graph, cpu, cpu, mods) == "device" and why(graph, meta, meta, mods) == "device"
    assert why(graph, p, cpu, mods) == "device" and why(graph, cpu, p, mods) == "device"
    assert why(types.SimpleNamespace(), p, p, mods) == "device"               # a graph without COO arrays on the device
    assert why(types.SimpleNamespace(is_shard=True, _src=None), p, p, mods) == "shard"
    assert why(graph, _OnDevice(cpu[0]), p, mods) == "shape"
    assert why(graph, p, _OnDevice(torch.zeros(6, 8)), mods) == "shape"
    assert why(graph, _OnDevice(torch.zeros(6, 0)), _OnDevice(torch.zeros(6, 0)), mods) == "shape"
    assert why(graph, _OnDevice(torch.zeros(2, 6, 16)), _OnDevice(torch.zeros(2, 6, 16)), mods) == "shape"
    for dt in (torch.float64, torch.int32):
        assert why(graph, _OnDevice(cpu.to(dt)), p, mods) == "dtype"
        assert why(graph, p, _OnDevice(cpu.to(dt)), mods) == "dtype"
    for dt in (torch.float16, torch.bfloat16):                                 # cast by the autograd Function
        assert why(graph, _OnDevice(cpu.to(dt)), _OnDevice(cpu.to(dt)), mods) is None
    lin = mods[0]
    for other in (torch.nn.Sequential(lin, torch.nn.ReLU()), torch.nn.Sequential(lin, torch.nn.GELU()),
                  torch.nn.Sequential(lin), torch.nn.Sequential(lin, torch.nn.SiLU(), torch.nn.SiLU()),
                  torch.nn.Sequential(torch.nn.Identity(), torch.nn.SiLU()), []):
        assert why(graph, p, p, other) == "embedding"

    class MySiLU(torch.nn.SiLU):          # a subclass may compute anything: exactly SiLU only
        pass
    assert why(graph, p, p, torch.nn.Sequential(lin, MySiLU())) == "embedding"
    assert why(graph, p, p, list(mods)) is None
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(graph, p, p, mods) == "compiling"
    assert why(graph, cpu, p, mods) == "device"                                # (the earlier clauses come first)
    monkeypatch.undo()
    monkeypatch.setattr(ops, "EDGE_EMBED_FUSED", False)
    assert why(graph, p, p, mods) == "switch"
    assert why(types.SimpleNamespace(is_shard=True), cpu, cpu, []) == "switch"


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "edge_embed_time.py"), doraise=True)
