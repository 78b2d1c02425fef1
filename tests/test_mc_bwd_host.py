"""stag_agg_bwd_w_mc (the per-edge parameter gradients of a Monte-Carlo batch from one pass) on the host: ABI surface, every
refusal before any device work, the compiler's resource report of the new kernels, the routing predicate of the two
autograd nodes of ops.aggregate_mc, and the timing tool."""
import ctypes as C
import os
import py_compile
import re
import subprocess
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ENOSYS = -22, -12, -38
MAX_K = 4              # kBwdWMcMaxK (csrc/agg_bwd_w_mc.hpp): samples per pass 4, 2, 1


def test_header_declares_and_library_exports_the_entry():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    proto = re.search(r"int stag_agg_bwd_w_mc\s*\(([^;]*)\);", header)
    assert proto, "prototype"
    args = re.sub(r"\s+", " ", proto.group(1))
    assert args == ("const stag_csr* csr, const stag_plan* plan, const float* x, int64_t ldx, const float* g, "
                    "int64_t ldg, int64_t g_sample_stride, int32_t D, const float* src_scale, const float* g_scale, "
                    "const stag_noise_spec* spec, int32_t n_samples, int64_t offset_stride, int32_t reduce_k, "
                    "float* dw0, float* dw1, int64_t ldw, void* stream")
    assert hasattr(_lib.lib(), "stag_agg_bwd_w_mc")
    assert len(_lib.lib().stag_agg_bwd_w_mc.argtypes) == 18
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19
    para = header[:proto.start()].rsplit("/* ----", 1)[1]
    assert "bit for bit" in para and "STAG_ENOSYS" in para and "STAG_EINVAL" in para and "No atomics" in para
    assert "STAG_PARAM_PER_EDGE " in para and "STAG_PARAM_PER_EDGE1" in para and "sample 0's term" in para


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, indptr.ctypes.data, None, indptr.ctypes.data)   # never dereferenced
    return _lib, _lib.lib(), indptr, csr, C.c_void_p(16)     # f: a non-null, 16-B aligned dummy "device pointer"


# argument positions of stag_agg_bwd_w_mc
CSR, PLAN, X, LDX, G, LDG, GSTRIDE, D_, SS, GS, SPEC, NS, OSTRIDE, RK, DW0, DW1, LDW, STREAM = range(18)


def _ok(_lib, csr, f, spec):
    """[E, D] parameters: D = 8, three samples, both gradient tables"""
    return [C.byref(csr), None, f, 8, f, 8, 16, 8, None, None, C.byref(spec), 3, 1, 0, f, f, 8, None]


def _ok1(_lib, csr, f, spec):
    """[E, 1] parameters: the sum over k as well"""
    a = _ok(_lib, csr, f, spec)
    a[RK], a[LDW] = 1, 1
    return a


def _pedge(_lib, **kw):
    s = _lib.NoiseSpec()
    s.kind, s.param_mode, s.p0, s.p1 = _lib.NOISE_NORMAL, _lib.PARAM_PER_EDGE, 32, 32
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _pedge1(_lib, **kw):
    return _pedge(_lib, **{"param_mode": _lib.PARAM_PER_EDGE1, **kw})


def test_entry_refuses_invalid_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_bwd_w_mc(*a)
    for ok, mk in ((_ok, _pedge), (_ok1, _pedge1)):
        spec = mk(_lib)
        for pos in (CSR, X, G, SPEC, DW0):                                     # NULL csr / x / g / spec / dw0
            a = ok(_lib, csr, f, spec); a[pos] = None
            assert call(a) == EINVAL, pos
        assert call(ok(_lib, csr, f, mk(_lib, p0=None))) == EINVAL             # NULL p0 of a graph with edges
        assert call(ok(_lib, csr, f, mk(_lib, p1=None))) == EINVAL             # NULL p1 (a Normal has two parameters)
        assert call(ok(_lib, csr, f, mk(_lib, kind=_lib.NOISE_UNIFORM, p1=None))) == EINVAL
        for d in (0, -4):                                                      # D <= 0
            a = ok(_lib, csr, f, spec); a[D_] = d
            assert call(a) == EINVAL
        a = ok(_lib, csr, f, spec); a[D_] = 16; a[LDG] = 16; a[GSTRIDE] = 32; a[LDW] = 16   # 0 < ldx < D
        assert call(a) == EINVAL
        a = ok(_lib, csr, f, spec); a[LDG] = 7                                 # ldg < D
        assert call(a) == EINVAL
        a = ok(_lib, csr, f, spec); a[LDW] = 0 if a[RK] else 7                 # ldw < (reduce_k ? 1 : D)
        assert call(a) == EINVAL
        for n in (0, -1):                                                      # n_samples < 1
            a = ok(_lib, csr, f, spec); a[NS] = n
            assert call(a) == EINVAL
        a = ok(_lib, csr, f, spec); a[OSTRIDE] = -1                            # offset_stride < 0
        assert call(a) == EINVAL
        a = ok(_lib, csr, f, spec); a[GSTRIDE] = 15                            # n_samples > 1: the samples' rows would overlap
        assert call(a) == EINVAL
        for kind in (_lib.NOISE_NONE, _lib.NOISE_EXPLICIT, _lib.NOISE_BERNOULLI, 9, -1):   # no reparameterised draw
            assert call(ok(_lib, csr, f, mk(_lib, kind=kind))) == EINVAL, kind
        for mode in (_lib.PARAM_SCALAR, _lib.PARAM_PER_CHANNEL, 7):            # stag_agg_bwd_dp's, unknown
            assert call(ok(_lib, csr, f, mk(_lib, param_mode=mode))) == EINVAL, mode
        for d in (1, 2):                                                       # a derivative selector
            assert call(ok(_lib, csr, f, mk(_lib, deriv=d))) == EINVAL
        assert call(ok(_lib, csr, f, mk(_lib, pos_base=-1))) == EINVAL         # counter bounds: positions
        assert call(ok(_lib, csr, f, mk(_lib, pos_base=(1 << 44) - 1))) == EINVAL
        for cb in (-1, 1 << 20):                                               # ... chunks
            assert call(ok(_lib, csr, f, mk(_lib, chunk_base=cb))) == EINVAL
        assert call(ok(_lib, csr, f, mk(_lib, kind=_lib.NOISE_UNIFORM, p1_log=1))) == EINVAL   # a log-scale is a Normal's
        plan = _lib.Plan(64, 2, 1, 2, None, None, None, None, None, 0, 0, 0, None)
        a = ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                    # a plan without units
        assert call(a) == EINVAL
    # the parameter mode goes with reduce_k
    assert call(_ok1(_lib, csr, f, _pedge(_lib))) == EINVAL                    # PER_EDGE with reduce_k
    assert call(_ok(_lib, csr, f, _pedge1(_lib))) == EINVAL                    # PER_EDGE1 without it


def test_entry_leaves_the_loop_its_cases_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_bwd_w_mc(*a)
    for ok, mk in ((_ok, _pedge), (_ok1, _pedge1)):
        spec = mk(_lib)
        assert call(ok(_lib, csr, f, mk(_lib, in_norm=1))) == ENOSYS           # in-norm
        a = ok(_lib, csr, f, spec); a[LDX] = 0                                 # a broadcast row
        assert call(a) == ENOSYS
        assert call(ok(_lib, csr, f, mk(_lib, chunk_base=1))) == ENOSYS        # a channel shard's chunk offset
        assert call(ok(_lib, csr, f, mk(_lib, pos_base=(1 << 32) - 1))) == ENOSYS   # across a 2^32 boundary
        a = ok(_lib, csr, f, spec); a[LDX] = 1 << 30                           # ldx * 4 >= 2^32
        assert call(a) == ENOSYS
        a = ok(_lib, csr, f, spec); a[LDG] = 1 << 30; a[GSTRIDE] = 1 << 32     # ldg * 4 >= 2^32
        assert call(a) == ENOSYS
        # an invalid argument is reported before a case of the loop
        assert call(ok(_lib, csr, f, mk(_lib, in_norm=1, deriv=1))) == EINVAL
        a = ok(_lib, csr, f, mk(_lib, chunk_base=1)); a[NS] = 0
        assert call(a) == EINVAL
        a = ok(_lib, csr, f, mk(_lib, in_norm=1)); a[LDX] = 0; a[DW0] = None
        assert call(a) == EINVAL
        # no rows, or no edges: nothing to do after the checks, whatever the pointers
        for empty in (_lib.Csr(0, 2, 0, _keep.ctypes.data, None, None, None),
                      _lib.Csr(2, 2, 0, _keep.ctypes.data, None, None, None)):
            a = ok(_lib, csr, f, mk(_lib, p0=None, p1=None)); a[CSR] = C.byref(empty)
            assert call(a) == 0
            a[NS] = 0                                                          # ... but after them
            assert call(a) == EINVAL


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls that pass every check launch on dummy pointers: no device may be present")
def test_entry_takes_every_listed_form():
    """What the header lists as served is refused by no check (without a device the launch itself fails)."""
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_bwd_w_mc(*a)
    for ok, mk in ((_ok, _pedge), (_ok1, _pedge1)):
        forms = [mk(_lib), mk(_lib, relu=1), mk(_lib, p1_log=1), mk(_lib, kind=_lib.NOISE_UNIFORM),
                 mk(_lib, kind=_lib.NOISE_UNIFORM, relu=1), mk(_lib, pos_base=(1 << 32) - 2),
                 mk(_lib, pos_base=(7 << 32) + 12345), mk(_lib, p0=36, p1=36)]           # (a 4-byte aligned table)
        for s in forms:
            for D, ld in ((8, 8), (7, 9), (1, 1), (260, 260), (2, 64)):
                for n in (1, 2, 4, 7):
                    a = ok(_lib, csr, f, s)
                    a[D_] = D; a[LDX] = a[LDG] = ld; a[NS] = n; a[GSTRIDE] = 2 * ld; a[OSTRIDE] = 3
                    a[LDW] = 1 if a[RK] else ld
                    assert call(a) not in (EINVAL, ENOSYS, ENOMEM), (s.kind, D, n)
        a = ok(_lib, csr, f, forms[0]); a[NS] = 1; a[GSTRIDE] = 0              # one sample: the stride is not read
        assert call(a) not in (EINVAL, ENOSYS, ENOMEM)
        a = ok(_lib, csr, f, forms[0]); a[OSTRIDE] = 0                         # the same draw S times: allowed
        assert call(a) not in (EINVAL, ENOSYS, ENOMEM)
        a = ok(_lib, csr, f, forms[0]); a[DW1] = None                          # one gradient table
        assert call(a) not in (EINVAL, ENOSYS, ENOMEM)
        a = ok(_lib, csr, f, forms[0]); a[DW0] = C.c_void_p(20); a[X] = C.c_void_p(20)   # unaligned pointers
        assert call(a) not in (EINVAL, ENOSYS, ENOMEM)
        units = np.zeros((4, 4), np.int32)
        plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, None, None, None, 0, 0, 0, None)
        a = ok(_lib, csr, f, forms[0]); a[PLAN] = C.byref(plan)                # no workspace, no counters
        assert call(a) not in (EINVAL, ENOSYS, ENOMEM)


def test_every_refusal_comes_before_the_launch():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "agg_bwd_w_mc.hip")).read()
    body = src[src.index('extern "C" int stag_agg_bwd_w_mc('):]
    launch = body.index("bwd_w_mc_launch(")
    assert "return STAG_E" not in body[launch:].replace("STAG_EIO", "")
    assert body[:launch].count("return STAG_E") >= 8 and "return STAG_ENOSYS" in body[:launch]
    assert "hipLaunchKernelGGL" not in body and "hipMemset" not in body    # the entry point itself touches no device
    # ... and nothing between the first check and the first launch leaves with anything but a refusal or "nothing to do"
    assert body[:launch].count("return STAG_OK") == 1
    assert "atomic" not in src.replace("No atomics", "")
    hpp = open(os.path.join(ROOT, "stag_amd", "csrc", "agg_bwd_w_mc.hpp")).read()
    assert int(re.search(r"kBwdWMcMaxK = (\d+);", hpp).group(1)) == MAX_K


def test_mc_bwd_kernels_use_no_scratch():
    """Every instantiation keeps the K gradient rows of a pass, the rows and parameter rows of two edges and both running
    sums in registers: 0 scratch bytes (the condition under which 4 samples ride in a pass)."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "agg_bwd_w_mc.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    passes = [k for k in (4, 2, 1) if k <= MAX_K]
    assert len(names) == 2 * len(passes) * 7 and all("agg_bwd_w_mc_kernel" in n for n in names)   # kinds x samples per pass x lanes per unit
    for k in passes:
        assert sum(re.search(rf"agg_bwd_w_mc_kernelILi\dELi{k}ELi\d+E", n) is not None for n in names) == 2 * 7, k
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]
    # a unit of its own: no other unit's report names these kernels
    obj = os.path.join(csrc, "_obj")
    others = [f for f in os.listdir(obj) if f.endswith(".remarks") and f != "agg_bwd_w_mc.remarks"]
    assert len(others) >= 20
    for f in others:
        assert "agg_bwd_w_mc" not in open(os.path.join(obj, f)).read(), f


def _noise(**kw):
    from stag_amd import _lib, ops
    graph = types.SimpleNamespace(number_of_edges=lambda: 5)
    d = dict(dn=16, kind=_lib.NOISE_NORMAL, param_mode=_lib.PARAM_PER_EDGE, in_norm=False, p1_log=True, deriv=0,
             n_samples=1, grad_params=None, chunk_base=0, pos_base=0, graph=graph)
    d.update(kw)
    n = ops.EdgeNoise.__new__(ops.EdgeNoise)
    n.__dict__.update(d)
    return n


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import _lib, ops
    monkeypatch.setattr(ops, "MC_BWD_FUSED", True)
    why = ops.mc_bwd_why_not
    graph = types.SimpleNamespace(number_of_edges=lambda: 5)
    x = torch.zeros(6, 16)
    E1 = _lib.PARAM_PER_EDGE1
    # a CPU tensor passes every clause but the device's (checked last, so that the others can be seen here)
    for n in (_noise(), _noise(kind=_lib.NOISE_UNIFORM, p1_log=False), _noise(n_samples=4), _noise(param_mode=E1),
              _noise(grad_params=(torch.zeros(5, 16, requires_grad=True),) * 2)):
        assert why(x, n, graph, False) == "device"
    assert why(x[0], _noise(), graph, False) == "shape"
    assert why(x[:1].expand(6, 16), _noise(), graph, False) == "broadcast row"
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        assert why(x.to(dt), _noise(), graph, False) == "dtype"
    assert why(x, torch.zeros(5, 16), graph, False) == "no descriptor"
    assert why(x, None, graph, False) == "no descriptor"
    for mode in (_lib.PARAM_SCALAR, _lib.PARAM_PER_CHANNEL):
        assert why(x, _noise(param_mode=mode), graph, False) == "noise parameters"
    for dn in (1, 4, 32):
        assert why(x, _noise(dn=dn), graph, False) == "noise width"
    assert why(x, _noise(in_norm=True), graph, False) == "in-norm"
    for kind in (_lib.NOISE_BERNOULLI, _lib.NOISE_EXPLICIT, _lib.NOISE_NONE):
        assert why(x, _noise(kind=kind), graph, False) == "kind"
    assert why(x, _noise(deriv=1), graph, False) == "derivative selector"
    assert why(x, _noise(chunk_base=2), graph, False) == "channel shard"
    assert why(x, _noise(pos_base=(1 << 32) - 4), graph, False) == "position range"
    assert why(x, _noise(pos_base=(1 << 32) - 5), graph, False) == "device"
    assert why(x, _noise(pos_base=3 << 32), graph, False) == "device"
    shard = types.SimpleNamespace(is_shard=True, number_of_edges=lambda: 5)
    assert why(x, _noise(), shard, False) == "shard"
    assert why(x, _noise(graph=shard), graph, False) == "shard"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(x, _noise(), graph, False) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "MC_BWD_FUSED", False)
    assert why(x, _noise(), graph, False) == "switch" and why(x, _noise(param_mode=E1), graph, True) == "switch"
    monkeypatch.setattr(ops, "MC_BWD_FUSED", True)
    assert why(torch.zeros(6, 16, device="meta"), _noise(), graph, False) == "device"


def test_the_two_routing_rules(monkeypatch):
    """[E, D] heads: the batched call whether or not x needs a gradient.  [E, 1] heads: the batched call when x needs none,
    or past one channel tile (D > 256); with dx at D <= 256 stag_agg_bwd_edge keeps its one gather per sample."""
    from stag_amd import _lib, ops
    monkeypatch.setattr(ops, "MC_BWD_FUSED", True)
    why = ops.mc_bwd_why_not
    graph = types.SimpleNamespace(number_of_edges=lambda: 5)
    passes = "device"       # (a CPU tensor: every other clause was passed)
    for D in (16, 256, 257, 300):
        x = torch.zeros(6, D)
        for need_x in (False, True):
            assert why(x, _noise(dn=D), graph, need_x) == passes, (D, need_x)
        e1 = _noise(dn=D, param_mode=_lib.PARAM_PER_EDGE1)
        assert why(x, e1, graph, False) == passes
        assert why(x, e1, graph, True) == ("one gather" if D <= 256 else passes), D


def test_the_switch_and_the_raw_binding_exist():
    from stag_amd import ops
    assert isinstance(ops.MC_BWD_FUSED, bool)
    assert callable(ops._bwd_w_mc_raw) and callable(ops.mc_bwd_why_not)


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "mc_bwd_time.py"), doraise=True)
