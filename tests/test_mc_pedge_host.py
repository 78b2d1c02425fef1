"""stag_agg_fwd_mc_pedge (Monte-Carlo samples of amortised [E, D] edge noise from one pass over the rows and the parameter
tables) on the host: ABI surface, every refusal before any device work, the compiler's resource report of the new
kernels, the routing predicate of ops.aggregate_mc, the model-level identity test, and the timing tool."""
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
MAX_K = 4              # kMcPEdgeMaxK (csrc/agg_mc_pedge.hpp): samples per pass 4, 2, 1


def test_header_declares_and_library_exports_the_entry():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    proto = re.search(r"int stag_agg_fwd_mc_pedge\s*\(([^;]*)\);", header)
    assert proto, "prototype"
    args = re.sub(r"\s+", " ", proto.group(1))
    assert args == ("const stag_csr* csr, const stag_plan* plan, const float* x, int64_t ldx, int32_t D, "
                    "const stag_noise_spec* spec, int32_t n_samples, int64_t offset_stride, int32_t reduce, "
                    "const float* src_scale, const float* dst_scale, float* out, int64_t ldo, "
                    "int64_t sample_stride, void* stream")
    assert hasattr(_lib.lib(), "stag_agg_fwd_mc_pedge")
    assert len(_lib.lib().stag_agg_fwd_mc_pedge.argtypes) == 15
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19
    para = header[:proto.start()].rsplit("/* ----", 1)[1]
    assert "bit for bit" in para and "STAG_ENOSYS" in para and "STAG_EINVAL" in para and "STAG_ENOMEM" in para
    assert "STAG_PARAM_PER_EDGE " in para and "[E, D]" in para


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, indptr.ctypes.data, None, indptr.ctypes.data)   # never dereferenced
    return _lib, _lib.lib(), indptr, csr, C.c_void_p(16)     # f: a non-null, 16-B aligned dummy "device pointer"


# argument positions of stag_agg_fwd_mc_pedge
CSR, PLAN, X, LDX, D_, SPEC, NS, OSTRIDE, REDUCE, SS, DS, OUT, LDO, SSTRIDE, STREAM = range(15)


def _ok(_lib, csr, f, spec):
    return [C.byref(csr), None, f, 8, 8, C.byref(spec), 3, 1, 0, None, None, f, 8, 16, None]


def _pedge(_lib, **kw):
    s = _lib.NoiseSpec()
    s.kind, s.param_mode, s.p0, s.p1 = _lib.NOISE_NORMAL, _lib.PARAM_PER_EDGE, 32, 32
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_entry_refuses_invalid_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _pedge(_lib)
    call = lambda a: lib.stag_agg_fwd_mc_pedge(*a)
    for pos in (CSR, X, SPEC, OUT):                                        # NULL csr / x / spec / out
        a = _ok(_lib, csr, f, spec); a[pos] = None
        assert call(a) == EINVAL, pos
    a = _ok(_lib, csr, f, _pedge(_lib, p0=None))                           # NULL p0 of a graph with edges
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _pedge(_lib, p1=None))                           # NULL p1 (a Normal has two parameters)
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _pedge(_lib, kind=_lib.NOISE_UNIFORM, p1=None))  # ... and so has a Uniform
    assert call(a) == EINVAL
    for d in (0, -4):                                                      # D <= 0
        a = _ok(_lib, csr, f, spec); a[D_] = d
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[D_] = 16; a[LDO] = 16; a[SSTRIDE] = 32  # 0 < ldx < D
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[LDO] = 7                                # ldo < D
    assert call(a) == EINVAL
    for n in (0, -1):                                                      # n_samples < 1
        a = _ok(_lib, csr, f, spec); a[NS] = n
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[OSTRIDE] = -1                           # offset_stride < 0
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[SSTRIDE] = 15                           # n_samples > 1: samples would overlap
    assert call(a) == EINVAL
    for kind in (_lib.NOISE_NONE, _lib.NOISE_EXPLICIT, 9, -1):             # kind NONE / EXPLICIT / unknown
        a = _ok(_lib, csr, f, _pedge(_lib, kind=kind))
        assert call(a) == EINVAL, kind
    for mode in (_lib.PARAM_SCALAR, _lib.PARAM_PER_CHANNEL, _lib.PARAM_PER_EDGE1, 7):   # any param_mode but PER_EDGE
        a = _ok(_lib, csr, f, _pedge(_lib, param_mode=mode))
        assert call(a) == EINVAL, mode
    for d in (1, 2):                                                       # a derivative
        a = _ok(_lib, csr, f, _pedge(_lib, deriv=d))
        assert call(a) == EINVAL
    for red in (2, -1):                                                    # unknown reduce
        a = _ok(_lib, csr, f, spec); a[REDUCE] = red
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _pedge(_lib, pos_base=-1))                       # counter bounds: positions
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _pedge(_lib, pos_base=(1 << 44) - 1))
    assert call(a) == EINVAL
    for cb in (-1, 1 << 20):                                               # ... chunks
        a = _ok(_lib, csr, f, _pedge(_lib, chunk_base=cb))
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _pedge(_lib, kind=_lib.NOISE_UNIFORM, p1_log=1)) # a log-scale is a Normal's
    assert call(a) == EINVAL
    plan = _lib.Plan(64, 2, 1, 2, None, None, None, None, None, 0, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # plan without units
    assert call(a) == EINVAL
    units = np.zeros((4, 4), np.int32)
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, None, None, f.value, 1 << 20, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # segments without long_seg_ptr
    assert call(a) == EINVAL


def test_entry_leaves_the_loop_its_cases_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _pedge(_lib)
    call = lambda a: lib.stag_agg_fwd_mc_pedge(*a)
    assert call(_ok(_lib, csr, f, _pedge(_lib, in_norm=1))) == ENOSYS      # in-norm
    a = _ok(_lib, csr, f, spec); a[LDX] = 0                                # a broadcast row
    assert call(a) == ENOSYS
    assert call(_ok(_lib, csr, f, _pedge(_lib, chunk_base=1))) == ENOSYS   # a channel shard's chunk offset
    assert call(_ok(_lib, csr, f, _pedge(_lib, kind=_lib.NOISE_BERNOULLI))) == ENOSYS   # per-edge probabilities
    assert call(_ok(_lib, csr, f, _pedge(_lib, pos_base=(1 << 32) - 1))) == ENOSYS      # across a 2^32 boundary
    units = np.zeros((4, 4), np.int32)
    need = lib.stag_plan_workspace_bytes(2, MAX_K * 8, 0)
    assert need >= 2 * MAX_K * 8 * 4
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, f.value, need - 1, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # workspace one byte short
    assert call(a) == ENOMEM
    a[NS] = 1                                                              # ... whatever the number of samples
    assert call(a) == ENOMEM
    # an invalid argument is reported before a case of the loop
    assert call(_ok(_lib, csr, f, _pedge(_lib, in_norm=1, deriv=1))) == EINVAL
    a = _ok(_lib, csr, f, _pedge(_lib, kind=_lib.NOISE_BERNOULLI)); a[NS] = 0
    assert call(a) == EINVAL
    assert call(_ok(_lib, csr, f, _pedge(_lib, in_norm=1, param_mode=_lib.PARAM_PER_EDGE1))) == EINVAL
    # no rows: nothing to do, whatever the pointers
    empty = _lib.Csr(0, 2, 0, _keep.ctypes.data, None, None, None)
    a = _ok(_lib, csr, f, spec); a[CSR] = C.byref(empty)
    assert call(a) == 0


def test_the_edge1_entry_still_refuses_per_edge_parameters():
    _lib, lib, _keep, csr, f = _fixture()
    assert lib.stag_agg_fwd_mc_edge(*_ok(_lib, csr, f, _pedge(_lib))) == EINVAL


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls that pass every check launch on dummy pointers: no device may be present")
def test_entry_takes_every_listed_form():
    """What the header lists as served is refused by no check (without a device the launch itself fails)."""
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_fwd_mc_pedge(*a)
    forms = [_pedge(_lib), _pedge(_lib, relu=1), _pedge(_lib, p1_log=1), _pedge(_lib, kind=_lib.NOISE_UNIFORM),
             _pedge(_lib, kind=_lib.NOISE_UNIFORM, relu=1), _pedge(_lib, pos_base=(1 << 32) - 2),
             _pedge(_lib, pos_base=(7 << 32) + 12345), _pedge(_lib, p0=36, p1=36)]       # (a 4-byte aligned table)
    for s in forms:
        for D, ld in ((8, 8), (7, 9), (1, 1), (260, 260), (2, 64)):
            for n in (1, 2, 4, 7):
                for red in (0, 1):
                    a = _ok(_lib, csr, f, s)
                    a[D_] = D; a[LDX] = a[LDO] = ld; a[REDUCE] = red; a[NS] = n; a[SSTRIDE] = 2 * ld; a[OSTRIDE] = 3
                    assert call(a) not in (EINVAL, ENOSYS, ENOMEM), (s.kind, D, n)
    a = _ok(_lib, csr, f, forms[0]); a[NS] = 1; a[SSTRIDE] = 0             # one sample: the stride is not read
    assert call(a) not in (EINVAL, ENOSYS, ENOMEM)
    a = _ok(_lib, csr, f, forms[0]); a[OSTRIDE] = 0                        # the same draw S times: allowed
    assert call(a) not in (EINVAL, ENOSYS, ENOMEM)
    units = np.zeros((4, 4), np.int32)
    need = lib.stag_plan_workspace_bytes(2, MAX_K * 8, 0)
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, f.value, need, 0, 0, None)
    a = _ok(_lib, csr, f, forms[0]); a[PLAN] = C.byref(plan)               # exactly enough; no counters
    assert call(a) not in (EINVAL, ENOSYS, ENOMEM)


def test_every_refusal_comes_before_the_launch():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "agg_mc_pedge.hip")).read()
    body = src[src.index('extern "C" int stag_agg_fwd_mc_pedge('):]
    launch = body.index("mc_pedge_launch(")
    assert "return STAG_E" not in body[launch:].replace("STAG_EIO", "")
    assert "hipLaunchKernelGGL" not in body and "hipMemset" not in body    # the entry point itself touches no device
    # ... and nothing between the first check and the first launch leaves with anything but a refusal or "no rows"
    assert body[:launch].count("return STAG_OK") == 1
    hpp = open(os.path.join(ROOT, "stag_amd", "csrc", "agg_mc_pedge.hpp")).read()
    assert int(re.search(r"kMcPEdgeMaxK = (\d+);", hpp).group(1)) == MAX_K


def test_mc_pedge_kernels_use_no_scratch():
    """The forward and merge kernels of agg_mc_pedge.hip keep every sample's sums, the rows and both parameter rows of a
    block in registers: 0 scratch bytes in every instantiation (the condition under which 4 samples ride in a pass)."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "agg_mc_pedge.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    passes = [k for k in (4, 2, 1) if k <= MAX_K]
    assert sum("agg_mc_pedge_fwd_kernel" in n for n in names) == 2 * len(passes) * 5   # kinds x samples per pass x lanes per row
    for k in passes:
        assert sum(re.search(rf"agg_mc_pedge_fwd_kernelILi\dELi{k}ELi\d+E", n) is not None for n in names) == 2 * 5, k
    assert sum("agg_mc_pedge_merge_kernel" in n for n in names) == 5
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]
    # a unit of its own: the [E, 1] unit's report names none of these kernels
    other = open(os.path.join(csrc, "_obj", "agg_mc_edge.remarks")).read()
    assert "agg_mc_pedge" not in other


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
    monkeypatch.setattr(ops, "MC_PEDGE_FUSED", True)
    why = ops.mc_pedge_why_not
    graph = types.SimpleNamespace(number_of_edges=lambda: 5)
    x = torch.zeros(6, 16)
    # a CPU tensor passes every clause but the device's (checked last, so that the others can be seen here)
    for n in (_noise(), _noise(kind=_lib.NOISE_UNIFORM, p1_log=False), _noise(n_samples=4),
              _noise(grad_params=(torch.zeros(5, 16, requires_grad=True),) * 2)):
        assert why(x, n, graph) == "device"
    assert why(x[0], _noise(), graph) == "shape"
    assert why(x[:1].expand(6, 16), _noise(), graph) == "broadcast row"
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        assert why(x.to(dt), _noise(), graph) == "dtype"
    assert why(x, torch.zeros(5, 16), graph) == "no descriptor"
    assert why(x, None, graph) == "no descriptor"
    for mode in (_lib.PARAM_SCALAR, _lib.PARAM_PER_CHANNEL, _lib.PARAM_PER_EDGE1):
        assert why(x, _noise(param_mode=mode), graph) == "noise parameters"
    for dn in (1, 4, 32):
        assert why(x, _noise(dn=dn), graph) == "noise width"
    assert why(x, _noise(in_norm=True), graph) == "in-norm"
    for kind in (_lib.NOISE_BERNOULLI, _lib.NOISE_EXPLICIT, _lib.NOISE_NONE):
        assert why(x, _noise(kind=kind), graph) == "kind"
    assert why(x, _noise(deriv=1), graph) == "derivative selector"
    assert why(x, _noise(chunk_base=2), graph) == "channel shard"
    assert why(x, _noise(pos_base=(1 << 32) - 4), graph) == "position range"
    assert why(x, _noise(pos_base=(1 << 32) - 5), graph) == "device"
    assert why(x, _noise(pos_base=3 << 32), graph) == "device"
    shard = types.SimpleNamespace(is_shard=True, number_of_edges=lambda: 5)
    assert why(x, _noise(), shard) == "shard"
    assert why(x, _noise(graph=shard), graph) == "shard"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(x, _noise(), graph) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "MC_PEDGE_FUSED", False)
    assert why(x, _noise(), graph) == "switch"
    monkeypatch.setattr(ops, "MC_PEDGE_FUSED", True)
    assert why(torch.zeros(6, 16, device="meta"), _noise(), graph) == "device"
    # the [E, 1] predicate keeps its answer for [E, D] parameters
    assert ops.mc_edge_why_not(x, _noise(), graph) in ("noise parameters", "switch")


def test_the_switch_and_the_raw_binding_exist():
    from stag_amd import ops
    assert isinstance(ops.MC_PEDGE_FUSED, bool)
    assert callable(ops._agg_fwd_mc_pedge_raw) and issubclass(ops._AggregateMCPEdge, torch.autograd.Function)


def test_which_leading_layers_are_the_identity():
    """What StagModel._mc_plan looks behind: Identity, a Dropout that is off, a Sequential of only such modules."""
    from stag_amd import models
    ident = models._is_identity
    nn = torch.nn
    assert ident(nn.Identity())
    assert ident(nn.Dropout(0.5).eval()) and not ident(nn.Dropout(0.5).train())
    assert ident(nn.Dropout(0.0).train())
    assert ident(nn.Sequential(nn.Identity(), nn.Dropout(0.3)).eval())
    assert not ident(nn.Sequential(nn.Identity(), nn.Dropout(0.3)).train())
    assert not ident(nn.Sequential(nn.Dropout(0.3), nn.ReLU()).eval())
    assert not ident(nn.Linear(3, 3).eval()) and not ident(nn.ReLU())


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "mc_pedge_time.py"), doraise=True)
