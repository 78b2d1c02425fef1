"""stag_agg_fwd_half (fp16 / bf16 feature rows) on the host: ABI surface, every refusal before any device work, the
compiler's resource report of the new kernels, the routing predicate of ops.aggregate, and the timing tool."""
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


def test_header_declares_and_library_exports_the_half_entry():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    assert re.search(r"\bstag_agg_fwd_half\s*\(", header)
    assert hasattr(_lib.lib(), "stag_agg_fwd_half")
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19
    assert re.search(r"#define STAG_DTYPE_F16 1\b", header) and re.search(r"#define STAG_DTYPE_BF16 2\b", header)
    assert (_lib.DTYPE_F16, _lib.DTYPE_BF16) == (1, 2)


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, indptr.ctypes.data, None, indptr.ctypes.data)   # never dereferenced
    return _lib, _lib.lib(), indptr, csr, C.c_void_p(16)     # f: a non-null, 16-B aligned dummy "device pointer"


# argument positions of stag_agg_fwd_half
CSR, PLAN, X, DTYPE, LDX, D_, SPEC, REDUCE, SS, DS, OUT, LDO, STREAM = range(13)


def _ok(_lib, csr, f, spec):
    return [C.byref(csr), None, f, _lib.DTYPE_BF16, 8, 8, C.byref(spec), 0, None, None, f, 8, None]


def _sampled(_lib, **kw):
    s = _lib.NoiseSpec()
    s.kind = _lib.NOISE_NORMAL
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_half_entry_refuses_invalid_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _lib.NoiseSpec()
    call = lambda a: lib.stag_agg_fwd_half(*a)
    for pos in (CSR, X, SPEC, OUT):                                        # NULL csr / x / spec / out
        a = _ok(_lib, csr, f, spec); a[pos] = None
        assert call(a) == EINVAL, pos
    for d in (0, -8):                                                      # D <= 0
        a = _ok(_lib, csr, f, spec); a[D_] = d
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[D_] = 16; a[LDO] = 16                  # 0 < ldx < D
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[LDO] = 7                                # ldo < D
    assert call(a) == EINVAL
    for dt in (0, 3, -1):                                                  # unknown dtype
        a = _ok(_lib, csr, f, spec); a[DTYPE] = dt
        assert call(a) == EINVAL
    bad = _lib.NoiseSpec(); bad.kind = 9                                   # unknown kind
    a = _ok(_lib, csr, f, bad)
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[REDUCE] = 2                             # unknown reduce
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, deriv=1))                         # a derivative
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, pos_base=-1))                     # counter bounds: positions
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, pos_base=(1 << 44) - 1))
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, chunk_base=(1 << 20) - 1))        # ... chunks: D = 8 is two of them
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, param_mode=_lib.PARAM_PER_CHANNEL))   # a per-channel row that is not there
    assert call(a) == EINVAL
    plan = _lib.Plan(64, 2, 1, 2, None, None, None, None, None, 0, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # plan without units
    assert call(a) == EINVAL


def test_half_entry_leaves_the_cast_route_its_cases_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _lib.NoiseSpec()
    call = lambda a: lib.stag_agg_fwd_half(*a)
    a = _ok(_lib, csr, f, spec); a[D_] = 4                                 # D % 8
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, spec); a[D_] = 12; a[LDX] = a[LDO] = 16
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, spec); a[LDX] = 12                               # ldx % 8
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, spec); a[X] = C.c_void_p(24)                     # x not 16-byte aligned
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, spec); a[LDX] = 0                                # a broadcast row
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, _sampled(_lib, in_norm=1))                       # in-norm
    assert call(a) == ENOSYS
    ex = _lib.NoiseSpec(); ex.kind = _lib.NOISE_EXPLICIT; ex.p0 = 32       # explicit weights
    a = _ok(_lib, csr, f, ex)
    assert call(a) == ENOSYS
    for mode in (_lib.PARAM_PER_EDGE1, _lib.PARAM_PER_EDGE):               # per-edge parameters
        a = _ok(_lib, csr, f, _sampled(_lib, param_mode=mode, p0=32, p1=32))
        assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, _sampled(_lib, p1_log=1))                        # a log-scale
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, _sampled(_lib, pos_base=(1 << 32) - 1))          # across a 2^32 boundary of the position
    assert call(a) == ENOSYS
    units = np.zeros((4, 4), np.int32)
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, f.value, 2 * 8 * 4 - 1, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # workspace one byte short of 2 segments x 8
    assert call(a) == ENOMEM


def test_half_kernels_use_no_scratch():
    """The forward and merge kernels of agg_half.hip keep their state in registers: 0 scratch bytes in every one."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "agg_half.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    assert sum("agg_half_fwd_kernel" in n for n in names) == 4 * 2 * 4     # kinds x dtypes x lanes per row
    assert sum("agg_half_merge_kernel" in n for n in names) == 4
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import _lib, ops
    monkeypatch.setattr(ops, "HALF_ROWS", True)
    why = ops.half_rows_why_not

    def noise(**kw):
        d = dict(kind=_lib.NOISE_NORMAL, param_mode=_lib.PARAM_SCALAR, in_norm=False, p1_log=False, deriv=0, n_samples=1,
                 grad_params=None, graph=types.SimpleNamespace())
        d.update(kw)
        return types.SimpleNamespace(**d)

    x = torch.zeros(6, 16, dtype=torch.bfloat16)
    # a CPU tensor passes every clause but the device's (checked last, so that the others can be seen here)
    for t in (x, x.half()):
        assert why(t, None, None, False) == "device" and why(t, None, noise(), False) == "device"
        assert not ops.half_rows_ok(t, None, noise(), False)
    assert why(x.float(), None, None, False) == "dtype"
    assert why(x, None, None, True) == "broadcast row"
    assert why(x, torch.zeros(3, 16), None, False) == "explicit weights"
    assert why(torch.zeros(6, 50, dtype=torch.bfloat16), None, None, False) == "width"
    assert why(torch.zeros(6, 4, dtype=torch.float16), None, None, False) == "width"
    big = torch.zeros(6, 40, dtype=torch.bfloat16)
    assert why(big[:, 8:24], None, None, False) == "device"                # row stride 40: a multiple of 8
    assert why(torch.zeros(6, 36, dtype=torch.bfloat16)[:, :16], None, None, False) == "strides"
    assert why(torch.zeros(16, 6, dtype=torch.bfloat16).t(), None, None, False) == "strides"
    assert why(x[:1].expand(6, 16), None, None, False) == "strides"
    assert why(x, None, noise(param_mode=_lib.PARAM_PER_CHANNEL), False) == "device"
    assert why(x, None, noise(kind=_lib.NOISE_BERNOULLI), False) == "device"
    assert why(x, None, noise(param_mode=_lib.PARAM_PER_EDGE1), False) == "noise parameters"
    assert why(x, None, noise(param_mode=_lib.PARAM_PER_EDGE), False) == "noise parameters"
    assert why(x, None, noise(in_norm=True), False) == "in-norm"
    assert why(x, None, noise(p1_log=True), False) == "log-scale"
    assert why(x, None, noise(n_samples=3), False) == "monte-carlo"
    p = torch.zeros((), requires_grad=True)
    assert why(x, None, noise(grad_params=(p, 1.0)), False) == "parameter gradients"
    assert why(x, None, noise(grad_params=(p.detach(), 1.0)), False) == "device"
    assert why(x, None, None, False, types.SimpleNamespace(is_shard=True)) == "shard"
    assert why(x, None, noise(graph=types.SimpleNamespace(is_shard=True)), False) == "shard"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(x, None, None, False) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "HALF_ROWS", False)
    assert why(x, None, None, False) == "switch"
    # a meta tensor is no device tensor either
    assert not ops.half_rows_ok(torch.zeros(6, 16, dtype=torch.bfloat16, device="meta"), None, None, False)


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "half_rows_time.py"), doraise=True)
