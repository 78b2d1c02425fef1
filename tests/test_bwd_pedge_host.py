"""stag_agg_bwd_pedge (dx and both [E, D] parameter gradients of one draw from one pass over the source-major CSR) on the
host: ABI surface, every refusal before any device work and in its order (invalid, then not served, then out of memory),
the compiler's resource report of the new kernels, the routing predicate of the two autograd nodes that take it, and the
timing tool."""
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


def test_header_declares_and_library_exports_the_entry():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    proto = re.search(r"int stag_agg_bwd_pedge\s*\(([^;]*)\);", header)
    assert proto, "prototype"
    args = re.sub(r"\s+", " ", proto.group(1))
    assert args == ("const stag_csr* csr_t, const stag_plan* plan_t, const float* g, int64_t ldg, int32_t D, "
                    "const stag_noise_spec* spec, const float* g_scale, const float* row_scale, "
                    "const float* x, int64_t ldx, float* dx, int64_t ldo, "
                    "float* dp0, float* dp1, int64_t ldp, void* stream")
    assert hasattr(_lib.lib(), "stag_agg_bwd_pedge")
    assert len(_lib.lib().stag_agg_bwd_pedge.argtypes) == 16
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19      # additive: no bump
    para = header[:proto.start()].rsplit("/* ----", 1)[1]
    for word in ("bit for bit", "STAG_ENOSYS", "STAG_EINVAL", "STAG_ENOMEM", "no atomics", "stag_agg_fwd_mc_pedge",
                 "stag_agg_bwd_w_mc", "dx may be NULL", "dp1 may be NULL"):
        assert word in para, word


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    p = indptr.ctypes.data
    csr = _lib.Csr(2, 2, 2, p, p, p, p)                       # never dereferenced
    return _lib, _lib.lib(), indptr, csr, C.c_void_p(16)     # f: a non-null, 16-B aligned dummy "device pointer"


# argument positions of stag_agg_bwd_pedge
CSR, PLAN, G, LDG, D_, SPEC, GS, RS, X, LDX, DX, LDO, DP0, DP1, LDP, STREAM = range(16)


def _ok(csr, f, spec):
    """D = 8, dx and both gradient tables, no plan"""
    return [C.byref(csr), None, f, 8, 8, C.byref(spec), None, None, f, 8, f, 8, f, f, 8, None]


def _pedge(_lib, **kw):
    s = _lib.NoiseSpec()
    s.kind, s.param_mode, s.p0, s.p1 = _lib.NOISE_NORMAL, _lib.PARAM_PER_EDGE, 32, 32
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _plan(_lib, f, unit_buf, **kw):
    """one long row of two segments: everything a merge reads is there, the workspace holds [2][8] floats"""
    d = dict(seg_len=1, n_units=3, n_long=1, n_seg=2, units=unit_buf.ctypes.data, long_rows=f.value, long_seg_ptr=f.value,
             workspace=f.value, workspace_bytes=2 * 8 * 4)
    d.update(kw)
    p = _lib.Plan()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def test_entry_refuses_invalid_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_bwd_pedge(*a)
    spec = _pedge(_lib)
    for pos in (CSR, G, SPEC, X, DP0):                                         # NULL csr_t / g / spec / x / dp0
        a = _ok(csr, f, spec); a[pos] = None
        assert call(a) == EINVAL, pos
    assert call(_ok(csr, f, _pedge(_lib, p0=None))) == EINVAL                  # NULL p0 of a graph with edges
    assert call(_ok(csr, f, _pedge(_lib, p1=None))) == EINVAL                  # NULL p1 (a Normal has two parameters)
    assert call(_ok(csr, f, _pedge(_lib, kind=_lib.NOISE_UNIFORM, p1=None))) == EINVAL
    p = _keep.ctypes.data
    for bad in (_lib.Csr(2, 2, 2, p, p, None, p), _lib.Csr(2, 2, 2, p, p, p, None)):   # NULL csr_t->eid / csr_t->nidx
        a = _ok(csr, f, spec); a[CSR] = C.byref(bad)
        assert call(a) == EINVAL
    for d in (0, -4):                                                          # D <= 0
        a = _ok(csr, f, spec); a[D_] = d
        assert call(a) == EINVAL
    a = _ok(csr, f, spec); a[LDG] = 7                                          # ldg < D
    assert call(a) == EINVAL
    for ldx in (7, 1, -1):                                                     # 0 < ldx < D (and a negative stride)
        a = _ok(csr, f, spec); a[LDX] = ldx
        assert call(a) == EINVAL
    a = _ok(csr, f, spec); a[LDO] = 7                                          # dx with ldo < D
    assert call(a) == EINVAL
    a = _ok(csr, f, spec); a[LDP] = 7                                          # ldp < D
    assert call(a) == EINVAL
    for kind in (_lib.NOISE_NONE, _lib.NOISE_EXPLICIT, _lib.NOISE_BERNOULLI, 9, -1):   # no reparameterised draw
        assert call(_ok(csr, f, _pedge(_lib, kind=kind))) == EINVAL, kind
    for mode in (_lib.PARAM_SCALAR, _lib.PARAM_PER_CHANNEL, _lib.PARAM_PER_EDGE1, 7):   # other entries', unknown
        assert call(_ok(csr, f, _pedge(_lib, param_mode=mode))) == EINVAL, mode
    for d in (1, 2):                                                           # a derivative selector
        assert call(_ok(csr, f, _pedge(_lib, deriv=d))) == EINVAL
    assert call(_ok(csr, f, _pedge(_lib, pos_base=-1))) == EINVAL              # counter bounds: positions
    assert call(_ok(csr, f, _pedge(_lib, pos_base=(1 << 44) - 1))) == EINVAL
    for cb in (-1, 1 << 20):                                                   # ... chunks
        assert call(_ok(csr, f, _pedge(_lib, chunk_base=cb))) == EINVAL
    assert call(_ok(csr, f, _pedge(_lib, kind=_lib.NOISE_UNIFORM, p1_log=1))) == EINVAL   # a log-scale is a Normal's
    units = np.zeros((4, 4), np.int32)
    a = _ok(csr, f, spec); a[PLAN] = C.byref(_plan(_lib, f, units, units=None))            # a plan without units
    assert call(a) == EINVAL
    for field in ("long_rows", "long_seg_ptr", "workspace"):                   # ... without what the merge of dx reads
        a = _ok(csr, f, spec); a[PLAN] = C.byref(_plan(_lib, f, units, **{field: None}))
        assert call(a) == EINVAL, field
    a = _ok(csr, f, spec); a[PLAN] = C.byref(_plan(_lib, f, units, n_seg=-1))
    assert call(a) == EINVAL


def test_entry_leaves_the_two_passes_their_cases_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_bwd_pedge(*a)
    spec = _pedge(_lib)
    assert call(_ok(csr, f, _pedge(_lib, in_norm=1))) == ENOSYS                # in-norm
    a = _ok(csr, f, spec); a[LDX] = 0                                          # a broadcast row
    assert call(a) == ENOSYS
    assert call(_ok(csr, f, _pedge(_lib, chunk_base=1))) == ENOSYS             # a channel shard's chunk offset
    assert call(_ok(csr, f, _pedge(_lib, pos_base=(1 << 32) - 1))) == ENOSYS   # across a 2^32 boundary
    a = _ok(csr, f, spec); a[LDX] = 1 << 30                                    # ldx * 4 >= 2^32
    assert call(a) == ENOSYS
    a = _ok(csr, f, spec); a[LDG] = 1 << 30                                    # ldg * 4 >= 2^32
    assert call(a) == ENOSYS
    # an invalid argument is reported before a case of the two passes
    assert call(_ok(csr, f, _pedge(_lib, in_norm=1, deriv=1))) == EINVAL
    a = _ok(csr, f, _pedge(_lib, chunk_base=1)); a[D_] = 0
    assert call(a) == EINVAL
    a = _ok(csr, f, _pedge(_lib, in_norm=1)); a[LDX] = 0; a[DP0] = None
    assert call(a) == EINVAL
    a = _ok(csr, f, _pedge(_lib, pos_base=(1 << 32) - 1)); a[LDP] = 7
    assert call(a) == EINVAL
    a = _ok(csr, f, _pedge(_lib, in_norm=1, p0=None))
    assert call(a) == EINVAL
    units = np.zeros((4, 4), np.int32)
    a = _ok(csr, f, spec); a[LDX] = 0; a[PLAN] = C.byref(_plan(_lib, f, units, long_rows=None))
    assert call(a) == EINVAL
    # a workspace that is too small, after both
    short = _plan(_lib, f, units, workspace_bytes=2 * 8 * 4 - 1)
    a = _ok(csr, f, spec); a[PLAN] = C.byref(short)
    assert call(a) == ENOMEM
    a = _ok(csr, f, _pedge(_lib, in_norm=1)); a[PLAN] = C.byref(short)
    assert call(a) == ENOSYS
    a = _ok(csr, f, spec); a[PLAN] = C.byref(short); a[LDG] = 7
    assert call(a) == EINVAL
    # no rows; or no edges and no dx: nothing to do after the checks, whatever the pointers
    for empty, dx in ((_lib.Csr(0, 2, 0, _keep.ctypes.data, None, None, None), f),
                      (_lib.Csr(0, 2, 0, _keep.ctypes.data, None, None, None), None),
                      (_lib.Csr(2, 2, 0, _keep.ctypes.data, None, None, None), None)):
        a = _ok(csr, f, _pedge(_lib, p0=None, p1=None)); a[CSR] = C.byref(empty); a[DX] = dx
        assert call(a) == 0
        a[D_] = 0                                                              # ... but after them
        assert call(a) == EINVAL


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls that pass every check launch on dummy pointers: no device may be present")
def test_entry_takes_every_listed_form():
    """What the header lists as served is refused by no check (without a device the launch itself fails)."""
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_bwd_pedge(*a)
    served = lambda a: call(a) not in (EINVAL, ENOSYS, ENOMEM)
    forms = [_pedge(_lib), _pedge(_lib, relu=1), _pedge(_lib, p1_log=1), _pedge(_lib, kind=_lib.NOISE_UNIFORM),
             _pedge(_lib, kind=_lib.NOISE_UNIFORM, relu=1), _pedge(_lib, pos_base=(1 << 32) - 2),
             _pedge(_lib, pos_base=(7 << 32) + 12345), _pedge(_lib, p0=36, p1=36)]      # (a 4-byte aligned table)
    for s in forms:
        for D, ld in ((8, 8), (7, 9), (1, 1), (260, 260), (2, 64)):
            a = _ok(csr, f, s)
            a[D_] = D; a[LDG] = a[LDX] = a[LDO] = a[LDP] = ld
            assert served(a), (s.kind, D)
    a = _ok(csr, f, forms[0]); a[DX] = None; a[LDO] = 0                        # parameter gradients only: ldo is not read
    assert served(a)
    a = _ok(csr, f, forms[0]); a[DP1] = None                                   # one gradient table
    assert served(a)
    a = _ok(csr, f, forms[0]); a[GS] = f; a[RS] = f                            # both scales
    assert served(a)
    a = _ok(csr, f, forms[0]); a[DP0] = C.c_void_p(20); a[X] = C.c_void_p(20); a[G] = C.c_void_p(20)   # unaligned pointers
    assert served(a)
    units = np.zeros((4, 4), np.int32)
    a = _ok(csr, f, forms[0]); a[PLAN] = C.byref(_plan(_lib, f, units))
    assert served(a)
    # without dx a plan needs neither the segment table of the merge nor a workspace
    bare = _plan(_lib, f, units, long_seg_ptr=None, workspace=None, workspace_bytes=0)
    a = _ok(csr, f, forms[0]); a[PLAN] = C.byref(bare); a[DX] = None
    assert served(a)
    # no edges, with dx: the walk writes the zero rows
    empty = _lib.Csr(2, 2, 0, _keep.ctypes.data, None, None, None)
    a = _ok(csr, f, _pedge(_lib, p0=None, p1=None)); a[CSR] = C.byref(empty)
    assert served(a)


def test_every_refusal_comes_before_the_launch():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "agg_bwd_pedge.hip")).read()
    body = src[src.index('extern "C" int stag_agg_bwd_pedge('):]
    launch = body.index("bwd_pedge_launch(")
    assert "return STAG_E" not in body[launch:].replace("STAG_EIO", "")
    assert body[:launch].count("return STAG_E") >= 8 and "return STAG_ENOSYS" in body[:launch] and "return STAG_ENOMEM" in body[:launch]
    assert body.index("return STAG_ENOSYS") < body.index("return STAG_ENOMEM")
    assert "hipLaunchKernelGGL" not in body and "hipMemset" not in body    # the entry point itself touches no device
    assert body[:launch].count("return STAG_OK") == 1
    assert "atomic" not in src.replace("No atomics", "")


def test_bwd_pedge_kernels_use_no_scratch():
    """Every instantiation keeps the parameter rows and gradient rows of a block of four edges, the unit's own row and the
    running dx sums in registers: 0 scratch bytes."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "agg_bwd_pedge.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    walk = [n for n in names if "agg_bwd_pedge_kernel" in n]
    merge = [n for n in names if "agg_bwd_pedge_merge_kernel" in n]
    assert len(walk) == 2 * 5 and len(merge) == 5 and len(names) == 15     # kinds x lanes per unit; lanes per unit
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]
    # a unit of its own: no other unit's report names these kernels
    obj = os.path.join(csrc, "_obj")
    others = [f for f in os.listdir(obj) if f.endswith(".remarks") and f != "agg_bwd_pedge.remarks"]
    assert len(others) >= 20
    for f in others:
        assert "agg_bwd_pedge" not in open(os.path.join(obj, f)).read(), f


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
    monkeypatch.setattr(ops, "PEDGE_BWD_FUSED", True)
    why = ops.pedge_bwd_why_not
    graph = types.SimpleNamespace(number_of_edges=lambda: 5)
    x = torch.zeros(6, 16)
    # a CPU tensor passes every clause but the device's (checked last, so that the others can be seen here)
    for n in (_noise(), _noise(kind=_lib.NOISE_UNIFORM, p1_log=False), _noise(n_samples=4),
              _noise(grad_params=(torch.zeros(5, 16, requires_grad=True),) * 2)):
        assert why(x, n, graph, True) == "device"
    assert why(x[0], _noise(), graph, True) == "shape"
    assert why(x[:1].expand(6, 16), _noise(), graph, True) == "broadcast row"
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        assert why(x.to(dt), _noise(), graph, True) == "dtype"
    assert why(x, torch.zeros(5, 16), graph, True) == "no descriptor"
    assert why(x, None, graph, True) == "no descriptor"
    for mode in (_lib.PARAM_SCALAR, _lib.PARAM_PER_CHANNEL, _lib.PARAM_PER_EDGE1):
        assert why(x, _noise(param_mode=mode), graph, True) == "noise parameters"
    for dn in (1, 4, 32):
        assert why(x, _noise(dn=dn), graph, True) == "noise width"
    assert why(x, _noise(in_norm=True), graph, True) == "in-norm"
    for kind in (_lib.NOISE_BERNOULLI, _lib.NOISE_EXPLICIT, _lib.NOISE_NONE):
        assert why(x, _noise(kind=kind), graph, True) == "kind"
    assert why(x, _noise(deriv=1), graph, True) == "derivative selector"
    assert why(x, _noise(chunk_base=2), graph, True) == "channel shard"
    assert why(x, _noise(pos_base=(1 << 32) - 4), graph, True) == "position range"
    assert why(x, _noise(pos_base=(1 << 32) - 5), graph, True) == "device"
    assert why(x, _noise(pos_base=3 << 32), graph, True) == "device"
    shard = types.SimpleNamespace(is_shard=True, number_of_edges=lambda: 5)
    assert why(x, _noise(), shard, True) == "shard"
    assert why(x, _noise(graph=shard), graph, True) == "shard"
    # x without a gradient: stag_agg_bwd_w alone is one pass already
    assert why(x, _noise(), graph, False) == "no dx"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(x, _noise(), graph, True) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "PEDGE_BWD_FUSED", False)
    assert why(x, _noise(), graph, True) == "switch" and why(x, _noise(), graph, False) == "switch"
    monkeypatch.setattr(ops, "PEDGE_BWD_FUSED", True)
    assert why(torch.zeros(6, 16, device="meta"), _noise(), graph, True) == "device"
    for D in (1, 7, 256, 257, 1433):                                           # any width
        assert why(torch.zeros(6, D), _noise(dn=D), graph, True) == "device"


def test_the_switch_and_the_raw_binding_exist():
    from stag_amd import ops
    assert isinstance(ops.PEDGE_BWD_FUSED, bool) and isinstance(ops.PEDGE_BWD_MC_LOOP, bool)
    assert callable(ops._agg_bwd_pedge_raw) and callable(ops.pedge_bwd_why_not)


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "pedge_bwd_time.py"), doraise=True)
