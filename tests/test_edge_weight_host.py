"""stag_agg_fwd_w1 (one weight per edge, shared by all channels) on the host: ABI surface, every refusal before any device
work, the compiler's resource report of the new kernels, the routing predicate of ops.aggregate, and the timing tool."""
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


def test_header_declares_and_library_exports_the_w1_entry():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    proto = re.search(r"int stag_agg_fwd_w1\s*\(([^;]*)\);", header)
    assert proto, "prototype"
    args = re.sub(r"\s+", " ", proto.group(1))
    assert args == ("const stag_csr* csr, const stag_plan* plan, const float* x, int64_t ldx, int32_t D, "
                    "const stag_noise_spec* spec, int32_t reduce, const float* src_scale, "
                    "const float* dst_scale, float* out, int64_t ldo, void* stream")
    assert hasattr(_lib.lib(), "stag_agg_fwd_w1")
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19
    para = header[:proto.start()].rsplit("/* ----", 1)[1]
    assert "IS NOT READ" in para and "STAG_ENOSYS" in para and "STAG_EINVAL" in para and "STAG_ENOMEM" in para


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, indptr.ctypes.data, None, indptr.ctypes.data)   # never dereferenced
    return _lib, _lib.lib(), indptr, csr, C.c_void_p(16)     # f: a non-null, 16-B aligned dummy "device pointer"


# argument positions of stag_agg_fwd_w1
CSR, PLAN, X, LDX, D_, SPEC, REDUCE, SS, DS, OUT, LDO, STREAM = range(12)


def _ok(_lib, csr, f, spec):
    return [C.byref(csr), None, f, 8, 8, C.byref(spec), 0, None, None, f, 8, None]


def _sampled(_lib, **kw):
    s = _lib.NoiseSpec()
    s.kind = _lib.NOISE_NORMAL
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _explicit(_lib, **kw):
    return _sampled(_lib, kind=_lib.NOISE_EXPLICIT, p0=32, **kw)


def test_w1_entry_refuses_invalid_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _sampled(_lib)
    call = lambda a: lib.stag_agg_fwd_w1(*a)
    for pos in (CSR, X, SPEC, OUT):                                        # NULL csr / x / spec / out
        a = _ok(_lib, csr, f, spec); a[pos] = None
        assert call(a) == EINVAL, pos
    for d in (0, -4):                                                      # D <= 0
        a = _ok(_lib, csr, f, spec); a[D_] = d
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[D_] = 16; a[LDO] = 16                  # 0 < ldx < D
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, spec); a[LDO] = 7                                # ldo < D
    assert call(a) == EINVAL
    for kind in (9, -1):                                                   # unknown kind
        a = _ok(_lib, csr, f, _sampled(_lib, kind=kind))
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, kind=_lib.NOISE_NONE))            # NONE is stag_agg_fwd's
    assert call(a) == EINVAL
    for red in (2, -1):                                                    # unknown reduce
        a = _ok(_lib, csr, f, spec); a[REDUCE] = red
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, param_mode=_lib.PARAM_PER_EDGE, p0=32, p1=32))   # [E, Dn] parameters
    assert call(a) == EINVAL
    for d in (1, 2):                                                       # a derivative
        a = _ok(_lib, csr, f, _sampled(_lib, deriv=d))
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, kind=_lib.NOISE_EXPLICIT))        # EXPLICIT without weights
    assert call(a) == EINVAL
    for grp in (2, 4, 16, -1):                                             # EXPLICIT: group 0, 1 or D (= 8)
        a = _ok(_lib, csr, f, _explicit(_lib, group=grp))
        assert call(a) == EINVAL, grp
    a = _ok(_lib, csr, f, _sampled(_lib, pos_base=-1))                     # counter bounds: positions
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, pos_base=(1 << 44) - 1))
    assert call(a) == EINVAL
    for cb in (-1, 1 << 20):                                               # ... chunks
        a = _ok(_lib, csr, f, _sampled(_lib, chunk_base=cb))
        assert call(a) == EINVAL
    for mode in (_lib.PARAM_PER_CHANNEL, _lib.PARAM_PER_EDGE1):            # parameter arrays that are not there
        a = _ok(_lib, csr, f, _sampled(_lib, param_mode=mode))
        assert call(a) == EINVAL
        a = _ok(_lib, csr, f, _sampled(_lib, param_mode=mode, p0=32))      # (a Normal has two)
        assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, param_mode=7))
    assert call(a) == EINVAL
    a = _ok(_lib, csr, f, _sampled(_lib, kind=_lib.NOISE_UNIFORM, p1_log=1))   # a log-scale is a Normal's
    assert call(a) == EINVAL
    plan = _lib.Plan(64, 2, 1, 2, None, None, None, None, None, 0, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # plan without units
    assert call(a) == EINVAL
    units = np.zeros((4, 4), np.int32)
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, None, None, f.value, 1 << 20, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # segments without long_seg_ptr
    assert call(a) == EINVAL


def test_w1_entry_leaves_the_two_launch_route_its_cases_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _sampled(_lib)
    call = lambda a: lib.stag_agg_fwd_w1(*a)
    for s in (_sampled(_lib, in_norm=1), _explicit(_lib, in_norm=1)):      # in-norm
        assert call(_ok(_lib, csr, f, s)) == ENOSYS
    a = _ok(_lib, csr, f, spec); a[LDX] = 0                                # a broadcast row
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, _sampled(_lib, chunk_base=1))                    # a channel shard's chunk offset
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, _sampled(_lib, pos_base=(1 << 32) - 1))          # across a 2^32 boundary of the position
    assert call(a) == ENOSYS
    a = _ok(_lib, csr, f, _sampled(_lib, param_mode=_lib.PARAM_PER_CHANNEL, p0=32, p1=32, p1_log=1))
    assert call(a) == ENOSYS                                               # a per-channel log-scale
    units = np.zeros((4, 4), np.int32)
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, f.value, 2 * 8 * 4 - 1, 0, 0, None)
    a = _ok(_lib, csr, f, spec); a[PLAN] = C.byref(plan)                   # workspace one byte short of 2 segments x 8
    assert call(a) == ENOMEM
    # an invalid argument is reported before a case of the other route
    a = _ok(_lib, csr, f, _sampled(_lib, in_norm=1, deriv=1))
    assert call(a) == EINVAL
    # no rows: nothing to do, whatever the pointers
    empty = _lib.Csr(0, 2, 0, _keep.ctypes.data, None, None, None)
    a = _ok(_lib, csr, f, spec); a[CSR] = C.byref(empty)
    assert call(a) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls that pass every check launch on dummy pointers: no device may be present")
def test_w1_entry_takes_every_listed_form():
    """What section 2 of the contract lists as served is refused by no check (without a device the launch itself fails)."""
    _lib, lib, _keep, csr, f = _fixture()
    call = lambda a: lib.stag_agg_fwd_w1(*a)
    forms = [_sampled(_lib), _sampled(_lib, relu=1), _sampled(_lib, p1_log=1),
             _sampled(_lib, kind=_lib.NOISE_UNIFORM), _sampled(_lib, kind=_lib.NOISE_BERNOULLI),
             _sampled(_lib, param_mode=_lib.PARAM_PER_CHANNEL, p0=32, p1=32),
             _sampled(_lib, kind=_lib.NOISE_BERNOULLI, param_mode=_lib.PARAM_PER_CHANNEL, p0=32),
             _sampled(_lib, param_mode=_lib.PARAM_PER_EDGE1, p0=32, p1=32, p1_log=1),
             _sampled(_lib, kind=_lib.NOISE_BERNOULLI, param_mode=_lib.PARAM_PER_EDGE1, p0=32),
             _sampled(_lib, pos_base=(1 << 32) - 2), _sampled(_lib, pos_base=1 << 40),
             _explicit(_lib), _explicit(_lib, group=1), _explicit(_lib, group=8), _explicit(_lib, relu=1)]
    for s in forms:
        for D, ld in ((8, 8), (7, 9), (1, 1), (260, 260), (2, 64)):
            if s.kind == _lib.NOISE_EXPLICIT and s.group > 1 and D != 8:
                continue
            for red in (0, 1):
                a = _ok(_lib, csr, f, s); a[D_] = D; a[LDX] = a[LDO] = ld; a[REDUCE] = red
                assert call(a) not in (EINVAL, ENOSYS, ENOMEM), (s.kind, s.param_mode, D)
    units = np.zeros((4, 4), np.int32)
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, f.value, 2 * 8 * 4, 0, 0, None)
    a = _ok(_lib, csr, f, forms[0]); a[PLAN] = C.byref(plan)               # exactly 2 segments x 8 floats; no counters
    assert call(a) not in (EINVAL, ENOSYS, ENOMEM)


def test_every_refusal_comes_before_the_launch():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "agg_w1.hip")).read()
    body = src[src.index('extern "C" int stag_agg_fwd_w1('):]
    launch = body.index("w1_fwd_launch(")
    assert "return STAG_E" not in body[launch:].replace("STAG_EIO", "")
    assert "hipLaunchKernelGGL" not in body and "hipMemset" not in body    # the entry point itself touches no device


def test_w1_kernels_use_no_scratch():
    """The forward and merge kernels of agg_w1.hip keep their state in registers: 0 scratch bytes in every one."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "agg_w1.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    assert sum("agg_w1_fwd_kernel" in n for n in names) == 4 * 5           # kinds x lanes per row
    assert sum("agg_w1_merge_kernel" in n for n in names) == 5
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import _lib, ops
    monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", True)
    why = ops.edge_weight_why_not
    graph = types.SimpleNamespace(number_of_edges=lambda: 5)

    def noise(**kw):
        d = dict(dn=1, kind=_lib.NOISE_NORMAL, param_mode=_lib.PARAM_SCALAR, in_norm=False, p1_log=False, deriv=0,
                 n_samples=1, grad_params=None, chunk_base=0, pos_base=0, graph=graph)
        d.update(kw)
        n = ops.EdgeNoise.__new__(ops.EdgeNoise)
        n.__dict__.update(d)
        return n

    x = torch.zeros(6, 16)
    w = torch.zeros(5, 1)
    # a CPU tensor passes every clause but the device's (checked last, so that the others can be seen here)
    for weight in (noise(), noise(kind=_lib.NOISE_BERNOULLI), noise(param_mode=_lib.PARAM_PER_EDGE1, p1_log=True),
                   noise(param_mode=_lib.PARAM_PER_CHANNEL), w, w[:, 0], w.double()):
        assert why(x, weight, graph, False) == "device"
    assert why(x[0], w, graph, False) == "shape"
    assert why(x, w, graph, True) == "broadcast row"
    assert why(x[:1].expand(6, 16), w, graph, False) == "broadcast row"
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        assert why(x.to(dt), w, graph, False) == "dtype"
    assert why(x, noise(dn=16), graph, False) == "noise width"
    assert why(x, noise(kind=_lib.NOISE_EXPLICIT), graph, False) == "noise parameters"
    assert why(x, noise(param_mode=_lib.PARAM_PER_EDGE), graph, False) == "noise parameters"
    assert why(x, noise(in_norm=True), graph, False) == "in-norm"
    assert why(x, noise(deriv=1), graph, False) == "derivative selector"
    assert why(x, noise(chunk_base=2), graph, False) == "channel shard"
    assert why(x, noise(n_samples=3), graph, False) == "monte-carlo"
    p = torch.zeros((), requires_grad=True)
    assert why(x, noise(grad_params=(p, 1.0)), graph, False) == "parameter gradients"
    assert why(x, noise(grad_params=(p.detach(), 1.0)), graph, False) == "device"
    assert why(x, noise(pos_base=(1 << 32) - 4), graph, False) == "position range"
    assert why(x, noise(pos_base=(1 << 32) - 5), graph, False) == "device"
    assert why(x, noise(pos_base=3 << 32), graph, False) == "device"
    assert why(x, torch.zeros(5, 2), graph, False) == "weight width"
    assert why(x, torch.zeros(5, 1, 1), graph, False) == "weight width"
    assert why(x, None, graph, False) == "no weight"
    shard = types.SimpleNamespace(is_shard=True, number_of_edges=lambda: 5)
    assert why(x, w, shard, False) == "shard"
    assert why(x, noise(graph=shard), graph, False) == "shard"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(x, w, graph, False) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", False)
    assert why(x, w, graph, False) == "switch" and why(x, noise(), graph, False) == "switch"
    monkeypatch.setattr(ops, "EDGE_WEIGHT_FUSED", True)
    assert why(torch.zeros(6, 16, device="meta"), w, graph, False) == "device"


def test_other_width_mismatches_keep_their_error():
    """Only width 1 is one weight per edge: any other noise width against the feature width is refused as before, before
    anything touches a device."""
    from stag_amd import _lib, ops
    n = ops.EdgeNoise.__new__(ops.EdgeNoise)
    n.__dict__.update(dn=4, n_samples=1, grad_params=None)
    graph = types.SimpleNamespace(number_of_edges=lambda: 5)
    with pytest.raises(ValueError, match="noise width 4 != feature width 16"):
        ops.aggregate(graph, torch.zeros(6, 16), n)
    with pytest.raises(ValueError, match="noise width 4 != feature width 16"):
        ops.aggregate_max(graph, torch.zeros(6, 16), n)


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "edge_weight_time.py"), doraise=True)
