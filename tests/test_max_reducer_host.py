"""The fused max reducer (stag_agg_max_fwd / stag_agg_max_bwd) on the host: ABI surface, argument checks before any
device work, the Meta kernels of the dispatcher ops, and the compiler's resource report of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ENOSYS = -22, -12, -38


def test_header_declares_and_library_exports_the_max_entries():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    for name in ("stag_agg_max_fwd", "stag_agg_max_bwd", "stag_agg_max_bwd_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(_lib.lib(), name), name
    assert "#define STAG_ABI_VERSION 19" in header
    lib = _lib.lib()
    assert lib.stag_agg_max_bwd_scratch_bytes(10, 12) == 10 * 3 * 8 * 4
    assert lib.stag_agg_max_bwd_scratch_bytes(10, 13) == 10 * 4 * 8 * 4
    assert lib.stag_agg_max_bwd_scratch_bytes(0, 12) == 0


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, indptr.ctypes.data, None, indptr.ctypes.data)   # never dereferenced
    return _lib, _lib.lib(), indptr, csr, C.c_void_p(16)     # f: a non-null, 16-B aligned dummy "device pointer"


def test_max_fwd_refuses_bad_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _lib.NoiseSpec()
    ok = lambda: [C.byref(csr), None, f, 4, 4, C.byref(spec), f, 4, f, 4, None]
    a = ok(); a[0] = None
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # no graph
    a = ok(); a[6] = None
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # no output
    a = ok(); a[3] = 2
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # ldx < D
    a = ok(); a[7] = 3
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # ldo < D
    a = ok(); a[9] = 3
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # ldc < D
    a = ok(); a[4] = 0
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # D = 0
    bad = _lib.NoiseSpec(); bad.kind = 9
    a = ok(); a[5] = C.byref(bad)
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # unknown kind
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_EXPLICIT
    a = ok(); a[5] = C.byref(bad)
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # explicit weights without p0
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_NORMAL; bad.pos_base = (1 << 44) - 1
    a = ok(); a[5] = C.byref(bad)
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # counter overflow (positions past 2^44)
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_NORMAL; bad.chunk_base = (1 << 20) - 1
    a = ok(); a[5] = C.byref(bad); a[3] = a[4] = a[7] = a[9] = 8
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # counter overflow (chunk field: 2 chunks)
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_NORMAL; bad.pos_base = (1 << 32) - 1
    a = ok(); a[5] = C.byref(bad)
    assert lib.stag_agg_max_fwd(*a) == ENOSYS                               # launch would straddle 2^32 positions
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_NORMAL; bad.in_norm = 1
    a = ok(); a[5] = C.byref(bad)
    assert lib.stag_agg_max_fwd(*a) == ENOSYS                               # in-norm: the composed route
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_NORMAL; bad.deriv = 1
    a = ok(); a[5] = C.byref(bad)
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # a derivative is not a message
    plan = _lib.Plan(64, 2, 1, 2, None, None, None, None, None, 0, 0, 0, None)
    a = ok(); a[1] = C.byref(plan)
    assert lib.stag_agg_max_fwd(*a) == EINVAL                               # plan without units
    units = np.zeros((4, 4), np.int32)
    plan = _lib.Plan(1, 3, 1, 2, units.ctypes.data, f.value, f.value, None, f.value, 8, 0, 0, None)
    a = ok(); a[1] = C.byref(plan)
    assert lib.stag_agg_max_fwd(*a) == ENOMEM                               # segment workspace too small (2 x 2 x 4 x 4)


def test_max_bwd_refuses_bad_arguments_without_gpu():
    _lib, lib, _keep, csr, f = _fixture()
    spec = _lib.NoiseSpec()
    ok = lambda: [C.byref(csr), None, f, 4, f, f, f, 4, 4, C.byref(spec), f, None, 0, None, None, 4, f, 1 << 20, None]
    a = ok(); a[0] = None
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # no graph
    a = ok(); a[10] = None
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # no output at all
    a = ok(); a[3] = 2
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # ldx < D
    a = ok(); a[4] = None
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # the forward's out missing
    a = ok(); a[5] = None
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # the tie counts missing
    a = ok(); a[13] = f
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # dp0 without dp1
    a = ok(); a[13] = f; a[14] = f
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # parameter rows of no draw
    a = ok(); a[11] = f; a[12] = 4
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # dw of weights that are not explicit
    a = ok(); a[17] = 16
    assert lib.stag_agg_max_bwd(*a) == ENOMEM                               # scratch too small
    bad = _lib.NoiseSpec(); bad.kind = 9
    a = ok(); a[9] = C.byref(bad)
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # unknown kind
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_NORMAL; bad.in_norm = 1
    a = ok(); a[9] = C.byref(bad)
    assert lib.stag_agg_max_bwd(*a) == ENOSYS                               # in-norm
    p = C.c_void_p(32)
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_NORMAL; bad.param_mode = _lib.PARAM_PER_EDGE1; bad.p0 = p; bad.p1 = p
    a = ok(); a[9] = C.byref(bad)
    assert lib.stag_agg_max_bwd(*a) == ENOSYS                               # [E, 1] parameters
    bad = _lib.NoiseSpec(); bad.kind = _lib.NOISE_UNIFORM; bad.pos_base = (1 << 44) - 1
    a = ok(); a[9] = C.byref(bad)
    assert lib.stag_agg_max_bwd(*a) == EINVAL                               # counter overflow


def test_max_dispatcher_ops_have_meta_kernels():
    from stag_amd import _torch_ext
    assert _torch_ext.loaded()
    ip = torch.zeros(6, dtype=torch.int32, device="meta")
    ix = torch.zeros(9, dtype=torch.int32, device="meta")
    x = torch.zeros(5, 12, device="meta")
    noise = ([2, 0, 0, 0, 0, 0, 0, 0], [1, 2, 0], [0.0, 1.0], None, None, None)
    plan = (None, None, None, None, None, None, [0] * 8)
    out, cnt = torch.ops.stag.agg_max_fwd(ip, ix, None, None, 5, *plan, x, False, *noise, True)
    assert out.shape == (5, 12) and out.dtype == torch.float32 and out.device.type == "meta"
    assert cnt.shape == (5, 12) and cnt.dtype == torch.int32
    out, cnt = torch.ops.stag.agg_max_fwd(ip, ix, None, None, 5, *plan, torch.zeros(1, 7, device="meta"), True, *noise, False)
    assert out.shape == (5, 7) and cnt.numel() == 0
    g = torch.zeros(5, 12, device="meta")
    c = torch.zeros(5, 12, dtype=torch.int32, device="meta")
    dx, dw, t0, t1 = torch.ops.stag.agg_max_bwd(ip, ix, None, None, 5, *plan, x, False, g, c, g, *noise, True, True, True)
    assert dx.shape == (5, 12) and dw.shape == (9, 12) and t0.shape == (5, 12) and t1.shape == (5, 12)
    dx, dw, t0, t1 = torch.ops.stag.agg_max_bwd(ip, ix, None, None, 5, *plan, x, False, g, c, g, *noise, True, False, False)
    assert dx.shape == (5, 12) and dw.numel() == 0 and t0.numel() == 0 and t1.numel() == 0


def test_max_kernels_use_no_scratch():
    """Every kernel of agg_max.hip keeps its state in registers: the compiler's report shows 0 scratch bytes."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "agg_max.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    for k in ("agg_max_fwd_kernel", "agg_max_merge_kernel", "agg_max_prep_kernel", "agg_max_bwd_kernel",
              "agg_max_bwd_merge_kernel"):
        assert any(k in n for n in names), k
    assert len(found) >= 5 * 2 * 7
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]
