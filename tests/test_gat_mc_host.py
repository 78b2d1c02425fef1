"""Monte-Carlo GAT forward (stag_gat_fwd_mc) on the host: ABI surface, workspace sizes, argument checks before any
device work, the Meta kernel of the dispatcher op, and the compiler's resource report of the new kernels (0 scratch;
the existing GAT kernels exactly as they compiled before the Monte-Carlo form was added)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ENOSYS = -22, -12, -38


def test_header_declares_and_library_exports_the_gat_mc_entries():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    for name in ("stag_gat_fwd_mc", "stag_gat_fwd_mc_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(_lib.lib(), name), name
    assert "#define STAG_ABI_VERSION 19" in header
    assert _lib.lib().stag_abi_version() == 19


def test_gat_mc_workspace_bytes():
    from stag_amd import _lib
    lib = _lib.lib()
    row = lambda H, F: ((H * F + 2 * H + 3) & ~3) * 4          # one segment state of stag_gat_workspace_bytes
    assert lib.stag_gat_fwd_mc_workspace_bytes(10, 8, 32, 1) == 10 * row(8, 32)
    assert lib.stag_gat_fwd_mc_workspace_bytes(10, 8, 32, 3) == 3 * 10 * row(8, 32)
    assert lib.stag_gat_fwd_mc_workspace_bytes(10, 8, 32, 4) == 4 * 10 * row(8, 32)
    assert lib.stag_gat_fwd_mc_workspace_bytes(10, 8, 32, 8) == 4 * 10 * row(8, 32)    # a pass carries <= 4 samples
    assert lib.stag_gat_fwd_mc_workspace_bytes(7, 4, 256, 2) == 2 * 7 * row(4, 256)
    assert lib.stag_gat_fwd_mc_workspace_bytes(7, 3, 5, 2) == 2 * 7 * row(3, 5)
    assert lib.stag_gat_fwd_mc_workspace_bytes(7, 4, 256, 2) == 2 * lib.stag_gat_workspace_bytes(7, 4, 256)
    assert lib.stag_gat_fwd_mc_workspace_bytes(0, 8, 32, 4) == 0
    assert lib.stag_gat_fwd_mc_workspace_bytes(10, 8, 32, 0) == 0


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, indptr.ctypes.data, None, indptr.ctypes.data)   # never dereferenced
    units = np.zeros((4, 4), np.int32)
    f = C.c_void_p(16)            # a non-null, 16-B aligned dummy "device pointer"
    # a block plan without segments (n_seg = 0): every check passes, so each case below isolates one refusal
    plan = _lib.Plan(64, 2, 0, 0, units.ctypes.data, None, None, None, None, 0, 0, 1, f.value, None, 0, 0)
    return _lib, _lib.lib(), (indptr, units), csr, plan, f


def _spec(_lib, **kw):
    s = _lib.NoiseSpec()
    s.kind, s.p0_scalar, s.p1_scalar = _lib.NOISE_NORMAL, 1.0, 0.5
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_gat_mc_refuses_bad_arguments_without_gpu():
    _lib, lib, _keep, csr, plan, f = _fixture()
    H, F = 8, 32
    good = _spec(_lib)
    # csr, plan, el, er, ft, H, F, neg_slope, spec, n_samples, offset_stride, out, out_stride, stats, stats_stride, stream
    ok = lambda: [C.byref(csr), C.byref(plan), f, f, f, H, F, 0.2, C.byref(good), 4, 1, f, 2 * H * F, f, 2 * 2 * H, None]
    call = lambda a: lib.stag_gat_fwd_mc(*a)

    def refuses(rc, **change):
        a = ok()
        for i, v in change.items():
            a[int(i[1:])] = v
        assert call(a) == rc, change

    def refuses_spec(rc, **kw):
        s = _spec(_lib, **kw)
        a = ok()
        a[8] = C.byref(s)
        assert call(a) == rc, kw

    # EINVAL: null pointers
    refuses(EINVAL, a0=None)                     # no graph
    refuses(EINVAL, a2=None)                     # el
    refuses(EINVAL, a3=None)                     # er
    refuses(EINVAL, a4=None)                     # ft
    refuses(EINVAL, a8=None)                     # spec
    refuses(EINVAL, a11=None)                    # out
    # EINVAL: counts and strides
    refuses(EINVAL, a9=0)                        # n_samples < 1
    refuses(EINVAL, a9=-3)
    refuses(EINVAL, a10=-1)                      # offset_stride < 0
    refuses(EINVAL, a12=2 * H * F - 4)           # out_stride smaller than one sample
    refuses(EINVAL, a14=2 * 2 * H - 1)           # stats_stride smaller than one sample
    refuses(EINVAL, a5=0)                        # H = 0
    refuses(EINVAL, a6=0)                        # F = 0
    # EINVAL: the noise it draws
    refuses_spec(EINVAL, kind=_lib.NOISE_NONE)
    refuses_spec(EINVAL, kind=_lib.NOISE_EXPLICIT, p0=16)
    refuses_spec(EINVAL, kind=9)
    refuses_spec(EINVAL, param_mode=_lib.PARAM_PER_EDGE1, p0=16, p1=16)
    refuses_spec(EINVAL, param_mode=_lib.PARAM_PER_EDGE, p0=16, p1=16)
    refuses_spec(EINVAL, param_mode=_lib.PARAM_PER_CHANNEL)          # per-head parameters without their rows
    refuses_spec(EINVAL, in_norm=1)
    refuses_spec(EINVAL, deriv=1)
    refuses_spec(EINVAL, pos_base=-1)                                # counter word: positions below 0
    refuses_spec(EINVAL, pos_base=(1 << 44) - 1)                     # ... and past 2^44
    # ENOSYS: outside the cooperative form, or across a 2^32 position boundary
    refuses_spec(ENOSYS, pos_base=(1 << 32) - 1)
    refuses(ENOSYS, a1=None)                                         # no plan
    noblk = _lib.Plan(64, 2, 0, 0, _keep[1].ctypes.data, None, None, None, None, 0, 0, 0, None, None, 0, 0)
    refuses(ENOSYS, a1=C.byref(noblk))                               # a plan without unit batches
    refuses(ENOSYS, a6=6, a12=2 * H * 6)                             # F % 4 != 0
    refuses(ENOSYS, a5=32, a6=4, a12=2 * 32 * 4, a14=2 * 2 * 32)     # H > 16
    refuses(ENOSYS, a5=8, a6=256, a12=2 * 8 * 256)                   # H * F > 1024
    refuses(ENOSYS, a11=C.c_void_p(20), a9=1)                        # out not 16-B aligned
    # with segments: the workspace must hold min(n_samples, samples per pass) states per segment
    segp = _lib.Plan(64, 2, 1, 2, _keep[1].ctypes.data, f.value, f.value, f.value, f.value,
                     lib.stag_gat_fwd_mc_workspace_bytes(2, H, F, 1), 0, 1, f.value, None, 0, 0)
    refuses(ENOMEM, a1=C.byref(segp))
    segp.workspace = None
    refuses(EINVAL, a1=C.byref(segp))                                # segments without a workspace


def test_gat_mc_dispatcher_op_has_a_meta_kernel():
    from stag_amd import _torch_ext
    assert _torch_ext.loaded()
    ip = torch.zeros(6, dtype=torch.int32, device="meta")
    ix = torch.zeros(9, dtype=torch.int32, device="meta")
    el = torch.zeros(7, 4, device="meta")
    ft = torch.zeros(7, 4, 12, device="meta")
    noise = ([2, 0, 0, 0, 0, 0, 0, 0], [1, 2, 0], [0.0, 1.0], None, None, None)
    plan = (None, None, None, None, None, None, [0] * 8)
    out, stats = torch.ops.stag.gat_fwd_mc(ip, ix, None, None, 7, *plan, el, el, ft, 0.2, *noise, 5, 1, True)
    assert out.shape == (5, 5, 4, 12) and out.dtype == torch.float32 and out.device.type == "meta"
    assert stats.shape == (5, 5, 8)
    out, stats = torch.ops.stag.gat_fwd_mc(ip, ix, None, None, 7, *plan, el, el, ft, 0.2, *noise, 3, 2, False)
    assert out.shape == (3, 5, 4, 12) and stats.numel() == 0


def _resources(path):
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = []
            continue
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if m and cur:
            res[cur].append(m.group(1))
    return res


def _gat_remarks():
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    return _resources(os.path.join(csrc, "_obj", "gat.remarks"))


def test_gat_mc_kernels_use_no_scratch():
    """Every instantiation of gat_fwd_mc_block_kernel keeps its accumulators in registers: 0 scratch bytes, no
    spilled VGPR — the (LPE, CPL, NRF) triples stag_gat_fwd launches: 5 of one chunk per lane, 2 x 2 wider."""
    res = {k: v for k, v in _gat_remarks().items() if "gat_fwd_mc_block_kernel" in k}
    assert len(res) == 9, sorted(res)
    for name, lines in res.items():
        assert "ScratchSize [bytes/lane]: 0" in lines, (name, lines)
        assert "VGPRs Spill: 0" in lines, (name, lines)


def test_existing_gat_kernels_compile_as_before():
    """The resource lines of every kernel of gat.hip (registers, SGPRs, LDS, scratch, occupancy) are those of
    tests/golden/gat_kernel_resources.json, recorded from the build before the fp32 and half-row forward kernels became
    one template (gat_fwd_block_kernel<DT, ...>: DT 0 fp32, 1 fp16, 2 bf16), under the names they have since; and
    gat.hip compiles exactly these kernels."""
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "gat_kernel_resources.json")))
    now = _gat_remarks()
    assert len(before) == 80
    assert set(now) == set(before), sorted(set(now) ^ set(before))
    changed = [k for k in before if now.get(k) != before[k]]
    assert not changed, changed
