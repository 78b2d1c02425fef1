"""stag_gat_fwd_half (the cooperative GAT forward on fp16 / bf16 ft rows) on the host: ABI surface, every refusal before
any device work, the routing predicate of ops.gat_aggregate clause by clause, the header against the ctypes
prototype, the documents, and the compiler's resource report of the new kernels."""
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

# argument positions of stag_gat_fwd_half
CSR, PLAN, EL, ER, FT, DTYPE, H_, F_, SLOPE, SPEC, NSCALE, DROP, OUT, STATS, STREAM = range(15)


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


def test_header_declares_and_library_exports_the_entry():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    assert re.search(r"\bstag_gat_fwd_half\s*\(", header)
    assert hasattr(_lib.lib(), "stag_gat_fwd_half")
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19      # additive: no bump


def test_header_prototype_matches_the_ctypes_one():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    m = re.search(r"\bint\s+stag_gat_fwd_half\s*\((.*?)\)\s*;", header, re.S)
    assert m
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "csr", "plan", "el", "er", "ft", "ft_dtype", "H", "F", "neg_slope", "spec", "norm_scale", "drop", "out",
        "stats_out", "stream"]

    def ctype(p):
        if "*" in p:
            for name, t in (("stag_csr", _lib.Csr), ("stag_plan", _lib.Plan), ("stag_noise_spec", _lib.NoiseSpec),
                            ("stag_gat_drop", _lib.GatDrop)):
                if name in p:
                    return C.POINTER(t)
            return C.c_void_p
        return {"int32_t": C.c_int32, "float": C.c_float, "int64_t": C.c_int64}[p.split()[-2]]
    assert [ctype(p) for p in params] == list(_lib.lib().stag_gat_fwd_half.argtypes)
    assert _lib.lib().stag_gat_fwd_half.restype == C.c_int


def test_entry_is_documented():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "stag_gat_fwd_half" in open(os.path.join(ROOT, doc)).read(), doc


def _harness():
    _lib, lib, keep, csr, plan, f = _fixture()
    good = _spec(_lib)
    ok = lambda: [C.byref(csr), C.byref(plan), f, f, f, _lib.DTYPE_BF16, 8, 32, 0.2, C.byref(good), None, None, f, f, None]

    def refuses(rc, spec=None, **change):
        a = ok()
        if spec is not None:
            a[SPEC] = C.byref(spec)
        for i, v in change.items():
            a[int(i[1:])] = v
        assert lib.stag_gat_fwd_half(*a) == rc, (change, spec)
    return _lib, lib, keep, csr, plan, f, ok, refuses


def test_refuses_invalid_arguments_without_gpu():
    _lib, lib, keep, csr, plan, f, ok, refuses = _harness()
    a = lambda pos, v: {"a%d" % pos: v}
    for pos in (CSR, SPEC, OUT):                                             # NULL csr / spec / out
        refuses(EINVAL, **a(pos, None))
    for pos in (EL, ER, FT):                                                 # NULL el / er / ft of a graph with edges
        refuses(EINVAL, **a(pos, None))
    refuses(EINVAL, **a(H_, 0))
    refuses(EINVAL, **a(F_, 0))
    refuses(EINVAL, **a(F_, -4))
    for dt in (0, 3, -1):                                                    # unknown ft_dtype
        refuses(EINVAL, **a(DTYPE, dt))
    refuses(EINVAL, spec=_spec(_lib, kind=9))                                # what stag_gat_fwd refuses
    refuses(EINVAL, spec=_spec(_lib, kind=-1))
    refuses(EINVAL, spec=_spec(_lib, kind=_lib.NOISE_BERNOULLI, in_norm=1))  # in-norm without its factors
    refuses(EINVAL, spec=_spec(_lib, kind=_lib.NOISE_EXPLICIT))              # explicit weights that are not there
    refuses(EINVAL, spec=_spec(_lib, param_mode=_lib.PARAM_PER_CHANNEL))     # per-head parameters without their rows
    refuses(EINVAL, spec=_spec(_lib, param_mode=_lib.PARAM_PER_EDGE, p0=16))
    refuses(EINVAL, spec=_spec(_lib, deriv=1))
    refuses(EINVAL, spec=_spec(_lib, pos_base=-1))                           # counter word: positions below 0
    refuses(EINVAL, spec=_spec(_lib, pos_base=(1 << 44) - 1))                # ... and past 2^44
    for keep_prob in (0.0, -0.5):                                            # attention dropout that keeps nothing
        d = _lib.GatDrop(); d.keep_prob = keep_prob
        refuses(EINVAL, **a(DROP, C.byref(d)))
    nounits = _lib.Plan(64, 2, 0, 0, None, None, None, None, None, 0, 0, 1, f.value, None, 0, 0)
    refuses(EINVAL, **a(PLAN, C.byref(nounits)))                             # a plan without unit records
    segp = _lib.Plan(64, 2, 1, 2, keep[1].ctypes.data, f.value, f.value, f.value, None,
                     lib.stag_gat_workspace_bytes(2, 8, 32), 0, 1, f.value, None, 0, 0)
    refuses(EINVAL, **a(PLAN, C.byref(segp)))                                # segments without a workspace
    big = _lib.Csr(2, 2, 1 << 31, keep[0].ctypes.data, keep[0].ctypes.data, None, None)
    refuses(EINVAL, **a(CSR, C.byref(big)))                                  # more edges than int32 positions


def test_leaves_the_cast_route_its_cases_without_gpu():
    _lib, lib, keep, csr, plan, f, ok, refuses = _harness()
    a = lambda pos, v: {"a%d" % pos: v}
    refuses(ENOSYS, **a(PLAN, None))                                         # no plan
    noblk = _lib.Plan(64, 2, 0, 0, keep[1].ctypes.data, None, None, None, None, 0, 0, 0, None, None, 0, 0)
    refuses(ENOSYS, **a(PLAN, C.byref(noblk)))                               # a plan without unit batches
    refuses(ENOSYS, **a(F_, 6))                                              # F % 4 != 0
    refuses(ENOSYS, a6=32, a7=4)                                             # H > 16
    refuses(ENOSYS, a6=12, a7=80)                                            # H * lanes_per_head = 12 * 32 > 256
    refuses(ENOSYS, a6=8, a7=256)                                            # H * F > 1024
    longseg = _lib.Plan(512, 2, 0, 0, keep[1].ctypes.data, None, None, None, None, 0, 0, 1, f.value, None, 0, 0)
    refuses(ENOSYS, **a(PLAN, C.byref(longseg)))                             # seg_len > STAG_BLOCK_EDGES
    refuses(ENOSYS, **a(FT, C.c_void_p(20)))                                 # ft not 8-byte aligned
    refuses(ENOSYS, **a(OUT, C.c_void_p(24)))                                # out not 16-byte aligned
    nbytes = lib.stag_gat_workspace_bytes(2, 8, 32)
    segp = _lib.Plan(64, 2, 1, 2, keep[1].ctypes.data, f.value, f.value, f.value, 24, nbytes, 0, 1, f.value, None, 0, 0)
    refuses(ENOSYS, **a(PLAN, C.byref(segp)))                                # workspace not 16-byte aligned
    refuses(ENOSYS, spec=_spec(_lib, chunk_base=1))                          # heads are not channel-sharded
    refuses(ENOSYS, spec=_spec(_lib, pos_base=(1 << 32) - 1))                # across a 2^32 position boundary
    segp.workspace, segp.workspace_bytes = f.value, nbytes - 1
    refuses(ENOMEM, **a(PLAN, C.byref(segp)))                                # workspace one byte short of 2 states
    # ft 8-byte (not 16-byte) aligned is within the kernel's load width: no refusal on that account
    if not torch.cuda.is_available():
        # the base call passes every check and reaches the launch, which has no device to go to (with a device the
        # dummy pointers would be dereferenced: not exercised there)
        for args in (ok(), [*ok()[:FT], C.c_void_p(24), *ok()[FT + 1:]]):
            assert lib.stag_gat_fwd_half(*args) not in (EINVAL, ENOSYS, ENOMEM)
    empty = _lib.Csr(0, 2, 0, keep[0].ctypes.data, None, None, None)
    assert lib.stag_gat_fwd_half(*[C.byref(empty), *ok()[1:]]) == 0          # no destination row: nothing to do


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import ops
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    why = ops.gat_half_rows_why_not
    ft = torch.zeros(6, 8, 32, dtype=torch.bfloat16)
    # a CPU tensor passes every clause but the device's (checked late, so that the others can be seen here)
    for t in (ft, ft.half()):
        assert why(t) == "device" and not ops.gat_half_rows_ok(t)
    assert why(ft.float()) == "dtype"
    assert why(torch.zeros(6, 4, 6, dtype=torch.bfloat16)) == "shape"            # F % 4
    assert why(torch.zeros(6, 32, 4, dtype=torch.float16)) == "shape"            # H > 16
    assert why(torch.zeros(6, 12, 80, dtype=torch.float16)) == "shape"           # H * lanes per head > 256
    assert why(torch.zeros(6, 256, dtype=torch.bfloat16)) == "shape"             # not [N, H, F]
    assert why(ft, 512) == "shape" and why(ft, None) == "shape" and why(ft, 0) == "shape"    # no block plan of such segments
    assert why(torch.zeros(6, 2, 40, dtype=torch.bfloat16)) == "device"          # F / 4 not a power of two is fine
    assert why(ft, attn_fn=lambda a: a) == "attention function"
    assert why(ft, noise=types.SimpleNamespace(n_samples=3)) == "monte-carlo"
    assert why(ft, noise=types.SimpleNamespace(n_samples=1, graph=types.SimpleNamespace())) == "device"
    assert why(ft, graph=types.SimpleNamespace(is_shard=True)) == "shard"
    assert why(ft, noise=types.SimpleNamespace(n_samples=1, graph=types.SimpleNamespace(is_shard=True))) == "shard"
    assert why(torch.zeros(6, 32, 8, dtype=torch.bfloat16).transpose(1, 2)) == "strides"
    assert why(torch.zeros(6, 8, 64, dtype=torch.bfloat16)[:, :, :32]) == "strides"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(ft) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", False)
    assert why(ft) == "switch"
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    assert not ops.gat_half_rows_ok(torch.zeros(6, 8, 32, dtype=torch.bfloat16, device="meta"))
    assert ops.GAT_HALF_FT is False                                               # autocast layers: opt-in


def test_layer_switch_is_inert_on_the_host(monkeypatch):
    """zoo.GAT on CPU tensors (no autocast on a device, no fused kernels) never takes the half-ft form."""
    import stag_amd
    from stag_amd import ops
    monkeypatch.setattr(ops, "GAT_HALF_FT", True)
    monkeypatch.setattr(ops, "GAT_HALF_ROWS", True)
    layer = stag_amd.zoo.GAT(12, 8, num_heads=4)
    h = torch.zeros(5, 12)
    assert layer._half_ft(None, h, 4, 8, None, False) is False
    assert layer.extra_offsets_per_forward() == 0
    layer.train()
    layer.attn_drop.p = 0.6
    assert layer.extra_offsets_per_forward() == 1                                 # counts what it counted


def test_half_kernels_use_no_scratch():
    """Every half-row instantiation of gat_fwd_block_kernel<DT, ...> (DT 1 fp16, 2 bf16) keeps its state in registers: 2 dtypes x (5 of one chunk per
    lane + 2 x 2 wider), 0 scratch bytes, no spilled VGPR."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "gat.remarks")).read()
    found = re.findall(r"Function Name: (\S*gat_fwd_block_kernelILi[12]E\S*).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)",
                       text, re.S)
    assert len(found) == 18, [n for n, _, _ in found]
    assert all(int(s) == 0 and int(v) == 0 for _, s, v in found), [n for n, s, v in found if int(s) or int(v)]


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "gat_half_time.py"), doraise=True)
