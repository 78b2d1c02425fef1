"""The fused node block (stag_node_norm_stats / _fwd / _bwd: BatchNorm1d + ReLU + Dropout between two layers) on the host:
ABI surface, every refusal before any device work and in the stated order, the compiler's resource report of the new
kernels, the routing predicate of FeatOnlyLayer clause by clause, the CPU route of FeatOnlyLayer, and the timing tool."""
import ctypes as C
import os
import py_compile
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ENOSYS = -22, -12, -38

PROTOTYPES = {
    "size_t stag_node_norm_workspace_bytes": ("int64_t n_rows, int32_t D", [C.c_int64, C.c_int32]),
    "int stag_node_norm_stats": (
        "const float* x, int64_t ldx, int64_t n_rows, int32_t D, float eps, float* mean_out, float* rstd_out, "
        "float* running_mean, float* running_var, float momentum_factor, void* workspace, size_t workspace_bytes, "
        "void* stream",
        "p q q i f p p p p f p z p"),
    "int stag_node_norm_fwd": (
        "const float* x, int64_t ldx, int64_t n_rows, int32_t D, const float* mean, const float* rstd, "
        "const float* gamma, const float* beta, int32_t relu, const stag_node_drop* drop, float* y, int64_t ldy, "
        "void* stream",
        "p q q i p p p p i d p q p"),
    "int stag_node_norm_bwd": (
        "const float* x, int64_t ldx, const float* g, int64_t ldg, int64_t n_rows, int32_t D, const float* mean, "
        "const float* rstd, const float* gamma, const float* beta, int32_t relu, const stag_node_drop* drop, "
        "int32_t batch_stats, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* workspace, "
        "size_t workspace_bytes, void* stream",
        "p q p q q i p p p p i d i p q p p p z p"),
}


def test_header_prototypes_match_the_ctypes_ones_and_the_abi_is_kept():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    kinds = {"p": C.c_void_p, "q": C.c_int64, "i": C.c_int32, "f": C.c_float, "z": C.c_size_t,
             "d": C.POINTER(_lib.NodeDrop)}
    first = None
    for decl, (args, ctypes_args) in PROTOTYPES.items():
        name = decl.split()[-1]
        m = re.search(re.escape(decl) + r"\s*\(([^;]*)\);", header)
        assert m, decl
        first = m.start() if first is None else min(first, m.start())
        assert re.sub(r"\s+", " ", m.group(1)) == args, name
        fn = getattr(_lib.lib(), name)
        want = ctypes_args if isinstance(ctypes_args, list) else [kinds[k] for k in ctypes_args.split()]
        assert list(fn.argtypes) == want, name
        assert len(want) == args.count(",") + 1
    assert _lib.lib().stag_node_norm_workspace_bytes.restype is C.c_size_t
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19      # additive
    # the struct: the layout of stag_gat_drop, field by field
    assert [(n, t) for n, t in _lib.NodeDrop._fields_] == [(n, t) for n, t in _lib.GatDrop._fields_]
    assert C.sizeof(_lib.NodeDrop) == C.sizeof(_lib.GatDrop) == 32
    s = re.search(r"typedef struct stag_node_drop \{(.*?)\} stag_node_drop;", header, re.S).group(1)
    assert re.findall(r"(float|uint64_t|const uint64_t\*) ([a-z_, ]+);", s) == [
        ("float", "keep_prob"), ("uint64_t", "seed, offset"), ("const uint64_t*", "epoch")]
    para = header[:first].rsplit("/* ----", 1)[1]
    for word in ("xhat", "[pre > 0]", "Chan", "slab order", "No atomics", "identity graph", "STAG_EINVAL", "STAG_ENOSYS",
                 "STAG_ENOMEM", "n_rows == 0"):
        assert word in para, word


def _lib_and_f():
    from stag_amd import _lib
    return _lib, _lib.lib(), C.c_void_p(16)     # f: a non-null, 16-byte aligned dummy "device pointer"


# argument positions
SX, SLDX, SN, SD, SEPS, SMEAN, SRSTD, SRM, SRV, SFAC, SWS, SWSB, SSTREAM = range(13)
FX, FLDX, FN, FD, FMEAN, FRSTD, FGAMMA, FBETA, FRELU, FDROP, FY, FLDY, FSTREAM = range(13)
(BX, BLDX, BG, BLDG, BN, BD, BMEAN, BRSTD, BGAMMA, BBETA, BRELU, BDROP, BBATCH, BDX, BLDDX, BDGAMMA, BDBETA, BWS, BWSB,
 BSTREAM) = range(20)
BIG = 1 << 30      # "enough" workspace bytes


def _stats_ok(f):
    return [f, 8, 100, 8, 1e-5, f, f, f, f, 0.1, f, BIG, None]


def _fwd_ok(f, drop=None):
    return [f, 8, 100, 8, f, f, f, f, 1, drop, f, 8, None]


def _bwd_ok(f, drop=None):
    return [f, 8, f, 8, 100, 8, f, f, f, f, 1, drop, 1, f, 8, f, f, f, BIG, None]


def _drop(_lib, keep=0.5):
    return _lib.NodeDrop(keep, 1, 2, None)


def test_workspace_bytes_is_a_function_of_the_shape_alone():
    _lib, lib, _f = _lib_and_f()
    ws = lib.stag_node_norm_workspace_bytes
    assert ws(0, 8) == 0 and ws(8, 0) == 0 and ws(-1, 8) == 0
    # (slabs + 1) rows of 2 D floats; 64-row slabs up to 131,072 rows, then at most 2048 slabs
    assert ws(1, 8) == 2 * 2 * 8 * 4 and ws(64, 8) == 2 * 2 * 8 * 4 and ws(65, 8) == 3 * 2 * 8 * 4
    assert ws(131072, 128) == 2049 * 2 * 128 * 4 and ws(131073, 128) == (1025 + 1) * 2 * 128 * 4
    assert ws(169343, 128) == (1323 + 1) * 2 * 128 * 4


def test_stats_entry_refuses_in_order_without_gpu():
    _lib, lib, f = _lib_and_f()
    call = lambda a: lib.stag_node_norm_stats(*a)
    for pos, bad in ((SD, 0), (SD, -4), (SN, -1), (SLDX, 7), (SLDX, 0), (SEPS, 0.0), (SEPS, -1e-5), (SEPS, float("inf")),
                     (SEPS, float("nan")), (SFAC, float("nan")), (SFAC, float("inf"))):
        a = _stats_ok(f); a[pos] = bad
        assert call(a) == EINVAL, (pos, bad)
    for pos in (SX, SMEAN, SRSTD, SWS):                                    # a NULL required pointer with rows
        a = _stats_ok(f); a[pos] = None
        assert call(a) == EINVAL, pos
    a = _stats_ok(f); a[SRM] = a[SRV] = None; a[SFAC] = float("nan")       # no running buffer: the factor is not read
    a[SWSB] = 0
    assert call(a) == ENOMEM
    need = lib.stag_node_norm_workspace_bytes(100, 8)
    a = _stats_ok(f); a[SWSB] = need - 1
    assert call(a) == ENOMEM
    # what the entry has no form for comes before the workspace, an invalid argument before both
    a = _stats_ok(f); a[SN] = (1 << 34) + 1; a[SWSB] = 0
    assert call(a) == ENOSYS
    a = _stats_ok(f); a[SD] = a[SLDX] = (1 << 22) + 1; a[SWSB] = 0
    assert call(a) == ENOSYS
    a[SEPS] = 0.0
    assert call(a) == EINVAL
    a = _stats_ok(f); a[SWSB] = 0; a[SX] = None
    assert call(a) == EINVAL
    # no rows: nothing to do, whatever the pointers, but the shape is still checked
    a = _stats_ok(f); a[SN] = 0; a[SWSB] = 0
    for pos in (SX, SMEAN, SRSTD, SRM, SRV, SWS):
        a[pos] = None
    assert call(a) == 0
    a[SD] = 0
    assert call(a) == EINVAL


def test_forward_entry_refuses_in_order_without_gpu():
    _lib, lib, f = _lib_and_f()
    call = lambda a: lib.stag_node_norm_fwd(*a)
    for pos, bad in ((FD, 0), (FD, -4), (FN, -1), (FLDX, 7), (FLDY, 7), (FLDY, 0)):
        a = _fwd_ok(f); a[pos] = bad
        assert call(a) == EINVAL, (pos, bad)
    for keep in (0.0, -0.5, 1.5, float("nan")):                            # keep_prob outside (0, 1]
        d = _drop(_lib, keep)
        assert call(_fwd_ok(f, C.byref(d))) == EINVAL, keep
    d = _drop(_lib)
    a = _fwd_ok(f, C.byref(d)); a[FN] = (1 << 44) + 1                      # rows outside the counter space
    assert call(a) == EINVAL
    a[FDROP] = None                                                        # ... without a mask: no form for that many
    assert call(a) == ENOSYS
    a = _fwd_ok(f, C.byref(d)); a[FD] = a[FLDX] = a[FLDY] = (1 << 22) + 1  # chunks outside the counter space
    assert call(a) == EINVAL
    a[FDROP] = None
    assert call(a) == ENOSYS
    a[FX] = None                                                           # an invalid argument comes first
    assert call(a) == EINVAL
    for pos in (FX, FMEAN, FRSTD, FY):
        a = _fwd_ok(f); a[pos] = None
        assert call(a) == EINVAL, pos
    a = _fwd_ok(f, C.byref(d)); a[FN] = 0
    for pos in (FX, FMEAN, FRSTD, FGAMMA, FBETA, FY):
        a[pos] = None
    assert call(a) == 0
    a[FLDX] = 7
    assert call(a) == EINVAL


def test_backward_entry_refuses_in_order_without_gpu():
    _lib, lib, f = _lib_and_f()
    call = lambda a: lib.stag_node_norm_bwd(*a)
    for pos, bad in ((BD, 0), (BD, -4), (BN, -1), (BLDX, 7), (BLDG, 7), (BLDDX, 7)):
        a = _bwd_ok(f); a[pos] = bad
        assert call(a) == EINVAL, (pos, bad)
    for keep in (0.0, -0.5, 1.5, float("nan")):
        d = _drop(_lib, keep)
        assert call(_bwd_ok(f, C.byref(d))) == EINVAL, keep
    d = _drop(_lib)
    a = _bwd_ok(f, C.byref(d)); a[BN] = (1 << 44) + 1
    assert call(a) == EINVAL
    for pos in (BX, BG, BMEAN, BRSTD, BWS):
        a = _bwd_ok(f); a[pos] = None
        assert call(a) == EINVAL, pos
    a = _bwd_ok(f); a[BWSB] = lib.stag_node_norm_workspace_bytes(100, 8) - 1
    assert call(a) == ENOMEM
    a[BN] = (1 << 34) + 1                                                  # no form: before the workspace
    assert call(a) == ENOSYS
    a[BLDG] = 7                                                            # invalid: before both
    assert call(a) == EINVAL
    # running statistics and no parameter gradient: no sums, so no workspace is read
    a = _bwd_ok(f); a[BBATCH] = 0; a[BDGAMMA] = a[BDBETA] = None; a[BWS] = None; a[BWSB] = 0; a[BDX] = None
    assert call(a) == 0                                                    # ... and nothing at all to do
    a = _bwd_ok(f); a[BDX] = None; a[BLDDX] = 0                            # the stride of an absent dx is not read
    a[BWSB] = 0
    assert call(a) == ENOMEM
    a = _bwd_ok(f, C.byref(d)); a[BN] = 0
    for pos in (BX, BG, BMEAN, BRSTD, BGAMMA, BBETA, BDX, BDGAMMA, BDBETA, BWS):
        a[pos] = None
    assert call(a) == 0
    a[BD] = 0
    assert call(a) == EINVAL


def test_every_refusal_comes_before_the_launch():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "node_norm.hip")).read()
    for entry, launch in (("stag_node_norm_stats(", "node_stats_launch("), ("stag_node_norm_fwd(", "node_fwd_launch("),
                          ("stag_node_norm_bwd(", "node_bwd_launch(")):
        body = src[src.index('extern "C" int ' + entry):]
        body = body[:body.index("\n}\n") + 3]
        at = body.index(launch)
        assert "return STAG_E" not in body[at:].replace("STAG_EIO", "")
        assert "hipLaunchKernelGGL" not in body and "hipMemset" not in body    # the entry points themselves touch no device
    assert "atomic" not in src.split("#include", 1)[1].lower()                 # (the header comment says "No atomics")


def test_node_norm_kernels_use_no_scratch():
    """Every instantiation of the six kernels of node_norm.hip keeps its state in registers: 0 scratch bytes."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "node_norm.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    for kernel in ("node_stats_kernel", "node_fwd_kernel", "node_bsum_kernel", "node_dx_kernel"):
        assert sum(kernel in n for n in names) == 5, kernel                # lanes per row: 64, 32, 16, 8, 4
    for kernel in ("node_stats_merge_kernel", "node_bsum_merge_kernel"):
        assert sum(kernel in n for n in names) == 1, kernel
    assert len(found) == 22
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]


class _OnDevice:
    """A stand-in that passes the device clause (no device is present here)."""

    def __init__(self, t):
        self.t = t
        self.is_cuda = True

    def __getattr__(self, k):
        return getattr(self.t, k)


def _block(*tail, width=8):
    return torch.nn.Sequential(torch.nn.BatchNorm1d(width), *tail)


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import ops
    nn = torch.nn
    monkeypatch.setattr(ops, "NODE_BLOCK_FUSED", True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    why = ops.node_block_why_not
    cpu = torch.zeros(6, 8)
    p = _OnDevice(cpu)
    for block in (_block(nn.ReLU(), nn.Dropout(0.5)), _block(nn.ReLU()), _block(nn.Dropout(0.5)), _block(),
                  _block(nn.ReLU(inplace=True), nn.Dropout(0.0)),
                  nn.Sequential(nn.BatchNorm1d(8, affine=False, track_running_stats=False, momentum=None), nn.ReLU())):
        assert why(block, p) is None, block
        assert why(block.eval(), p) is None

    class MyReLU(nn.ReLU):               # a subclass may compute anything: exactly the three classes
        pass

    class MyBN(nn.BatchNorm1d):
        pass

    class MySeq(nn.Sequential):
        pass
    for other in (_block(nn.Tanh()), nn.Sequential(nn.ReLU(), nn.BatchNorm1d(8)), nn.BatchNorm1d(8),
                  _block(nn.Dropout(0.5), nn.ReLU()), _block(nn.ReLU(), nn.ReLU()), _block(nn.ReLU(), nn.Dropout(0.5), nn.ReLU()),
                  _block(nn.ReLU(), nn.Dropout(0.5), nn.Dropout(0.5)), _block(MyReLU()), nn.Sequential(MyBN(8), nn.ReLU()),
                  MySeq(nn.BatchNorm1d(8), nn.ReLU()), nn.Sequential(), nn.Sequential(nn.LayerNorm(8), nn.ReLU()),
                  _block(nn.ReLU(), nn.AlphaDropout(0.5)), nn.Sequential(nn.BatchNorm2d(8), nn.ReLU()),
                  _block(nn.ReLU()).double(), nn.Identity(), nn.Dropout(0.5)):
        assert why(other, p) == "module", other
    block = _block(nn.ReLU(), nn.Dropout(0.5))
    assert why(block, _OnDevice(torch.zeros(2, 8, 5))) == "shape"            # [N, C, L]
    assert why(block, _OnDevice(torch.zeros(8))) == "shape"
    assert why(block, _OnDevice(torch.zeros(6, 9))) == "shape"
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        assert why(block, _OnDevice(cpu.to(dt))) == "dtype"
    assert why(block, cpu) == "device" and why(block, torch.zeros(6, 8, device="meta")) == "device"
    assert why(block, _OnDevice(cpu[:1])) == "rows"                          # torch raises on one training row
    assert why(block.eval(), _OnDevice(cpu[:1])) is None
    assert why(block, _OnDevice(cpu[:0])) == "rows"
    norun = nn.Sequential(nn.BatchNorm1d(8, track_running_stats=False)).eval()   # batch statistics in eval mode too
    assert why(norun, _OnDevice(cpu[:1])) == "rows" and why(norun, _OnDevice(cpu[:2])) is None
    block.train()
    assert why(_block(nn.Dropout(1.0)), p) == "dropout"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(block, p) == "compiling"
    assert why(block, cpu) == "device"                                       # (the earlier clauses come first)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert why(block, p) == "capturing"
    assert why(_block(nn.Dropout(1.0)), p) == "dropout"
    monkeypatch.setattr(ops, "NODE_BLOCK_FUSED", False)
    assert why(block, p) == "switch" and why(nn.Identity(), cpu) == "switch"


def test_double_backward_is_refused_not_wrong():
    from stag_amd import ops
    import inspect
    assert "once_differentiable" in inspect.getsource(ops._NodeBlock)


@pytest.mark.parametrize("train", [True, False])
def test_feat_only_layer_on_cpu_is_the_torch_route_bit_for_bit(train, monkeypatch):
    import stag_amd
    from stag_amd import ops, random as srandom
    monkeypatch.setattr(ops, "NODE_BLOCK_FUSED", True)
    torch.manual_seed(3)
    block = torch.nn.Sequential(torch.nn.BatchNorm1d(8), torch.nn.ReLU(), torch.nn.Dropout(0.5))
    twin = torch.nn.Sequential(torch.nn.BatchNorm1d(8), torch.nn.ReLU(), torch.nn.Dropout(0.5))
    twin.load_state_dict(block.state_dict())
    layer = stag_amd.layers.FeatOnlyLayer(block)
    assert layer.generator is None                                           # random.node_generator
    layer.train(train); twin.train(train)
    x = torch.randn(12, 8)
    before = (srandom.default_generator.offset, srandom.node_generator.offset)
    torch.manual_seed(11)
    got = layer(None, x)
    torch.manual_seed(11)
    ref = twin(x)
    assert torch.equal(got, ref)
    for k, v in twin.state_dict().items():
        assert torch.equal(block.state_dict()[k], v), k
    assert (srandom.default_generator.offset, srandom.node_generator.offset) == before
    plain = stag_amd.layers.FeatOnlyLayer(torch.nn.Linear(8, 4))             # anything else: the module itself
    assert torch.equal(plain(None, x), plain.layer(x))


def test_node_generator_is_a_stream_of_its_own():
    import stag_amd
    from stag_amd import random as srandom
    assert srandom.node_generator is not srandom.default_generator
    assert srandom.NODE_DROP_DOMAIN not in (0, srandom.ATTN_DROP_DOMAIN) and srandom.NODE_DROP_DOMAIN < 1 << 64
    state = (srandom.default_generator.get_state(), srandom.node_generator.get_state())
    try:
        srandom.node_generator.next_offset()
        stag_amd.manual_seed(77)                                             # seeds both, and rewinds both
        assert (srandom.default_generator.seed, srandom.default_generator.offset) == (77, 0)
        assert (srandom.node_generator.seed, srandom.node_generator.offset) == (77, 0)
        srandom.node_generator.next_offset()
        assert srandom.default_generator.offset == 0
    finally:
        srandom.default_generator.set_state(state[0])
        srandom.node_generator.set_state(state[1])


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "node_block_time.py"), doraise=True)
