"""The fused likelihood head (stag_nll_categorical_fwd / _bwd, stag_nll_bernoulli_fwd / _bwd: the masked mean NLL of
model.loss) on the host: ABI surface, every refusal before any device work and in the stated order, the compiler's resource
report of the new kernels, the routing predicate clause by clause, the numpy references of tests/nll_cases.py against
torch's own distributions, the condition on the device tests' inputs, and the timing tool."""
import ctypes as C
import os
import py_compile
import re
import subprocess

import numpy as np
import pytest
import torch

import nll_cases as cases
from util import TOL, scaled_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ENOSYS = -22, -12, -38

PROTOTYPES = {
    "size_t stag_nll_workspace_bytes": ("int64_t n_rows, int32_t C", "q i"),
    "int stag_nll_categorical_fwd": (
        "const float* probs, int64_t ldp, int64_t n_rows, int32_t C, const int64_t* y, const uint8_t* mask, float* value, "
        "float* denom, void* workspace, size_t workspace_bytes, void* stream",
        "p q q i p p p p p z p"),
    "int stag_nll_categorical_bwd": (
        "const float* probs, int64_t ldp, int64_t n_rows, int32_t C, const int64_t* y, const uint8_t* mask, "
        "const float* g, const float* denom, float* dprobs, int64_t lddp, void* stream",
        "p q q i p p p p p q p"),
    "int stag_nll_bernoulli_fwd": (
        "const float* probs, int64_t ldp, const float* y, int64_t ldy, int64_t n_rows, int32_t C, const uint8_t* mask, "
        "float* value, float* denom, void* workspace, size_t workspace_bytes, void* stream",
        "p q p q q i p p p p z p"),
    "int stag_nll_bernoulli_bwd": (
        "const float* probs, int64_t ldp, const float* y, int64_t ldy, int64_t n_rows, int32_t C, const uint8_t* mask, "
        "const float* g, const float* denom, float* dprobs, int64_t lddp, void* stream",
        "p q p q q i p p p p q p"),
}


def test_header_prototypes_match_the_ctypes_ones_and_the_abi_is_kept():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    kinds = {"p": C.c_void_p, "q": C.c_int64, "i": C.c_int32, "z": C.c_size_t}
    first = None
    for decl, (args, ctypes_args) in PROTOTYPES.items():
        name = decl.split()[-1]
        m = re.search(re.escape(decl) + r"\s*\(([^;]*)\);", header)
        assert m, decl
        first = m.start() if first is None else min(first, m.start())
        plain = re.sub(r"/\*.*?\*/", "", m.group(1))                         # (the prototypes carry comments)
        assert re.sub(r"\s+", " ", plain).replace(" ,", ",").strip() == args, name
        fn = getattr(_lib.lib(), name)
        want = [kinds[k] for k in ctypes_args.split()]
        assert list(fn.argtypes) == want, name
        assert len(want) == args.count(",") + 1
    assert _lib.lib().stag_nll_workspace_bytes.restype is C.c_size_t
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19      # additive
    para = header[:first].rsplit("/* ----", 1)[1]
    for word in ("eps = 2^-23", "[eps <= q <= 1 - eps]", "log1p", "count == 0", "NaN", "device-asserts", "slab order",
                 "No atomics", "butterfly", "16-byte", "hipGraph", "STAG_EINVAL", "STAG_ENOSYS", "STAG_ENOMEM",
                 "n_rows == 0"):
        assert word in para, word


def _lib_and_f():
    from stag_amd import _lib
    return _lib, _lib.lib(), C.c_void_p(16)     # f: a non-null, 16-byte aligned dummy "device pointer"


BIG = 1 << 30      # "enough" workspace bytes
# argument positions
CF = dict(p=0, ldp=1, n=2, C=3, y=4, mask=5, value=6, denom=7, ws=8, wsb=9)
CB = dict(p=0, ldp=1, n=2, C=3, y=4, mask=5, g=6, denom=7, dp=8, lddp=9)
BF = dict(p=0, ldp=1, y=2, ldy=3, n=4, C=5, mask=6, value=7, denom=8, ws=9, wsb=10)
BB = dict(p=0, ldp=1, y=2, ldy=3, n=4, C=5, mask=6, g=7, denom=8, dp=9, lddp=10)


def _entries(lib, f):
    """(name, call, positions, a good argument list) of the four entry points"""
    return [
        ("categorical_fwd", lib.stag_nll_categorical_fwd, CF, lambda: [f, 8, 100, 8, f, f, f, f, f, BIG, None]),
        ("categorical_bwd", lib.stag_nll_categorical_bwd, CB, lambda: [f, 8, 100, 8, f, f, f, f, f, 8, None]),
        ("bernoulli_fwd", lib.stag_nll_bernoulli_fwd, BF, lambda: [f, 8, f, 8, 100, 8, f, f, f, f, BIG, None]),
        ("bernoulli_bwd", lib.stag_nll_bernoulli_bwd, BB, lambda: [f, 8, f, 8, 100, 8, f, f, f, f, 8, None]),
    ]


def test_workspace_bytes_is_a_function_of_the_rows_alone():
    _lib, lib, _f = _lib_and_f()
    ws = lib.stag_nll_workspace_bytes
    assert ws(0, 8) == 0 and ws(8, 0) == 0 and ws(-1, 8) == 0
    # one (sum, count) per slab; 64-row slabs up to 131,072 rows, then at most 2048 slabs
    assert ws(1, 8) == 8 and ws(64, 8) == 8 and ws(65, 8) == 16 and ws(65, 1000) == 16
    assert ws(131072, 40) == 2048 * 8 and ws(131073, 40) == 1025 * 8 and ws(169343, 40) == 1323 * 8


def test_every_entry_refuses_in_order_without_gpu():
    _lib, lib, f = _lib_and_f()
    for name, call, P, ok in _entries(lib, f):
        fwd = "ws" in P
        strides = [k for k in ("ldp", "ldy", "lddp") if k in P]
        for key, bad in [("C", 0), ("C", -4), ("n", -1)] + [(k, 7) for k in strides] + [(k, 0) for k in strides]:
            a = ok(); a[P[key]] = bad
            assert call(*a) == EINVAL, (name, key, bad)
        required = [k for k in ("p", "y", "value", "denom", "g", "dp", "ws") if k in P]
        for key in required:                                                # a NULL required pointer with rows
            a = ok(); a[P[key]] = None
            assert call(*a) == EINVAL, (name, key)
        a = ok(); a[P["mask"]] = None                                       # no mask: every row (nothing to refuse:
        a[P["n"]] = (1 << 34) + 1                                           #  the next refusal is reached)
        assert call(*a) == ENOSYS, name
        # what the entry has no form for comes before the workspace, an invalid argument before both
        a = ok(); a[P["n"]] = (1 << 34) + 1
        if fwd:
            a[P["wsb"]] = 0
        assert call(*a) == ENOSYS, name
        a[P["p"]] = None
        assert call(*a) == EINVAL, name
        a = ok(); a[P["C"]] = (1 << 30) + 1
        for k in strides:
            a[P[k]] = (1 << 30) + 1
        if fwd:
            a[P["wsb"]] = 0
        assert call(*a) == ENOSYS, name
        a[P["ldp"]] = 1 << 30                                               # a stride below C: invalid comes first
        assert call(*a) == EINVAL, name
        if fwd:
            need = lib.stag_nll_workspace_bytes(100, 8)
            assert need == 16
            a = ok(); a[P["wsb"]] = need - 1
            assert call(*a) == ENOMEM, name
            a[P["wsb"]] = 0
            assert call(*a) == ENOMEM, name
            a[P["ws"]] = None                                               # the NULL workspace is the earlier refusal
            assert call(*a) == EINVAL, name
        # no rows: nothing to do, whatever the pointers, but the shape is still checked
        a = ok(); a[P["n"]] = 0
        for key in required + ["mask"]:
            a[P[key]] = None
        if fwd:
            a[P["wsb"]] = 0
        assert call(*a) == 0, name
        a[P["ldp"]] = 7
        assert call(*a) == EINVAL, name
        a[P["ldp"]] = 8; a[P["C"]] = 0
        assert call(*a) == EINVAL, name


def test_every_refusal_comes_before_the_launch():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "nll.hip")).read()
    for entry, launch in (("int nll_fwd(", "nll_fwd_launch("), ("int nll_bwd(", "nll_bwd_launch(")):
        body = src[src.index("\n" + entry):]
        body = body[:body.index("\n}\n") + 3]
        at = body.index(launch)
        assert "return STAG_E" not in body[at:].replace("STAG_EIO", "")
        assert "hipLaunchKernelGGL" not in body and "hipMemset" not in body and "hipMemcpy" not in body
    for name in ("categorical_fwd", "categorical_bwd", "bernoulli_fwd", "bernoulli_bwd"):   # the C entries only forward
        body = src[src.index('extern "C" int stag_nll_' + name + "("):]
        body = body[body.index("{"):body.index("\n}\n")]
        assert body.count(";") == 1 and ("return nll_fwd(" in body or "return nll_bwd(" in body), name
    code = src.split("#include", 1)[1].lower()                                 # (the header comment says "No atomics")
    assert "atomic" not in code and "hipmemcpy" not in code and "synchronize" not in code


def test_nll_kernels_use_no_scratch():
    """Every instantiation of the kernels of nll.hip keeps its state in registers: 0 scratch bytes."""
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "nll.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    names = [n for n, _ in found]
    for kernel in ("nll_cat_fwd_kernel", "nll_bern_fwd_kernel", "nll_cat_bwd_kernel", "nll_bern_bwd_kernel"):
        assert sum(kernel in n for n in names) == 7, kernel                # lanes per row: 64, 32, 16, 8, 4, 2, 1
    assert sum("nll_merge_kernel" in n for n in names) == 1
    assert len(found) == 29
    assert all(int(s) == 0 for _, s in found), [n for n, s in found if int(s)]


# ---- the routing predicate -------------------------------------------------------------------------------------------
class _OnDevice:
    """A stand-in that passes the device clause (no device is present here)."""

    def __init__(self, t):
        self.t = t
        self.is_cuda = True

    def __getattr__(self, k):
        return getattr(self.t, k)


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import likelihoods, ops
    monkeypatch.setattr(ops, "NLL_FUSED", True)
    monkeypatch.setattr(likelihoods, "VALIDATE_ON_DEVICE", False)
    why = ops.nll_why_not
    cat, bern = likelihoods.CategoricalLikelihood(), likelihoods.BernoulliLikelihood()
    cpu = torch.rand(6, 8)
    p = _OnDevice(cpu)
    y = torch.zeros(6, dtype=torch.int64)
    t = torch.zeros(6, 8)
    mask = torch.zeros(6, dtype=torch.bool)
    assert why(cat, p, y) is None and why(cat, p, y, mask) is None and why(cat, p, y, None) is None
    assert why(bern, p, t) is None and why(bern, p, t, mask) is None
    wide = _OnDevice(torch.rand(6, 12)[:, :8])                                  # a column slice: ldp > C
    assert why(cat, wide, y) is None and why(bern, wide, torch.zeros(6, 12)[:, 2:10]) is None

    class MyCat(likelihoods.CategoricalLikelihood):      # a subclass may compute anything: exactly the two classes
        pass

    class Other(likelihoods.Likelihood):
        def condition(self, feat):
            return torch.distributions.Categorical(probs=feat)

    swapped = likelihoods.CategoricalLikelihood()
    swapped.distribution = torch.distributions.OneHotCategorical
    for other in (MyCat(), Other(torch.distributions.Categorical), swapped, torch.nn.Identity(), None):
        assert why(other, p, y) == "likelihood", other
    monkeypatch.setattr(likelihoods, "VALIDATE_ON_DEVICE", True)
    assert why(cat, p, y) == "validating" and why(MyCat(), p, y) == "likelihood"
    monkeypatch.setattr(likelihoods, "VALIDATE_ON_DEVICE", False)
    assert why(cat, cpu, y) == "device" and why(cat, torch.zeros(6, 8, device="meta"), y) == "device"
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        assert why(cat, _OnDevice(cpu.to(dt)), y) == "dtype"
    assert why(cat, _OnDevice(torch.zeros(2, 3, 8)), y) == "shape" and why(cat, _OnDevice(torch.zeros(8)), y) == "shape"
    assert why(cat, _OnDevice(cpu[:0]), y[:0]) == "shape"                      # N == 0: the mean of nothing is torch's
    assert why(cat, _OnDevice(torch.rand(8, 6).t()), y) == "stride"            # a transposed view
    assert why(cat, _OnDevice(torch.rand(6, 16)[:, ::2]), y) == "stride"
    assert why(cat, _OnDevice(torch.rand(1, 8).expand(6, 8)), y) == "stride"   # stride(0) == 0 < C
    # categorical labels: int64 [N] on feat's device
    for bad in (y.int(), y.float(), y[:5], y.view(6, 1), torch.zeros(6, dtype=torch.int64, device="meta"), [0] * 6):
        assert why(cat, p, bad) == "labels", bad
    # Bernoulli targets: fp32 of feat's shape with unit column stride
    for bad in (t.double(), t.long(), t[:, :7], torch.zeros(8, 6).t(), torch.zeros(6, 16)[:, ::2], t[0],
                torch.zeros(6, 8, device="meta"), y):
        assert why(bern, p, bad) == "labels", bad
    assert why(bern, p, torch.zeros(6, 12)[:, :8]) is None
    # the mask: None or bool [N] (on any device)
    for bad in (mask.long(), mask.float(), mask[:5], mask.view(6, 1), torch.tensor([0, 2]), [True] * 6):
        assert why(cat, p, y, bad) == "mask", bad
        assert why(bern, p, t, bad) == "mask", bad
    assert why(bern, p, t.clone().requires_grad_(True)) == "label gradient"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(cat, p, y) == "compiling" and why(cat, cpu, y) == "device"      # (the earlier clauses come first)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: False)
    monkeypatch.setattr(ops, "NLL_FUSED", False)
    assert why(cat, p, y) == "switch" and why(None, cpu, None) == "switch"
    with pytest.raises(ValueError, match="no fused form"):                     # nll_mean itself never falls back
        ops.nll_mean(cat, cpu, y)


def test_functions_save_nothing_row_sized_and_refuse_a_double_backward():
    import inspect
    from stag_amd import ops
    for fn in (ops._CategoricalNll, ops._BernoulliNll):
        src = inspect.getsource(fn)
        assert "once_differentiable" in src
        assert src.count("save_for_backward") == 1 and "ctx.save_for_backward(probs, y, mask, out)" in src
        assert ".item()" not in src and ".cpu()" not in src and "synchronize" not in src


# ---- the references --------------------------------------------------------------------------------------------------
def _torch_value_and_grad(kind, p, y, mask, dtype):
    from stag_amd import likelihoods
    from stag_amd.models import _masked_mean
    lk = likelihoods.CategoricalLikelihood() if kind == "categorical" else likelihoods.BernoulliLikelihood()
    pt = torch.tensor(np.asarray(p), dtype=dtype, requires_grad=True)
    yt = torch.tensor(np.asarray(y)) if kind == "categorical" else torch.tensor(np.asarray(y), dtype=dtype)
    mt = None if mask is None else torch.tensor(np.asarray(mask))
    value = _masked_mean(-lk.log_prob(pt, yt), mt)
    (0.25 * value).backward()
    return value.item(), pt.grad.numpy()


HOST_CASES = [(1000, 2, "half"), (63, 3, "all"), (1000, 7, "single"), (4099, 40, "half"),
              (1000, 41, "ends"), (63, 65, "one_slab"), (65, 256, "none"), (1, 257, "all"), (2, 1000, "ends")]


@pytest.mark.parametrize("n,C,kind", HOST_CASES)
def test_categorical_reference_is_torchs_in_float64(n, C, kind):
    """Away from the clamp (float64 torch clamps at its own eps; C = 1 sits on it and is a float32 case below) the closed
    form is torch's Categorical + _masked_mean."""
    p, y, mask, value, d = cases.categorical_case(n, C, kind)
    tv, tg = _torch_value_and_grad("categorical", p, y, mask, torch.float64)
    assert abs(value - tv) <= 1e-13 * (1 + abs(tv))
    assert scaled_err(0.25 * d, tg) <= 1e-12


@pytest.mark.parametrize("n,C,kind", [(1000, 1, "half"), (63, 5, "all"), (65, 121, "one_slab"), (64, 260, "none"),
                                      (4099, 121, "half")])
def test_bernoulli_reference_is_torchs_in_float64(n, C, kind):
    p, y, mask, value, d = cases.bernoulli_case(n, C, kind)
    tv, tg = _torch_value_and_grad("bernoulli", p, y, mask, torch.float64)
    assert abs(value - tv) <= 1e-13 * (1 + abs(tv))
    assert scaled_err(0.25 * d, tg) <= 1e-12


def test_clamp_edges_of_the_reference_are_torchs_in_float32():
    """At the clamp torch's float32 arithmetic is the contract (eps = 2^-23): value and window, row by row."""
    p, y, inside = cases.edge_categorical()
    for r in range(len(y)):
        mask = np.zeros(len(y), bool); mask[r] = True
        value, d = cases.categorical_ref(p, y, mask)
        v32, d32 = cases.categorical_ref(p, y, mask, dtype=np.float32)
        tv, tg = _torch_value_and_grad("categorical", p, y, mask, torch.float32)
        assert abs(value - tv) <= TOL * (1 + abs(tv)) and abs(v32 - value) <= TOL * (1 + abs(value)), r
        assert scaled_err(0.25 * d, tg) <= TOL and scaled_err(d32, d) <= TOL, r
        assert bool(np.any(d[r] != 0)) == bool(inside[r]) == bool(np.any(d32[r] != 0)), r
        assert not np.any(np.delete(d, r, 0))
    value, _ = cases.categorical_ref(p, y, np.arange(len(y)) == 0)
    assert value == -np.log(cases.EPS)                                       # p_y = 0
    value, _ = cases.categorical_ref(p, y, np.arange(len(y)) == 1)
    assert value == -np.log(1 - cases.EPS)                                   # one-hot
    p, t = cases.edge_bernoulli()
    value, d = cases.bernoulli_ref(p, t)
    tv, tg = _torch_value_and_grad("bernoulli", p, t, None, torch.float32)
    assert abs(value - tv) <= TOL * (1 + abs(tv))
    assert scaled_err(0.25 * d, tg) <= TOL
    assert not d[:, :2].any() and d[:, 2:].all()                              # p = 0, 1: clamped; eps, 1 - eps: inside


def test_reference_edges_nan_and_bad_labels():
    p, y = cases.categorical_inputs(200, 7)
    y = y.copy(); y[70] = -1; y[71] = 7
    mask = np.ones(200, bool)
    value, d = cases.categorical_ref(p, y, mask)
    assert np.isnan(value) and not d[70:72].any() and np.isfinite(d).all() and d[:70].all()
    mask[70:72] = False
    value, d2 = cases.categorical_ref(p, y, mask)
    assert np.isfinite(value)
    value, d = cases.categorical_ref(p, y, np.zeros(200, bool))
    assert np.isnan(value) and not d.any()
    value, d = cases.bernoulli_ref(*cases.bernoulli_inputs(10, 5), np.zeros(10, bool))
    assert np.isnan(value) and not d.any()
    q = p.copy(); q[3, 2] = np.nan
    assert np.isnan(cases.categorical_ref(q, np.clip(y, 0, 6), None)[0])
    m = np.ones(200, bool); m[3] = False
    assert np.isfinite(cases.categorical_ref(q, np.clip(y, 0, 6), m)[0])


@pytest.mark.parametrize("n,C,kind", cases.cat_case_list())
def test_categorical_inputs_are_inside_the_bar_in_float32(n, C, kind):
    """The condition on the device tests' inputs: a float32 evaluation of the formulas meets the bar the device is held
    to, for the value, the gradient, and the gradient of the row sum (count x the gradient)."""
    p, y, mask, value, d = cases.categorical_case(n, C, kind)
    v32, d32 = cases.categorical_ref(p, y, mask, dtype=np.float32)
    count = cases.count_of(mask, n)
    if count == 0:
        assert np.isnan(value) and np.isnan(v32) and not d.any() and not d32.any()
        return
    assert abs(float(v32) - value) <= TOL * (1 + abs(value))
    assert scaled_err(d32, d) <= TOL and scaled_err(d32.astype(np.float64) * count, d * count) <= TOL
    if C > 1:
        assert d[mask if mask is not None else slice(None)].all()            # away from the clamp: every row has a gradient


@pytest.mark.parametrize("n,C,kind", cases.bern_case_list())
def test_bernoulli_inputs_are_inside_the_bar_in_float32(n, C, kind):
    p, y, mask, value, d = cases.bernoulli_case(n, C, kind)
    v32, d32 = cases.bernoulli_ref(p, y, mask, dtype=np.float32)
    count = cases.count_of(mask, n)
    if count == 0:
        assert np.isnan(value) and np.isnan(v32) and not d.any() and not d32.any()
        return
    assert abs(float(v32) - value) <= TOL * (1 + abs(value))
    assert scaled_err(d32, d) <= TOL and scaled_err(d32.astype(np.float64) * count * C, d * count * C) <= TOL


def test_case_lists_cover_the_shapes_the_kernels_branch_on():
    cat = cases.cat_case_list()
    assert {C for _, C, _ in cat} == {1, 2, 3, 7, 40, 41, 64, 65, 121, 256, 257, 1000}
    assert {n for n, _, _ in cat} == {1, 2, 63, 64, 65, 1000, 4099}
    assert {k for _, _, k in cat} == set(cases.MASKS)
    bern = cases.bern_case_list()
    assert {C for _, C, _ in bern} == {1, 5, 121, 260} and {n for n, _, _ in bern} == {1, 2, 63, 64, 65, 1000, 4099}
    assert {k for _, _, k in bern} == set(cases.MASKS)


# ---- through the model -----------------------------------------------------------------------------------------------
def test_a_subclass_that_overrides_log_prob_takes_the_composed_route(monkeypatch):
    """model.loss on a likelihood whose log_prob is its own: mean_nll is the base's composed expression, and the fused
    entry is never asked for (it would raise here: there is no device)."""
    from stag_amd import likelihoods, models, ops
    monkeypatch.setattr(ops, "NLL_FUSED", True)
    calls = []
    monkeypatch.setattr(ops, "nll_mean", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError("fused")))

    class Tempered(likelihoods.CategoricalLikelihood):
        def log_prob(self, feat, y):
            return 0.5 * super().log_prob(feat, y)

    class Layer(torch.nn.Module):
        vi = False

        def forward(self, graph, feat):
            return torch.softmax(feat, -1)

    class G:
        def local_var(self):
            return self

    torch.manual_seed(0)
    x = torch.randn(9, 4, requires_grad=True)
    y = torch.randint(0, 4, (9,))
    mask = torch.rand(9) < 0.6
    for lk in (Tempered(), likelihoods.CategoricalLikelihood()):
        model = models.StagModel([Layer()], likelihood=lk)
        got = model.loss(G(), x, y, mask=mask)
        scale = 0.5 if isinstance(lk, Tempered) else 1.0
        ref = -(scale * torch.distributions.Categorical(probs=torch.softmax(x, -1)).log_prob(y))[mask].mean()
        assert torch.equal(got, ref)
    assert calls == []
    assert ops.nll_why_not(Tempered(), _OnDevice(x.detach()), y, mask) == "likelihood"

    class Legacy(torch.nn.Module):                   # a likelihood object from before mean_nll: the two lines still run
        def log_prob(self, feat, y):
            return torch.distributions.Categorical(probs=feat).log_prob(y)

    model = models.StagModel([Layer()], likelihood=likelihoods.CategoricalLikelihood())
    model.likelihood = Legacy()
    assert torch.equal(model.loss(G(), x, y, mask=mask),
                       -torch.distributions.Categorical(probs=torch.softmax(x, -1)).log_prob(y)[mask].mean())


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "loss_head_time.py"), doraise=True)
