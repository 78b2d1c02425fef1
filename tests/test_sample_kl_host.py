"""stag_sample_kl (the sample-based KL against a mixture prior, fused) on the host: ABI surface, every refusal before any
device work, the workspace size, and the routing predicate of StagLayer.kl_divergence clause by clause.  Nothing is
dereferenced: a small real indptr, dummy values for device pointers; only refusals are called, because a call that
passes the checks would launch."""
import ctypes as C
import os
import py_compile
import re
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ENOSYS = -22, -12, -38
P = 16      # a non-null, 16-byte aligned dummy "device pointer"

# argument positions of stag_sample_kl
CSR, SPEC, DN, LOGW, MLOC, MSCALE, K_, KL, DP0, DP1, WS, WSB, STREAM = range(13)


def _fixture():
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    csr = _lib.Csr(2, 2, 2, indptr.ctypes.data, P, P, P)       # never dereferenced
    return _lib, _lib.lib(), indptr, csr


def _spec(_lib, **kw):
    s = _lib.NoiseSpec()
    s.kind, s.p0_scalar, s.p1_scalar = _lib.NOISE_NORMAL, 1.0, 0.5
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_header_declares_library_exports_and_lib_binds_both():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    lib = _lib.lib()
    for name in ("stag_sample_kl", "stag_sample_kl_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "#define STAG_KL_MAX_COMPONENTS 8" in header and _lib.KL_MAX_COMPONENTS == 8
    assert lib.stag_sample_kl_workspace_bytes.restype == C.c_size_t
    assert "#define STAG_ABI_VERSION 19" in header and lib.stag_abi_version() == 19          # additive: no bump


def test_header_prototype_matches_the_ctypes_one():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    m = re.search(r"\bint\s+stag_sample_kl\s*\((.*?)\)\s*;", header, re.S)
    assert m
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "csr", "spec", "Dn", "mix_logw", "mix_loc", "mix_scale", "K", "kl_mean", "dp0", "dp1", "workspace",
        "workspace_bytes", "stream"]

    def ctype(p):
        if "*" in p:
            for name, t in (("stag_csr", _lib.Csr), ("stag_noise_spec", _lib.NoiseSpec)):
                if name in p:
                    return C.POINTER(t)
            return C.c_void_p
        return {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t}[p.split()[-2]]
    assert [ctype(p) for p in params] == list(_lib.lib().stag_sample_kl.argtypes)
    assert [C.c_int64, C.c_int32] == list(_lib.lib().stag_sample_kl_workspace_bytes.argtypes)


def _harness():
    _lib, lib, indptr, csr = _fixture()
    good = _spec(_lib)
    nbytes = lib.stag_sample_kl_workspace_bytes(2, 8)
    ok = lambda: [C.byref(csr), C.byref(good), 8, P, P, P, 2, P, P, P, P, nbytes, None]

    def refuses(rc, spec=None, **change):
        a = ok()
        if spec is not None:
            a[SPEC] = C.byref(spec)
        for i, v in change.items():
            a[int(i[1:])] = v
        assert lib.stag_sample_kl(*a) == rc, (change, spec)
    return _lib, lib, indptr, csr, ok, refuses, nbytes


def test_refuses_invalid_arguments():
    _lib, lib, indptr, csr, ok, refuses, nbytes = _harness()
    a = lambda pos, v: {"a%d" % pos: v}
    for k in (0, -1, 9):                                                     # K < 1, K > STAG_KL_MAX_COMPONENTS
        refuses(EINVAL, **a(K_, k))
    for dn in (0, -4):
        refuses(EINVAL, **a(DN, dn))
    empty = _lib.Csr(2, 2, 0, indptr.ctypes.data, None, None, None)
    refuses(EINVAL, **a(CSR, C.byref(empty)))                                # n_edges == 0: no mean
    for pos in (LOGW, MLOC, MSCALE, KL, WS):                                 # a NULL mix_* / kl_mean / workspace
        refuses(EINVAL, **a(pos, None))
    refuses(EINVAL, spec=_spec(_lib, deriv=1))
    refuses(EINVAL, spec=_spec(_lib, deriv=2))
    for pos in (CSR, SPEC):                                                  # what check_csr / check_spec refuse
        refuses(EINVAL, **a(pos, None))
    refuses(EINVAL, spec=_spec(_lib, kind=9))
    refuses(EINVAL, spec=_spec(_lib, param_mode=_lib.PARAM_PER_CHANNEL))     # a row that is not there
    refuses(EINVAL, spec=_spec(_lib, pos_base=-1))
    refuses(EINVAL, spec=_spec(_lib, pos_base=(1 << 44) - 1))
    big = _lib.Csr(2, 2, 1 << 31, indptr.ctypes.data, P, P, P)
    refuses(EINVAL, **a(CSR, C.byref(big)))


def test_leaves_the_composed_route_its_cases():
    _lib, lib, indptr, csr, ok, refuses, nbytes = _harness()
    for kind in (_lib.NOISE_NONE, _lib.NOISE_UNIFORM, _lib.NOISE_BERNOULLI):
        refuses(ENOSYS, spec=_spec(_lib, kind=kind))
    refuses(ENOSYS, spec=_spec(_lib, kind=_lib.NOISE_EXPLICIT, p0=P))
    refuses(ENOSYS, spec=_spec(_lib, in_norm=1))
    refuses(ENOSYS, spec=_spec(_lib, param_mode=_lib.PARAM_PER_EDGE, p0=P, p1=P))
    refuses(ENOSYS, spec=_spec(_lib, param_mode=_lib.PARAM_PER_CHANNEL, p0=P, p1=P, p1_log=1))


def test_short_workspace():
    _lib, lib, indptr, csr, ok, refuses, nbytes = _harness()
    refuses(ENOMEM, **{"a%d" % WSB: nbytes - 1})
    refuses(ENOMEM, **{"a%d" % WSB: 0})
    # the refusals above come before this one
    refuses(EINVAL, **{"a%d" % WSB: 0, "a%d" % K_: 9})
    refuses(ENOSYS, spec=_spec(_lib, in_norm=1), **{"a%d" % WSB: 0})


def test_workspace_bytes_positive_and_monotone():
    from stag_amd import _lib
    f = _lib.lib().stag_sample_kl_workspace_bytes
    edges = (1, 2, 7, 64, 65, 1000, 4096, 100000, 1166243, (1 << 31) - 1)
    widths = (1, 3, 4, 6, 8, 64, 128, 256, 257, 260, 1024)
    for dn in widths:
        sizes = [f(e, dn) for e in edges]
        assert sizes[0] > 0 and sizes == sorted(sizes), (dn, sizes)
    for e in edges:
        sizes = [f(e, dn) for dn in widths]
        assert sizes[0] > 0 and sizes == sorted(sizes), (e, sizes)
    assert f(1000, 8) % 4 == 0
    assert f(1166243, 128) < (1 << 22)             # partials, not a sample: 1.1 MB at the arxiv shape


def _mix(k=2, **kw):
    D = torch.distributions
    return D.MixtureSameFamily(D.Categorical(torch.full((k,), 1.0 / k)),
                               D.Normal(torch.linspace(0.0, 1.0, k), torch.full((k,), 0.5), **kw))


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import EdgeNoise, _lib, ops
    D = torch.distributions
    monkeypatch.setattr(ops, "SAMPLED_KL_FUSED", True)
    why = ops.sampled_kl_why_not
    graph = types.SimpleNamespace(number_of_edges=lambda: 5, device=torch.device("cpu"))
    noise = lambda kind=_lib.NOISE_NORMAL, g=graph, **kw: EdgeNoise(g, 8, kind, 1.0, 0.5, **kw)
    # CPU tensors pass every clause but the device's (checked last, so that the others can be seen here)
    assert why(noise(), _mix()) == "device"
    assert why(noise(relu=True), _mix(8)) == "device"
    assert why(torch.zeros(5, 8), _mix()) == "noise kind"
    assert why(None, _mix()) == "noise kind"
    assert why(noise(_lib.NOISE_UNIFORM), _mix()) == "noise kind"
    assert why(EdgeNoise(graph, 8, _lib.NOISE_BERNOULLI, 0.5), _mix()) == "noise kind"
    assert why(noise(in_norm=True), _mix()) == "in-norm"
    assert why(EdgeNoise(graph, 8, _lib.NOISE_NORMAL, torch.ones(5, 8), torch.ones(5, 8)), _mix()) == "per-edge parameters"
    assert why(EdgeNoise(graph, 8, _lib.NOISE_NORMAL, torch.ones(5, 1), torch.ones(5, 1), p1_log=True), _mix()) == "device"
    n = noise()
    n.n_samples = 3
    assert why(n, _mix()) == "monte-carlo"
    n = noise()
    n.deriv = 1
    assert why(n, _mix()) == "derivative selector"
    shard = types.SimpleNamespace(number_of_edges=lambda: 5, device=torch.device("cpu"), is_shard=True)
    assert why(noise(g=shard), _mix()) == "shard"
    empty = types.SimpleNamespace(number_of_edges=lambda: 0, device=torch.device("cpu"))
    assert why(noise(g=empty), _mix()) == "no edges"
    # the prior: a MixtureSameFamily whose component is a Normal of batch shape [K], K <= 8
    assert why(noise(), D.Normal(1.0, 1.0)) == "prior"
    assert why(noise(), None) == "prior"
    assert why(noise(), _mix(9)) == "prior"
    assert why(noise(), D.MixtureSameFamily(D.Categorical(torch.ones(2)),
                                            D.Uniform(torch.zeros(2), torch.ones(2)))) == "prior"
    assert why(noise(), D.MixtureSameFamily(D.Categorical(torch.ones(3, 2)),
                                            D.Normal(torch.zeros(3, 2), torch.ones(3, 2)))) == "prior"
    assert why(noise(), D.MixtureSameFamily(D.Categorical(torch.ones(2)),
                                            D.Independent(D.Normal(torch.zeros(2, 8), torch.ones(2, 8)), 1))) == "prior"
    meta = types.SimpleNamespace(number_of_edges=lambda: 5, device=torch.device("meta"))
    assert why(noise(g=meta), _mix()) == "prior device"
    live = D.MixtureSameFamily(D.Categorical(torch.ones(2)),
                               D.Normal(torch.zeros(2, requires_grad=True), torch.ones(2)))
    assert why(noise(), live) == "prior gradients"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(noise(), _mix()) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "SAMPLED_KL_FUSED", False)
    assert why(noise(), _mix()) == "switch"


def test_the_layer_keeps_the_composed_route_when_the_predicate_says_so(monkeypatch):
    """The fallback branch of StagLayer._kl_unweighted asks sampled_kl_why_not and otherwise runs the old lines."""
    import stag_amd
    from stag_amd import ops
    asked = []
    monkeypatch.setattr(ops, "sampled_kl_why_not", lambda n, p: asked.append((n, p)) or "switch")
    layer = stag_amd.layers.StagLayer(stag_amd.zoo.GCN(8, 4), q_a=torch.distributions.Normal(1.0, 0.5), p_a=_mix(), vi=True)
    graph = types.SimpleNamespace(number_of_edges=lambda: 5, device=torch.device("cpu"))
    h = stag_amd.EdgeNoise(graph, 8, stag_amd._lib.NOISE_NORMAL, 1.0, 0.5)
    monkeypatch.setattr(h, "materialize", lambda: torch.full((5, 8), 0.75))
    layer._edge_weight_handle = h
    kl = layer.kl_divergence()
    assert asked and asked[0][0] is h and asked[0][1] is layer.p_a
    assert layer._kl_sampled and torch.is_tensor(layer._edge_weight_handle)       # the composed route materialised it
    w = torch.full((5, 8), 0.75)
    ref = layer.q_a.log_prob(w).sum(-1).mean() - layer.p_a.log_prob(w).sum(-1).mean()
    assert torch.allclose(kl, ref)


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "sample_kl_time.py"), doraise=True)


def test_entry_is_documented():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "stag_sample_kl" in open(os.path.join(ROOT, doc)).read(), doc
