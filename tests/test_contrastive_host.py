"""stag_contrastive_nll (the contrastive NLL of amortised edge noise, fused) on the host: ABI surface, every refusal before
any device work, the workspace size, the routing predicate of models.nll_contrastive clause by clause, and the composed
route on CPU tensors.  Nothing is dereferenced: dummy values for device pointers; only refusals are called, because a
call that passes the checks would launch."""
import ctypes as C
import math
import os
import py_compile
import re
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -22, -12
P = 16      # a non-null, 16-byte aligned dummy "device pointer"
NAMES = ("stag_contrastive_nll", "stag_contrastive_nll_workspace_bytes")

# argument positions of stag_contrastive_nll
(LOC, LS, NE, FSRC, FDST, PS, PD, LDP, HID, WH, BH, POS, NEG, NLL, DLOC, DLS, DPRE, DWH, DBH, WS, WSB, STREAM) = range(22)


def test_header_declares_library_exports_and_lib_binds_both():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.stag_contrastive_nll_workspace_bytes.restype == C.c_size_t
    assert "#define STAG_ABI_VERSION 19" in header and lib.stag_abi_version() == 19          # additive: no bump


def test_header_prototype_matches_the_ctypes_one():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    m = re.search(r"\bint\s+stag_contrastive_nll\s*\((.*?)\)\s*;", header, re.S)
    assert m
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "loc", "log_scale", "n_edges", "fake_src", "fake_dst", "ps", "pd", "ldp", "hidden", "wh", "bh", "pos_value",
        "neg_value", "nll_mean", "dloc", "dlog_scale", "dpre", "dwh", "dbh", "workspace", "workspace_bytes", "stream"]

    def ctype(p):
        if "*" in p:
            return C.c_void_p
        return {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float}[p.split()[-2]]
    assert [ctype(p) for p in params] == list(_lib.lib().stag_contrastive_nll.argtypes)
    m = re.search(r"\bsize_t\s+stag_contrastive_nll_workspace_bytes\s*\((.*?)\)\s*;", header, re.S)
    assert m and " ".join(m.group(1).split()) == "int32_t hidden"
    assert [C.c_int32] == list(_lib.lib().stag_contrastive_nll_workspace_bytes.argtypes)


def _harness(hidden=2):
    from stag_amd import _lib
    lib = _lib.lib()
    nbytes = lib.stag_contrastive_nll_workspace_bytes(hidden)
    ok = lambda: [P, P, 5, P, P, P, P, 2 * hidden, hidden, P, P, 1.0, 0.0, P, P, P, P, P, P, P, nbytes, None]

    def refuses(rc, **change):
        a = ok()
        for i, v in change.items():
            a[int(i[1:])] = v
        assert lib.stag_contrastive_nll(*a) == rc, change
    return lib, refuses, nbytes


def _a(pos, v):
    return {"a%d" % pos: v}


def test_refuses_invalid_arguments():
    lib, refuses, nbytes = _harness()
    for n in (0, -1):
        refuses(EINVAL, **_a(NE, n))
    for h in (0, -1, 9):
        refuses(EINVAL, **_a(HID, h))
    refuses(EINVAL, **_a(LDP, 1))                        # ldp < hidden
    refuses(EINVAL, **_a(LDP, 1 << 30))
    refuses(EINVAL, **_a(LDP, 1 << 40))
    for pos in (LOC, LS, FSRC, FDST, PS, PD, WH, NLL):
        refuses(EINVAL, **_a(pos, None))


def test_short_or_missing_workspace():
    for hidden in (1, 2, 3, 8):
        lib, refuses, nbytes = _harness(hidden)
        assert nbytes > 0
        refuses(ENOMEM, **_a(WSB, nbytes - 1))
        refuses(ENOMEM, **_a(WSB, 0))
        refuses(ENOMEM, **_a(WS, None))
        # with every gradient NULL as well
        refuses(ENOMEM, **{**_a(WSB, nbytes - 1), **{"a%d" % p: None for p in (DLOC, DLS, DPRE, DWH, DBH, BH)}})
        # the argument refusals come first
        refuses(EINVAL, **{**_a(WSB, 0), **_a(NE, 0)})
        refuses(EINVAL, **{**_a(WS, None), **_a(LOC, None)})


def test_workspace_bytes_do_not_decrease_with_hidden():
    from stag_amd import _lib
    f = _lib.lib().stag_contrastive_nll_workspace_bytes
    sizes = [f(h) for h in range(1, 9)]
    assert sizes[0] > 0 and sizes == sorted(sizes), sizes
    assert all(s % 4 == 0 for s in sizes) and sizes[-1] < (1 << 16)          # block partials: tens of kilobytes


def _stub_q(E=5, in_features=3, hidden=None, **kw):
    from stag_amd.distributions import AmortizedDistribution
    q = AmortizedDistribution(in_features, 1, hidden_features=hidden, **kw)
    q.new_parameters = {k: torch.zeros(E, 1) for k in q.new_parameter_names}
    return q


def test_routing_predicate_clause_by_clause(monkeypatch):
    from stag_amd import ops
    monkeypatch.setattr(ops, "CONTRASTIVE_FUSED", True)
    why = ops.contrastive_why_not
    cpu = torch.device("cpu")
    graph = types.SimpleNamespace(number_of_edges=lambda: 5, _src=None)
    # a stand-in for device features: the predicate reads is_cuda, dim() and device only
    feat = types.SimpleNamespace(is_cuda=True, dim=lambda: 2, device=cpu, shape=(4, 3))
    assert why(_stub_q(), graph, feat) is None
    assert why(_stub_q(hidden=ops.NARROW_MAX_HIDDEN), graph, feat) is None
    assert why(_stub_q(), graph, torch.zeros(4, 3)) == "features"                       # a CPU tensor
    assert why(_stub_q(), graph, types.SimpleNamespace(is_cuda=True, dim=lambda: 3, device=cpu)) == "features"
    q = _stub_q()
    q.embedding_mlp = torch.nn.Sequential(torch.nn.Identity(), torch.nn.SiLU())
    assert why(q, graph, feat) == "not narrow"
    assert why(_stub_q(activation=torch.nn.ReLU()), graph, feat) == "not narrow"
    assert why(_stub_q(hidden=ops.NARROW_MAX_HIDDEN + 1), graph, feat) == "not narrow"
    from stag_amd.distributions import AmortizedDistribution
    wide = AmortizedDistribution(3, 4)
    wide.new_parameters = {k: torch.zeros(5, 4) for k in wide.new_parameter_names}
    assert why(wide, graph, feat) == "not narrow"
    assert why(_stub_q(), types.SimpleNamespace(number_of_edges=lambda: 5), feat) == "not narrow"     # no edge list
    class Uniform(torch.distributions.Uniform):        # (torch's own keeps its constraints in a property)
        arg_constraints = {"low": torch.distributions.constraints.real, "high": torch.distributions.constraints.real}
    assert why(_stub_q(base_distribution_class=Uniform), graph, feat) == "base distribution"
    assert why(_stub_q(base_distribution_class=torch.distributions.Laplace), graph, feat) == "base distribution"
    q = _stub_q()
    q.new_parameters = None
    assert why(q, graph, feat) == "parameters"                                          # condition() has not run
    assert why(_stub_q(E=4), graph, feat) == "parameters"                               # another graph's edges
    q = _stub_q()
    q.new_parameters["loc"] = torch.zeros(5)
    assert why(q, graph, feat) == "parameters"
    q = _stub_q()
    q.new_parameters["loc"] = torch.zeros(5, 1, device="meta")
    assert why(q, graph, feat) == "parameters"
    shard = types.SimpleNamespace(number_of_edges=lambda: 5, _src=None, is_shard=True)
    assert why(_stub_q(), shard, feat) == "shard"
    empty = types.SimpleNamespace(number_of_edges=lambda: 0, _src=None)
    assert why(_stub_q(E=0), empty, feat) == "no edges"
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert why(_stub_q(), graph, feat) == "compiling"
    monkeypatch.undo()
    monkeypatch.setattr(ops, "CONTRASTIVE_FUSED", False)
    assert why(_stub_q(), graph, feat) == "switch"


def _cpu_case(seed=0, N=12, E=40, in_features=6, hidden=3):
    import stag_amd
    gen = torch.Generator().manual_seed(seed)
    g = stag_amd.Graph(torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen), N)
    feat = torch.randn(N, in_features, generator=gen)
    torch.manual_seed(seed)
    q = stag_amd.distributions.AmortizedDistribution(in_features, 1, hidden_features=hidden)
    q.condition(g, feat)
    return q, g, feat


def _hand_formula(q, g, feat, fake_src, fake_dst):
    d = torch.float64
    lin = q.embedding_mlp[0]
    x = torch.cat([feat[fake_src], feat[fake_dst]], -1).to(d)
    h = torch.nn.functional.silu(x @ lin.weight.to(d).t() + lin.bias.to(d))
    nlp = lambda v, m, l: 0.5 * ((v - m) * torch.exp(-l)) ** 2 + l + 0.5 * math.log(2 * math.pi)
    mf = h @ q.parameters_mlp["loc"].weight.to(d).t() + q.parameters_mlp["loc"].bias.to(d)
    lf = h @ q.parameters_mlp["log_scale"].weight.to(d).t() + q.parameters_mlp["log_scale"].bias.to(d)
    t = nlp(1.0, q.new_parameters["loc"].to(d), q.new_parameters["log_scale"].to(d)) + nlp(0.0, mf, lf)
    return t.sum(-1).mean()


def test_cpu_tensors_take_the_composed_route_and_equal_the_hand_formula(monkeypatch):
    from stag_amd import models, ops

    def never(*a, **k):
        raise AssertionError("the fused route was entered on CPU tensors")
    monkeypatch.setattr(ops, "contrastive_nll", never)
    q, g, feat = _cpu_case()
    assert ops.contrastive_why_not(q, g, feat) == "features"
    torch.manual_seed(11)
    got = models.nll_contrastive(q, g, feat)
    torch.manual_seed(11)
    fs = torch.randint(high=12, size=[40])
    fd = torch.randint(high=12, size=[40])
    ref = _hand_formula(q, g, feat, fs, fd)
    assert got.dim() == 0 and abs(float(got.detach()) - float(ref.detach())) <= 1e-5 * (1 + abs(float(ref.detach())))


def test_switch_off_never_enters_the_fused_function(monkeypatch):
    from stag_amd import models, ops

    def never(*a, **k):
        raise AssertionError("the fused route was entered with the switch off")
    monkeypatch.setattr(ops, "CONTRASTIVE_FUSED", False)
    monkeypatch.setattr(ops, "contrastive_nll", never)
    monkeypatch.setattr(ops, "_ContrastiveNll", None)
    q, g, feat = _cpu_case(1)
    assert ops.contrastive_why_not(q, g, feat) == "switch"
    torch.manual_seed(5)
    got = models.nll_contrastive(q, g, feat)
    torch.manual_seed(5)
    fs = torch.randint(high=12, size=[40])
    fd = torch.randint(high=12, size=[40])
    ref = _hand_formula(q, g, feat, fs, fd)
    assert abs(float(got.detach()) - float(ref.detach())) <= 1e-5 * (1 + abs(float(ref.detach())))


def test_fused_route_gets_the_fake_edges_the_composed_route_would_draw(monkeypatch):
    """When the predicate says yes, nll_contrastive hands over the result of the same two randint calls, in order."""
    from stag_amd import models, ops
    seen = []
    monkeypatch.setattr(ops, "contrastive_why_not", lambda q, g, f: None)
    monkeypatch.setattr(ops, "contrastive_nll", lambda q, g, f, fs, fd: seen.append((fs, fd)) or torch.tensor(2.5))
    q, g, feat = _cpu_case(2)
    torch.manual_seed(9)
    assert float(models.nll_contrastive(q, g, feat)) == 2.5
    after = torch.get_rng_state()
    torch.manual_seed(9)
    fs = torch.randint(high=12, size=[40])
    fd = torch.randint(high=12, size=[40])
    assert torch.equal(seen[0][0], fs) and torch.equal(seen[0][1], fd)
    assert torch.equal(after, torch.get_rng_state())


def test_condition_uses_the_lifted_tables():
    from stag_amd.distributions import AmortizedDistribution
    import inspect
    assert "_narrow_tables(feat)" in inspect.getsource(AmortizedDistribution.condition)


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "contrastive_time.py"), doraise=True)


def test_entry_is_documented():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "stag_contrastive_nll" in open(os.path.join(ROOT, doc)).read(), doc
