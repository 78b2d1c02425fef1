"""reorder_graph on the host: the "custom" relabelling of a CPU graph (structure, keying, frames, helpers), the oracle's
aggregation on the relabelled graph against the one on the original — exactly —, every refusal of the Python entry and
of the C entries (before any device work), and the compiler's resource report of the new unit."""
import ctypes as C
import os
import py_compile
import re
import subprocess

import numpy as np
import pytest
import torch

from util import oracle_graph, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -22, -12
N, E, HUB = 200, 1500, 100


def _pair(seed, noise="original", **kw):
    import stag_amd
    g = random_graph(N, E, seed, hub=HUB)
    perm = torch.from_numpy(np.random.default_rng(seed + 100).permutation(N))
    g2 = stag_amd.reorder_graph(g, "custom", {"nodes_perm": perm}, noise=noise, **kw)
    return g, g2, perm


@pytest.mark.parametrize("seed", [0, 1])
def test_custom_structure_and_keying(seed):
    g, g2, perm = _pair(seed)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    assert torch.equal(g2.node_perm, perm) and torch.equal(g2.node_inv, inv)
    assert g2.node_perm.dtype == torch.int64 and g2.node_inv.dtype == torch.int64
    s, d = g.edges()
    s2, d2 = g2.edges()
    assert torch.equal(s2, inv[s]) and torch.equal(d2, inv[d])                 # the edge list maps through inv, ids kept
    assert g2.number_of_nodes() == N and g2.number_of_edges() == g.number_of_edges()
    pos_of_eid = torch.empty(g.number_of_edges(), dtype=torch.int64)
    pos_of_eid[g.csr.eid.long()] = torch.arange(g.number_of_edges())
    for name in ("csr", "csr_t"):
        v, v0 = getattr(g2, name), getattr(g, name)
        indptr, eid = v.indptr.long(), v.eid.long()
        rows = torch.repeat_interleave(torch.arange(N), indptr[1:] - indptr[:-1])
        same_row = rows[1:] == rows[:-1]
        assert bool((eid[1:][same_row] > eid[:-1][same_row]).all()), name          # ascending edge id inside a row
        assert torch.equal(v.nidx.long(), pos_of_eid[eid]), name                   # the position of the same edge in g.csr
        assert v.nidx.dtype == torch.int32
        # the rows are the original's, moved: row inv[r] of g2 holds the edge ids of row r of g
        r = int(perm[7])
        a, b = int(v0.indptr[r]), int(v0.indptr[r + 1])
        a2, b2 = int(v.indptr[7]), int(v.indptr[8])
        assert torch.equal(v0.eid[a:b], v.eid[a2:b2])
    assert torch.equal(g2.csr_t.nidx.long(), pos_of_eid[g2.csr_t.eid.long()])


@pytest.mark.parametrize("transposed", [False, True])
def test_oracle_rows_are_exactly_the_originals(oracle, transposed):
    """Same draws (nidx), same order (ascending edge id inside a row), fp64 sums: not one bit differs."""
    g, g2, perm = _pair(3)
    x = np.random.default_rng(5).standard_normal((N, 12)).astype(np.float32)
    spec = oracle.make_spec("normal", 1.0, 0.5, seed=77, offset=9, Dn=12, n_edges=g.number_of_edges())
    ref = oracle.agg_fwd(oracle_graph(oracle, g, transposed), x, spec)
    got = oracle.agg_fwd(oracle_graph(oracle, g2, transposed), x[perm.numpy()], spec)
    assert np.array_equal(g2.rows_to_original(torch.from_numpy(got)).numpy(), ref)
    assert np.abs(ref).max() > 0
    own = _pair(3, noise="own")[1]
    other = oracle.agg_fwd(oracle_graph(oracle, own, transposed), x[perm.numpy()], spec)
    assert not np.array_equal(own.rows_to_original(torch.from_numpy(other)).numpy(), ref)   # ... and the keying is why


def test_frames_ids_helpers_and_own_keying():
    import stag_amd
    g = random_graph(N, E, 4, hub=HUB)
    g.ndata["feat"] = torch.randn(N, 5)
    g.ndata["label"] = torch.arange(N)
    g.ndata["other"] = torch.randn(N + 1, 2)              # not a per-node tensor: carried as it is
    g.edata["w"] = torch.randn(g.number_of_edges(), 3)
    perm = torch.randperm(N)
    g2 = stag_amd.reorder_graph(g, "custom", {"nodes_perm": perm}, noise="own")
    assert torch.equal(g2.ndata["feat"], g.ndata["feat"][perm]) and torch.equal(g2.ndata["label"], perm)
    assert g2.ndata["other"] is g.ndata["other"] and g2.edata["w"] is g.edata["w"]
    assert torch.equal(g2.ndata["_ID"], perm)
    assert "_ID" not in stag_amd.reorder_graph(g, "custom", {"nodes_perm": perm}, store_ids=False).ndata
    t = torch.randn(N, 3, requires_grad=True)
    assert torch.equal(g2.rows_to_original(g2.rows_from_original(t)), t)
    assert torch.equal(g2.rows_from_original(g2.rows_to_original(t)), t)
    g2.rows_from_original(t)[0].sum().backward()          # plain indexing: differentiable
    assert float(t.grad[perm[0]].sum()) == 3.0 and float(t.grad.sum()) == 3.0
    assert g2.csr.nidx is None and g2.noise_keying == "own"
    assert torch.equal(g2.csr_t.nidx.long(), _fwd_pos(g2))                    # ... keyed by its own positions
    lv = g2.local_var()
    assert lv.csr is g2.csr and lv.node_perm is g2.node_perm
    with pytest.raises(ValueError):
        g.rows_to_original(t)                              # an ordinary graph has no permutation


def _fwd_pos(g):
    pos = torch.empty(g.number_of_edges(), dtype=torch.int64)
    pos[g.csr.eid.long()] = torch.arange(g.number_of_edges())
    return pos[g.csr_t.eid.long()]


def test_python_refusals():
    import stag_amd
    from stag_amd import _lib
    g = random_graph(N, E, 6)
    ok = torch.randperm(N)
    bad = ok.clone()
    bad[0] = bad[1]
    with pytest.raises(ValueError, match="permutation"):
        stag_amd.reorder_graph(g, "custom", {"nodes_perm": bad})                    # a node twice
    with pytest.raises(ValueError, match="permutation"):
        stag_amd.reorder_graph(g, "custom", {"nodes_perm": ok[:-1]})                # too short
    with pytest.raises(ValueError, match="permutation"):
        stag_amd.reorder_graph(g, "custom", {"nodes_perm": ok + 1})                 # out of range
    with pytest.raises(ValueError, match="node_permute_algo"):
        stag_amd.reorder_graph(g, "rcmk")                                           # an unknown algo
    b = stag_amd.batch([random_graph(20, 50, 1), random_graph(30, 60, 2)])
    with pytest.raises(ValueError, match="batched"):
        stag_amd.reorder_graph(b, "custom", {"nodes_perm": torch.randperm(50)})     # a batched graph
    for keying in ("original", "own"):
        g2 = stag_amd.reorder_graph(g, "custom", {"nodes_perm": ok}, noise=keying)
        with pytest.raises(ValueError, match="reordered"):
            stag_amd.batch([g2, g])                                                 # batch() over a reordered graph
    with pytest.raises(_lib.StagHipError):
        stag_amd.reorder_graph(g, "locality")                                       # "locality" has no CPU path


# argument positions of stag_reorder_locality
CSR, CSR_T, DIMS, ROUNDS, SEED, PERM, INV, WS, WS_BYTES, STREAM = range(10)


def _c_fixture(n=2, e=2):
    from stag_amd import _lib
    indptr = np.array([0, 1, 2], np.int32)
    p = indptr.ctypes.data                                   # host memory standing in for device arrays: never dereferenced
    mk = lambda nd, ns, ne: _lib.Csr(nd, ns, ne, p, p, None, None)
    return _lib, _lib.lib(), indptr, mk, C.c_void_p(256)


def test_c_entry_refusals_without_gpu():
    _lib, lib, _keep, mk, f = _c_fixture()
    csr, csr_t = mk(2, 2, 2), mk(2, 2, 2)
    need = lib.stag_reorder_workspace_bytes(2, 2, 16)
    assert need >= 2 * 2 * 16 * 4

    def args():
        return [C.byref(csr), C.byref(csr_t), 16, 8, 0, f, f, f, need, None]

    call = lambda a: lib.stag_reorder_locality(*a)
    for pos in (CSR, CSR_T, PERM, INV):                                          # NULL arguments
        a = args(); a[pos] = None
        assert call(a) == EINVAL, pos
    for dims in (0, 2, 6, 36, -4):                                               # bad dims
        a = args(); a[DIMS] = dims
        assert call(a) == EINVAL, dims
    a = args(); a[ROUNDS] = -1                                                   # rounds < 0
    assert call(a) == EINVAL
    rect = mk(2, 3, 2)                                                           # n_dst != n_src
    a = args(); a[CSR] = C.byref(rect)
    assert call(a) == EINVAL
    for other in (mk(3, 3, 2), mk(2, 2, 3), mk(2, 3, 2)):                        # a csr_t of other sizes
        a = args(); a[CSR_T] = C.byref(other)
        assert call(a) == EINVAL
    a = args(); a[WS_BYTES] = need - 1                                           # a short workspace
    assert call(a) == ENOMEM
    a = args(); a[WS] = None
    assert call(a) == ENOMEM
    empty = mk(0, 0, 0)                                                          # n == 0
    a = args(); a[CSR] = a[CSR_T] = C.byref(empty); a[WS] = None; a[WS_BYTES] = 0
    assert call(a) == 0
    # stag_relabel_edges
    assert lib.stag_relabel_edges(f, f, -1, f, f, f, None) == EINVAL
    assert lib.stag_relabel_edges(None, None, 0, None, None, None, None) == 0
    for pos in range(5):
        a = [f, f, 3, f, f, f, None]
        a[pos if pos < 2 else pos + 1] = None
        assert lib.stag_relabel_edges(*a) == EINVAL, pos


def test_header_abi_and_exports():
    from stag_amd import _lib
    header = open(os.path.join(ROOT, "include", "stag_hip.h")).read()
    for name in ("stag_reorder_workspace_bytes", "stag_reorder_locality", "stag_relabel_edges"):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(_lib.lib(), name)
    assert "#define STAG_ABI_VERSION 19" in header and _lib.lib().stag_abi_version() == 19


def test_reorder_kernels_use_no_scratch():
    csrc = os.path.join(ROOT, "stag_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(csrc, "_obj", "reorder.remarks")).read()
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S)
    ours = [(n, s) for n, s in found if "reorder_" in n or "relabel_" in n]
    for k in ("reorder_init_kernel", "reorder_smooth_kernel", "reorder_stats1_kernel", "reorder_stats2_kernel",
              "reorder_normalise_kernel", "reorder_keys_kernel", "reorder_inverse_kernel", "relabel_edges_kernel"):
        assert any(k in n for n, _ in ours), k
    assert all(int(s) == 0 for _, s in ours), [n for n, s in ours if int(s)]


def test_timing_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "reorder_time.py"), doraise=True)
