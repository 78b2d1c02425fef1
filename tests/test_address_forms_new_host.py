"""The shapes of tests/test_gpu_address_forms_new.py on the side of each host rule that test means to run, without a GPU:
narrow_rows (csrc/entry_args.hpp) through the stand-alone program of tests/test_address_forms_host.py for
stag_edge_embed_bwd's two switches and stag_agg_bwd_pedge's one, and gat.hip's narrow_extent for the fp32 GAT family.
narrow_extent is `static` in gat.hip, a source of device code that a host program cannot include, so its rule is restated
here and the line of the source it restates is looked up, so that the two cannot drift apart unnoticed."""
import os
import re

import pytest

import test_gpu_address_forms as G
import test_gpu_address_forms_new as N
from test_address_forms_host import _ask, program  # noqa: F401  (the fixture that builds the stand-alone program)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K24, K32 = 1 << 24, 1 << 32


def _rows(program, n, ld, D):
    rc, x_bytes = _ask(program, "rows", n, ld, D, 4)
    assert rc == 0
    return x_bytes


@pytest.mark.parametrize("form", list(G.FORMS))
def test_the_gathered_table_of_each_form(program, form):
    """stag_edge_embed_bwd's `other` (x_bytes) and stag_agg_bwd_pedge's g (g_bytes) take the table of the form; the [46, D]
    gradient table of the embedding, and every table of the packed twin, stay narrow."""
    f = G.FORMS[form]
    m = len(f["sources"])
    for D in f["widths"]:
        xb = _rows(program, f["n_src"], f["stride_bytes"] // 4, D)
        assert (xb == 0) == f["wide"], (form, D, xb)
        if form == "d":
            assert xb >= 1 << 31, "the top of the narrow form: offsets that use all 32 bits"
        assert _rows(program, G.N_EDGES, D, D) == G.N_EDGES * D * 4, "g [E, D] of the embedding: narrow"
        assert _rows(program, m, D, D) == m * D * 4, "the packed twin: narrow"


def test_the_per_edge_runs(program):
    E = G.PE_EDGES
    # stag_edge_embed_bwd: g [E, 8] wide for its rows alone (its extent is below 2^32 bytes), `other` narrow
    D = N.PE_HIDDEN
    assert E >= K24 and E * D * 4 < K32
    assert _rows(program, E, D, D) == 0 and _rows(program, K24 - 1, D, D) > 0
    assert _rows(program, G.PE_N_SRC, D, D) == G.PE_N_SRC * D * 4
    # ... and the compact graph of the checked rows: some 12 rows of 2097 edges, narrow on both
    k = 12 * (E // G.PE_N_DST + 1)
    assert _rows(program, k, D, D) == k * D * 4
    # stag_agg_bwd_pedge at D = 4: the gathered table narrow; the [E, 4] parameter tables have no switch (64-bit indices)
    assert _rows(program, G.PE_N_SRC, 4, 4) == G.PE_N_SRC * 16 and E * 4 * 4 < K32
    # stag_edge_embed_fwd: node ids and edge ids past 2^24; with padded rows e * ldh passes 2^31 elements
    assert N.FWD_NODES > K24 and E > K24 and (E - 1) * max(N.FWD_WIDTHS) < 1 << 31 <= (K24 - 1) * N.FWD_LDH


def _narrow_extent(rows, row_bytes):
    """gat.hip: narrow_extent"""
    nbytes = rows * row_bytes
    return nbytes if nbytes < K32 and rows < K24 else 0


def test_the_gat_rule_is_the_one_restated_here():
    src = open(os.path.join(ROOT, "stag_amd", "csrc", "gat.hip")).read()
    body = re.search(r"static uint32_t narrow_extent\(int64_t rows, uint64_t row_bytes\) \{(.*?)\n\}", src, re.S).group(1)
    lines = [l.strip() for l in body.strip().splitlines()]
    assert lines == ["const uint64_t bytes = (uint64_t)rows * row_bytes;",
                     "return (bytes < (1ull << 32) && rows < (1 << 24)) ? (uint32_t)bytes : 0u;"], lines
    # every extent the fp32 family fills comes from it: ft by source rows, G by destination rows
    assert len(re.findall(r"ft_bytes = narrow_extent\(csr->n_src, \(uint64_t\)(?:a\.)?HF \* (?:4u|ft_esize)\)", src)) == 3
    assert len(re.findall(r"g_bytes = narrow_extent\(csr->n_dst, \(uint64_t\)HF \* 4u\)", src)) == 2


@pytest.mark.parametrize("form", list(N.GAT_FORMS))
def test_the_gat_shapes(form):
    from stag_amd import ops
    f = N.GAT_FORMS[form]
    n, row_bytes, m = f["n"], f["H"] * f["F"] * 4, len(f["nodes"])
    assert ops.gat_cooperative_shape(f["H"], f["F"], N.GAT_SEG)
    assert (_narrow_extent(n, row_bytes) == 0) == f["wide"]           # the graph is square: ft_bytes and g_bytes alike
    assert _narrow_extent(m, row_bytes) == m * row_bytes, "the packed twin: narrow"
    assert min(f["nodes"]) == 0 and max(f["nodes"]) == n - 1 and sorted(f["nodes"]) == f["nodes"]
    last = (n - 1) * row_bytes
    assert (n >= K24) == (form == "a") and (last >= K32) == (form == "c")
    if form == "d":
        assert n == K24 - 1 and row_bytes == 256 and _narrow_extent(n, row_bytes) == K32 - 256
    if form == "c":
        offs = [v * row_bytes for v in f["nodes"]]
        for bound in (1 << 31, K32):
            assert bound - row_bytes in offs and bound in offs, "a gathered row on either side"
    # the destinations (tests/test_gpu_address_forms_new.py: _gat_graphs) sit at both ends of the node range
    dn = [m - 1, 2, m - 2, 0]
    assert f["nodes"][dn[0]] == n - 1 and f["nodes"][dn[3]] == 0 and dn[2] not in (dn[0], dn[3])
