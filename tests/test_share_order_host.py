"""The share order of a plan's units (stag_plan_share, the host builder): whole-row units that gather the same source
row side by side, inside their class of equal trip count, aligned to absolute unit indices.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from stag_amd import _lib, synthetic
from stag_amd.graph import repeated_sources

HEAVY = _lib.HEAVY_LEN


def csr_of(rows):
    """(indptr, indices) of a list of per-destination source lists"""
    indptr = np.zeros(len(rows) + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.array([s for r in rows for s in r], np.int32)
    return indptr, indices


def csr_of_edges(src, dst, n):
    order = np.argsort(dst, kind="stable")
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    return indptr, src[order].astype(np.int32)


def host_plan(indptr, seg_len):
    lib = _lib.lib()
    n = len(indptr) - 1
    nu, nl, ns, nh = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(lib.stag_plan_count(indptr.ctypes.data, n, seg_len, C.byref(nu), C.byref(nl), C.byref(ns), C.byref(nh)), "count")
    units = np.zeros((max(nu.value, 1), 4), np.int32)
    long_rows, long_seg_ptr = np.zeros(max(nl.value, 1), np.int32), np.zeros(nl.value + 1, np.int32)
    _lib.check(lib.stag_plan_fill(indptr.ctypes.data, n, seg_len, units.ctypes.data, long_rows.ctypes.data,
                                  long_seg_ptr.ctypes.data), "fill")
    return units[:nu.value], ns.value, nh.value


def share_host(units, n_seg, n_heavy, seg_len, indices):
    out = np.full_like(units, -7)
    idx = np.ascontiguousarray(indices, np.int32)
    _lib.check(_lib.lib().stag_plan_share(units.ctypes.data, len(units), n_seg, n_heavy, seg_len, idx.ctypes.data, len(idx),
                                          out.ctypes.data), "stag_plan_share")
    return out


def check_contract(units, out, n_seg, n_heavy):
    """What every share order must keep, whichever builder made it."""
    assert out.shape == units.shape
    as_set = lambda a: sorted(map(tuple, a.tolist()))
    assert as_set(out[n_seg:]) == as_set(units[n_seg:]), "not a permutation of the whole-row records"
    assert np.array_equal(out[:n_seg], units[:n_seg]), "a segment record moved"
    trips = (out[n_seg:, 2] + 1) // 2
    assert np.all(trips[:-1] >= trips[1:]), "trip counts must not increase"
    assert np.array_equal(trips, (units[n_seg:, 2] + 1) // 2), "a record left its class of equal trip count"
    assert np.all(out[n_seg:, 3] == -1)
    assert np.all(out[n_seg:n_heavy, 2] > HEAVY) and np.all(out[n_heavy:, 2] <= HEAVY), "n_heavy is no longer a prefix"


def positions(out):
    """unit index of every whole row"""
    return {int(r): i for i, (r, _, _, slot) in enumerate(out.tolist()) if slot < 0}


def paired_rows(n_rows, partner, length=3):
    """rows of `length` edges; row r and partner(r) share exactly one source, every other source is unique"""
    rows, fresh = [], 10_000
    for r in range(n_rows):
        p = partner(r)
        row = [min(r, p)] if p is not None else []
        while len(row) < length:
            row.append(fresh)
            fresh += 1
        rows.append(row)
    return rows


@pytest.mark.parametrize("partner", [lambda r: r ^ 1, lambda r: (r + 32) % 64], ids=["neighbours", "far"])
def test_every_pair_is_found(partner):
    indptr, indices = csr_of(paired_rows(64, partner))
    units, n_seg, n_heavy = host_plan(indptr, 64)
    assert n_seg == 0 and len(units) == 64
    out = share_host(units, n_seg, n_heavy, 64, indices)
    check_contract(units, out, n_seg, n_heavy)
    at = positions(out)
    for r in range(64):
        a, b = sorted((at[r], at[partner(r)]))
        assert a % 2 == 0 and b == a + 1, f"rows {r} and {partner(r)} share a source and lie at {a}, {b}"
    assert repeated_sources(out, n_seg, indices, block=2) == 32 == repeated_sources(out, n_seg, indices, block=8)


def test_quads_and_octets_are_aligned():
    # 8 rows around source 0, 4 around source 1, 2 around source 2, spread over 40 rows of 4 edges
    rows, fresh = [], 10_000
    member = {r: 0 for r in (1, 6, 11, 17, 22, 29, 33, 38)}
    member.update({r: 1 for r in (3, 12, 25, 36)})
    member.update({r: 2 for r in (8, 30)})
    for r in range(40):
        row = [member[r]] if r in member else []
        while len(row) < 4:
            row.append(fresh)
            fresh += 1
        rows.append(row)
    indptr, indices = csr_of(rows)
    units, n_seg, n_heavy = host_plan(indptr, 64)
    out = share_host(units, n_seg, n_heavy, 64, indices)
    check_contract(units, out, n_seg, n_heavy)
    at = positions(out)
    for size, s in ((8, 0), (4, 1), (2, 2)):
        where = sorted(at[r] for r in member if member[r] == s)
        assert where[0] % size == 0 and where == list(range(where[0], where[0] + size)), (size, where)
    assert repeated_sources(out, n_seg, indices) == 7 + 3 + 1


def test_five_node_graph():
    indptr, indices = csr_of([[1, 2], [0], [], [0, 1, 4], [0]])
    for seg_len in (2, 64):
        units, n_seg, n_heavy = host_plan(indptr, seg_len)
        out = share_host(units, n_seg, n_heavy, seg_len, indices)
        check_contract(units, out, n_seg, n_heavy)


def test_empty_rows_and_no_edges():
    rows = paired_rows(20, lambda r: r ^ 1, length=2)
    rows = [r if i % 3 else [] for i, r in enumerate(rows)]
    indptr, indices = csr_of(rows)
    units, n_seg, n_heavy = host_plan(indptr, 64)
    out = share_host(units, n_seg, n_heavy, 64, indices)
    check_contract(units, out, n_seg, n_heavy)
    indptr, indices = csr_of([[], [], []])
    units, n_seg, n_heavy = host_plan(indptr, 64)
    out = share_host(units, n_seg, n_heavy, 64, np.zeros(1, np.int32)[:0])
    check_contract(units, out, n_seg, n_heavy)


@pytest.mark.parametrize("n_hub_edges", [0, 17, 24])
def test_odd_class_sizes_and_alignment_holes(n_hub_edges):
    # classes of 5, 7 and 11 rows (6, 4 and 2 edges) behind 0, 3 or 3 segments of a hub (seg_len 8): every class starts
    # off a multiple of 8 somewhere; each class holds pairs and single rows to fill the hole in front of them
    rows, fresh = [], 10_000
    shared = 100
    pairs = []
    for length, n_rows, n_pairs in ((6, 5, 2), (4, 7, 2), (2, 11, 4)):
        base = len(rows)
        for k in range(n_rows):
            row = []
            if k < 2 * n_pairs:
                row.append(shared + k // 2)
            while len(row) < length:
                row.append(fresh)
                fresh += 1
            rows.append(row)
        pairs += [(base + 2 * k, base + 2 * k + 1) for k in range(n_pairs)]
        shared += 50
    if n_hub_edges:
        rows.append(list(range(20_000, 20_000 + n_hub_edges)))
    indptr, indices = csr_of(rows)
    units, n_seg, n_heavy = host_plan(indptr, 8)
    assert n_seg == (0 if not n_hub_edges else -(-n_hub_edges // 8))
    out = share_host(units, n_seg, n_heavy, 8, indices)
    check_contract(units, out, n_seg, n_heavy)
    at = positions(out)
    for a, b in pairs:
        lo, hi = sorted((at[a], at[b]))
        assert lo % 2 == 0 and hi == lo + 1, f"rows {a}, {b} at {lo}, {hi} (n_seg {n_seg})"


def test_too_few_single_rows_for_the_hole():
    # 3 rows of 6 edges, then 8 rows of 4 edges that are all paired: the hole of 5 in front of index 8 takes one pair whole
    # and another apart — still a permutation inside the class, and the pairs that were not taken apart stay aligned
    rows = paired_rows(3, lambda r: None, length=6) + [[500 + r // 2, 600 + r, 700 + r, 800 + r] for r in range(8)]
    indptr, indices = csr_of(rows)
    units, n_seg, n_heavy = host_plan(indptr, 64)
    out = share_host(units, n_seg, n_heavy, 64, indices)
    check_contract(units, out, n_seg, n_heavy)
    assert repeated_sources(out, n_seg, indices, block=2) >= 3


def test_skewed_graph_keeps_the_contract_and_finds_repeats():
    src, dst = synthetic.arxiv_like(n_nodes=2000, n_edges=12000, max_in_degree=1200, n_hubs=5, seed=4)
    indptr, indices = csr_of_edges(src, dst, 2000)
    for seg_len in (8, 64):
        units, n_seg, n_heavy = host_plan(indptr, seg_len)
        out = share_host(units, n_seg, n_heavy, seg_len, indices)
        check_contract(units, out, n_seg, n_heavy)
        assert np.array_equal(out, share_host(units, n_seg, n_heavy, seg_len, indices))
        plan_order, share_order = repeated_sources(units, n_seg, indices), repeated_sources(out, n_seg, indices)
        assert share_order > plan_order and share_order >= 100, (seg_len, plan_order, share_order)


def test_refusals():
    indptr, indices = csr_of([[1], [0]])
    units, n_seg, n_heavy = host_plan(indptr, 64)
    out = np.zeros_like(units)
    lib = _lib.lib()
    args = lambda **kw: [kw.get("units", units.ctypes.data), kw.get("n_units", 2), kw.get("n_seg", 0), kw.get("n_heavy", 0),
                         kw.get("seg_len", 64), kw.get("indices", indices.ctypes.data), 2, kw.get("out", out.ctypes.data)]
    assert lib.stag_plan_share(*args()) == 0
    for bad in (dict(n_seg=1), dict(n_heavy=3), dict(seg_len=0), dict(seg_len=(1 << 20) + 1), dict(units=None),
                dict(indices=None), dict(out=None), dict(out=units.ctypes.data), dict(n_units=-1)):
        assert lib.stag_plan_share(*args(**bad)) == -22, bad
    header = open(_lib.__file__.replace("stag_amd/_lib.py", "include/stag_hip.h")).read()
    assert "stag_plan_share_device(" in header and "#define STAG_ABI_VERSION 19" in header      # additive: no bump
