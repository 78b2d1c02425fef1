"""Everything tests/test_gpu_edge_embed_range.py takes for granted, without a GPU: the graph of
tests/edge_embed_range_cases.py plants every value on both tables and meets the planted node of the containment tests from
both sides; and the bar is a property of the INPUTS, not of the kernel: the documented formula restated in numpy float32
(loss_range_cases._silu32) stays within util.TOL (util.assert_close for h, util.assert_close_cond for the sums) of the
float64 reference on every planted input, at every width and at the scaled magnitudes.  STAG_PRINT_ERR=1 prints each
distance; the worst recorded here, against the bar of 1e-05: SiLU 3.9e-08 and SiLU' 3.3e-07 on the planted edges, h
1.1e-07 over all edges, and 0.26 of the conditioned bar for the sums (hidden 260, d pd).  No planted value had to be moved."""
import numpy as np
import pytest

import edge_embed_range_cases as ec
from util import TOL, assert_close, assert_close_cond, scaled_err

F32 = np.float32


def test_the_graph():
    src, dst = ec.edges()
    pl = ec.planted_edges()
    assert len(set(pl.ravel().tolist())) == 2 * len(ec.PLANTED)
    ps, pd, g = ec.tables(5)
    pre = ps[src] + pd[dst]
    assert pre.dtype == F32
    for i, v in enumerate(ec.PLANTED):
        assert (pre[pl[i]] == F32(v)).all(), v
        assert (ps[src[pl[i, 0]]] == F32(v)).all() and (pd[dst[pl[i, 0]]] == 0).all(), "through the source's row"
        assert (pd[dst[pl[i, 1]]] == F32(v)).all() and (ps[src[pl[i, 1]]] == 0).all(), "through the destination's row"
    indeg, outdeg = np.bincount(dst, minlength=ec.N), np.bincount(src, minlength=ec.N)
    for i in range(len(ec.PLANTED)):
        a = 4 * i
        assert indeg[a + 1] == indeg[a + 3] == 4 and outdeg[a] == outdeg[a + 2] == 4, "a planted term is summed with three others"
    assert indeg[ec.HUB] > ec.N_HUB and indeg[ec.N - 1] == outdeg[ec.N - 1] == 0
    for node in (ec.NAN_NODE, ec.NAN_NODE + 1):            # the rows the containment tests plant NaN and +-inf in
        assert indeg[node] >= 2 and outdeg[node] >= 2 and ec.FIRST_FREE <= node < ec.N - 1 and node != ec.HUB
    assert len(set(src[dst == ec.HUB])) > 16, "the hub's row is cut into segments at seg_len 16"
    assert sorted(np.unique(src * ec.N + dst, return_counts=True)[1])[-1] > 1, "multi-edges"
    assert (src == dst).any(), "self loops"
    # what the planted values are for
    big = np.exp(np.float64(88.5)), np.exp(np.float64(88.75))
    assert big[0] < np.finfo(F32).max < big[1], "expf(-pre) overflows between -88.5 and -88.75"
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(F32(104.0))) and np.isfinite(np.exp(F32(87.0)))
    one = F32(1)
    sg = lambda v: one / (one + np.exp(-F32(v)))
    assert one - sg(16.0) > 0 and one - sg(17.0) == 0 and one - sg(18.0) == 0, "1 - sg vanishes from 17 on"
    assert abs(ec.silu64(-1.2785)[1]) < 1e-4 and ec.silu64(-1.3)[1] < 0 < ec.silu64(-1.25)[1], "the zero of SiLU'"


def test_the_two_float64_forms_agree_where_both_are_finite():
    pre = np.concatenate([np.linspace(-700, 700, 2801), np.asarray(ec.PLANTED)])
    for a, b in zip(ec.silu64(pre), ec.silu_formula64(pre)):
        assert scaled_err(b, a) <= 1e-12
    h, dh = ec.silu64(np.array([0.0, 64.0, -256.0, 1000.0, -1000.0]))
    assert h[0] == 0 and dh[0] == 0.5 and dh[3] == 1 and dh[4] == 0 and h[3] == 1000 and h[4] == 0
    # +-inf: the documented formula gives NaN for SiLU' on both sides, SiLU = inf | NaN
    h, dh = ec.silu_formula64(np.array([np.inf, -np.inf]))
    assert np.isnan(dh).all() and h[0] == np.inf and np.isnan(h[1])


@pytest.mark.parametrize("hidden", ec.HIDDENS)
def test_the_float32_restatement_stays_inside_the_bars(hidden):
    ps, pd, g = ec.tables(hidden)
    h, ds, dd, ds_abs, dd_abs = ec.reference(ps, pd, g)
    h32, ds32, dd32 = ec.reference32(ps, pd, g)
    for a in (h, ds, dd):
        assert np.isfinite(a).all()
    assert np.isfinite(h32).all() and np.isfinite(ds32).all() and np.isfinite(dd32).all()
    assert_close(h32, h, what=f"float32 restatement hidden={hidden} h")
    assert_close_cond(ds32, ds, ds_abs, what=f"float32 restatement hidden={hidden} d ps")
    assert_close_cond(dd32, dd, dd_abs, what=f"float32 restatement hidden={hidden} d pd")
    # the planted edges alone, term by term, at the plain bar
    src, dst = ec.edges()
    pl = ec.planted_edges().ravel()
    pre = (ps[src[pl]] + pd[dst[pl]]).astype(F32)
    (h64, d64), (hq, dq) = ec.silu64(pre.astype(np.float64)), ec.silu32(pre)
    assert_close(hq, h64, what=f"float32 restatement hidden={hidden} planted SiLU")
    assert_close(dq, d64, what=f"float32 restatement hidden={hidden} planted SiLU'")
    assert scaled_err(hq, h64) <= 0.05 * TOL and scaled_err(dq, d64) <= 0.2 * TOL, "far inside: nothing has to be moved"


@pytest.mark.parametrize("g_exp", (60, -60))
def test_the_scaled_magnitudes(g_exp):
    """Tables at 2^-60, g at 2^+-60: every number involved is a normal fp32 number, and scaling back is exact."""
    ps, pd, g = ec.tables(16, scale=2.0 ** -60, g_scale=2.0 ** g_exp)
    h, ds, dd, ds_abs, dd_abs = ec.reference(ps, pd, g)
    h32, ds32, dd32 = ec.reference32(ps, pd, g)
    tiny = np.finfo(F32).tiny
    assert np.abs(h32[h32 != 0]).min() > tiny and np.abs(ds32[ds32 != 0]).min() > tiny and np.abs(ds32).max() < 3e38
    k, kg = 2.0 ** 60, 2.0 ** -g_exp
    assert_close(h32.astype(np.float64) * k, h * k, what="scaled h")
    assert_close_cond(ds32.astype(np.float64) * kg, ds * kg, ds_abs * kg, what="scaled d ps")
    assert_close_cond(dd32.astype(np.float64) * kg, dd * kg, dd_abs * kg, what="scaled d pd")
