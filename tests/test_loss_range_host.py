"""The fixtures of tests/test_gpu_loss_range.py without a GPU (tests/loss_range_cases.py).  For every case:
  - the float64 reference is finite wherever the case says finite, and every expected output is an fp32 number;
  - the float32 restatement of the kernel's per-element formula alone meets the bar the device test uses, so every
    bar is achievable in fp32 — and the arithmetic stag_sample_kl had before misses it from s / |loc| = 2^-14 on;
  - the conditions a case was selected for hold: the clipped share, the distance to the clip, components 40 sigmas
    away, exponents more than 104 apart, a -inf logit, the second trip of the grid stride.
The standard draw z comes from a seeded numpy generator here and from the device's counters there."""
import numpy as np
import pytest

import loss_range_cases as lc
from util import TOL, assert_close, scaled_err

F32 = np.float32


def _draw(dn, E=lc.E_SMALL):
    return np.random.default_rng(77).standard_normal((E, dn)).astype(F32)


def _fp32_numbers(*arrays):
    for a in arrays:
        a = np.asarray(a, np.float64)
        assert np.isfinite(a).all() and np.isfinite(a.astype(F32)).all(), "finite, and representable in fp32"


def _s_compare(case, got, ref, what):
    sc = lc.s_grad_scale(case.mode, lc.E_SMALL)
    assert_close(got[0], ref[0], what=what + " kl")
    assert_close(np.asarray(got[1], np.float64) * sc, ref[1] * sc, what=what + " d p0")
    assert_close(np.asarray(got[2], np.float64) * sc, ref[2] * sc, what=what + " d p1")


@pytest.mark.parametrize("case", lc.S_CASES, ids=lambda c: f"{c.group} {c.name}")
def test_group_S(case):
    z = _draw(case.dn)
    p0, p1 = lc.s_params(case)
    mix = lc.s_mixture(case)
    ref = lc.sample_kl_ref(z, p0, p1, case.log, case.relu, mix)
    _fp32_numbers(*ref)
    _s_compare(case, lc.sample_kl_f32(z, p0, p1, case.log, case.relu, mix, case.mode), ref, case.name)
    s = np.exp(np.asarray(p1, np.float64)) if case.log else np.asarray(p1, np.float64)
    w = np.asarray(p0, np.float64) + s * z
    if case.relu:
        assert lc.relu_margin_ok(z, p0, p1, case.log)
        share = float((w <= 0).mean())
        if case.loc is None:
            assert 0.35 < share < 0.47, share           # P(z < -1/4) = 0.401
        elif case.s != "sweep":                          # (the sweep's widest channels clip a few of theirs)
            assert share == (0.0 if case.loc > 0 else 1.0)
    lw, m, sj = (np.asarray(t, np.float64) for t in mix)
    expo = lw - np.log(sj) - 0.5 * ((w[..., None] - m) / sj) ** 2
    if case.mix.startswith("far"):
        assert (np.abs(w[..., None] - m) >= 40 * sj).all() and expo.max() < -103, "every exp would underflow unshifted"
    if case.mix.startswith("dom"):
        assert (expo[..., 0:1] - expo[..., 1:] > 104).all(), "responsibilities of exactly (1, 0) in fp32"
    if case.mix.startswith("zero") or case.mix == "all8":
        assert np.isneginf(lw).sum() == 1
    if case.mix == "all8":
        assert len(lw) == 8
        assert (np.sort(expo, -1)[..., :3] < expo.max(-1, keepdims=True) - 104).all(), "far components underflow"
    if case.mode == "per_edge1" and case.log and case.mix in lc.DEVICE_EXP_CASES:
        terms = lc.device_exp_terms(z, p0, p1, case.relu, mix, ref)
        assert lc.device_exp_rel_error(p1).max() < 5e-7
        for i in (1, 2):       # what the device's exponential may add stays a small multiple of the bar
            assert (terms[i] * lc.E_SMALL <= 10 * TOL * (1 + np.abs(ref[i] * lc.E_SMALL))).all()
    if case.mix in lc.S_TWINS:
        key, with_value = lc.S_TWINS[case.mix]
        alone = lc.sample_kl_ref(z, p0, p1, case.log, case.relu, lc.scaled_mix(key, case.c))
        sc = lc.s_grad_scale(case.mode, lc.E_SMALL)
        for i in ((0, 1, 2) if with_value else (1, 2)):
            k = 1.0 if i == 0 else sc
            assert_close(ref[i] * k, alone[i] * k, what=f"{case.name} against the one component [{i}]")


@pytest.mark.parametrize("s", [2.0 ** -14, 2.0 ** -20])
def test_the_replaced_arithmetic_misses_the_bar(s):
    """What S1 is for: the form that rebuilds u from the rounded sample is outside the bar for narrow posteriors."""
    case = next(c for c in lc.s_cases("S1", "per_edge1", False) if c.s == s and not c.relu)
    z = _draw(case.dn)
    p0, p1 = lc.s_params(case)
    ref = lc.sample_kl_ref(z, p0, p1, False, False, lc.s_mixture(case))
    got = lc.sample_kl_parent_f32(z, p0, p1, False, False, lc.s_mixture(case), case.mode)
    assert scaled_err(np.asarray(got[2], np.float64) * lc.E_SMALL, ref[2] * lc.E_SMALL) > TOL


def test_case_table_covers_what_it_says():
    for mode, log in lc.VARIANTS:
        s1 = lc.s_cases("S1", mode, log)
        assert {c.s for c in s1 if not c.relu} >= set(lc.RATIOS) | {20.0}
        assert any(c.relu and c.loc is None for c in s1) and any(c.relu and c.loc == -3.0 for c in s1)
        assert len(lc.s_cases("S3", mode, log)) == 4
    assert {len(lc.MIXTURES[c.mix][0]) for c in lc.s_cases("S2")} == {2, 3, 8}
    assert any(c.dn == 260 for c in lc.S_CASES) and any(c.s == "sweep" for c in lc.S_CASES)
    assert {c.dn % 4 for c in lc.S_CASES} == {0, 2}, "a tail chunk and whole chunks"
    assert lc.N_LONG > lc.STRIDE and lc.N_LONG % 256 != 0


@pytest.mark.parametrize("p_scale", lc.PRIOR_SCALES)
@pytest.mark.parametrize("kind", lc.N_KINDS)
def test_group_N(kind, p_scale):
    loc, ls, m2, s2 = lc.n_inputs(kind, p_scale)
    n, u = loc.size, lc.prior_grad_units(s2)
    ref = lc.normal_kl_ref(loc, ls, m2, s2)
    got = lc.normal_kl_f32(loc, ls, m2, s2)
    _fp32_numbers(*ref)
    what = f"{kind} prior scale {p_scale}"
    assert_close(got[0], ref[0], what=what + " kl")
    assert_close(got[1].astype(np.float64) * n, ref[1] * n, what=what + " n d loc")
    assert_close(got[2].astype(np.float64) * n, ref[2] * n, what=what + " n d log_scale")
    assert_close(float(got[3]) * u, ref[3] * u, what=what + " s2 d prior loc")
    assert_close(float(got[4]) * u, ref[4] * u, what=what + " s2 d prior scale")
    if kind == "equal":
        for i, k in ((0, 1.0), (1, n), (2, n), (3, u), (4, u)):
            assert np.abs(ref[i] * k).max() <= TOL, "the reference itself is 0 within the bar"
    if kind == "near":
        assert np.abs(loc - m2).max() <= 1.001e-3 and np.abs(ls - np.log(np.float64(s2))).max() <= 1.001e-3
    if kind == "wide":
        assert ls.min() < -15.9 and ls.max() > 7.9


@pytest.mark.parametrize("hidden", lc.HIDDENS)
def test_group_M(hidden):
    src, dst, P, wh, bh, g = lc.m_inputs(hidden)
    ref = lc.edge_mlp_ref(src, dst, P, wh, bh, g)
    got = lc.edge_mlp_f32(src, dst, P, wh, bh, g)
    _fp32_numbers(*ref)
    for r, q, nm in zip(ref, got, ("par", "d pre", "d wh", "d bh")):
        assert_close(q, r, what=f"hidden={hidden} {nm}")
    pre = P[src[:4], :hidden] + P[dst[:4], hidden:]
    assert (pre == np.asarray(lc.SATURATED, F32)[:, None]).all()
    assert np.abs(ref[1][1]).max() < 1e-38 and (ref[1][3] == 0).all(), "SiLU' saturates to 0 at -100 and -1000"
    assert (ref[1][0] == (g[:, 0] @ wh.T.astype(np.float64))).all(), "and to the identity at 100"
    touched = (src == lc.NAN_NODE) | (dst == lc.NAN_NODE)
    assert touched[lc.STRIDE:].any() and touched[:lc.STRIDE].any() and not touched[:4].any()


@pytest.mark.parametrize("hidden", (1, 3))
@pytest.mark.parametrize("kind", lc.C_KINDS)
def test_group_C(kind, hidden):
    args = lc.c_inputs(kind, hidden)
    ref = lc.contrastive_ref(*args)
    got = lc.contrastive_f32(*args)
    _fp32_numbers(*ref)
    E = args[0].size
    for i, nm in enumerate(("nll", "E d loc", "E d log_scale", "E d pre", "d wh", "d bh")):
        k = E if nm.startswith("E ") else 1.0
        assert_close(np.asarray(got[i], np.float64) * k, ref[i] * k, what=f"{kind} hidden={hidden} {nm}")
    if kind == "on_target":
        assert np.abs(args[0] - 1.0).max() <= 2.0 ** -20 and (args[1] == -16.0).all()


@pytest.mark.parametrize("C", lc.P_COLS)
@pytest.mark.parametrize("K", lc.P_KS)
def test_group_P_node_project(K, C):
    x, w, b, gy = lc.p_inputs(1001, K, C)
    for r, q, nm in zip(lc.node_project_ref(x, w, b, gy), lc.node_project_f32(x, w, b, gy), ("y", "dx", "dw", "db")):
        assert_close(q, r, what=f"K={K} C={C} {nm}")
    for c in lc.POW2:
        assert np.array_equal(lc.node_project_f32(x * F32(c), w, None, gy)[0], lc.node_project_f32(x, w, None, gy)[0] * F32(c))


@pytest.mark.parametrize("H,F", lc.HD_SHAPES)
def test_group_P_head_dot(H, F):
    args = lc.hd_inputs(1001, H, F)
    for r, q, nm in zip(lc.head_dot_ref(*args), lc.head_dot_f32(*args), ("el", "er", "d ft", "d attn_l", "d attn_r")):
        assert_close(q, r, what=f"H={H} F={F} {nm}")
