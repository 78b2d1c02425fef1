"""Case tables, float64 references and float32 restatements of the loss-side kernels (stag_sample_kl, stag_normal_kl_*,
stag_edge_mlp_*, stag_contrastive_nll, stag_node_project_*, stag_head_dot_*) away from ordinary numbers.

tests/test_loss_range_host.py runs every case here without a GPU (z from a seeded numpy generator) and proves that the
float32 restatement of each kernel's per-element formula meets the bar the device test uses;
tests/test_gpu_loss_range.py runs the kernels (z from EdgeNoise(...).materialize(): the same counters).

Bars: util.assert_close at util.TOL, element by element, never divided by a tensor's maximum.  A gradient that carries
1/E or 1/n is multiplied by E or n first; a gradient that is a sum over all edges is compared as it is.
Two places reason about the conditioning of their inputs instead: prior_grad_units() (the units of the prior's own
gradients) and DEVICE_EXP_CASES (a log-scale exponentiated on the device under a spike-and-slab prior)."""
from collections import namedtuple

import numpy as np
import torch

F32 = np.float32
GRAPH = dict(n=48, e=200, seed=7, hub=100)        # 300 edges: a permuted eid, a 100-edge row and an empty row
E_SMALL = 300
STRIDE = 512 * 256                                # threads of the grid-stride kernels (amort.hip, contrastive.hip)
N_LONG = STRIDE + 300                             # the second trip of the stride, partly filled
RELU_MARGIN = 2.0 ** -18                          # no sample this close (relatively) to the clip


# ---- mixtures -----------------------------------------------------------------------------------------------------------
def mk_mix(K):
    """tests/test_gpu_sample_kl.make_mix in numpy: (logits, loc, scale) in fp32."""
    j = np.arange(K, dtype=F32)
    probs = (1.0 + j) / (1.0 + j).sum()
    loc = -0.5 + 2.0 * j / max(K - 1, 1) if K > 1 else np.array([0.4])
    return np.log(probs).astype(F32), loc.astype(F32), (0.3 + 0.2 * j).astype(F32)


def _mix(w, m, s):
    w = np.asarray(w, np.float64)
    with np.errstate(divide="ignore"):
        return np.log(w / w.sum()).astype(F32), np.asarray(m, F32), np.asarray(s, F32)


SPIKE = float(np.exp(-6.0))
MIXTURES = {
    "mk2": mk_mix(2),
    # (a) every component at least 40 of its own sigmas from every sample
    "far2": _mix([1, 2], [50, -50], [1, 1]),
    "far3": _mix([1, 2, 3], [50, -50, 52], [1, 1, 1]),
    "far8": _mix(range(1, 9), [50, -50, 52, -52, 54, -54, 56, -56], [1] * 8),
    # (b) exponents more than 104 apart at every sample: the responsibilities are exactly (1, 0) in fp32
    "dom2": _mix([1, 3], [1.0, 30.0], [0.5, 1.0]),
    "dom3": _mix([1, 3, 2], [1.0, 30.0, -30.0], [0.5, 1.0, 1.0]),
    "dom_alone": _mix([1], [1.0], [0.5]),
    # (c) two identical components
    "twin": _mix([0.25, 0.75], [0.4, 0.4], [0.7, 0.7]),
    "twin_alone": _mix([1], [0.4], [0.7]),
    # (d) a zero-weight component that would dominate if its -inf logit were mishandled
    "zero2": _mix([1, 0], [-0.5, 1.0], [0.3, 0.05]),
    "zero3": _mix([1, 0, 2], [-0.5, 1.0, 1.5], [0.3, 0.05, 0.5]),
    # (e) spike and slab
    "spike": _mix([1, 1], [0, 0], [1.0, SPIKE]),
    # (f) K = 8, the capacity of sample_kl_kernel8: slab, spike, far ones, dominated ones and a zero weight on the posterior
    "all8": _mix([2, 2, 1, 1, 0, 1, 1, 1], [0, 0, 50, -50, 0.01, 30, -30, 50], [1.0, SPIKE, 1, 1, 0.005, 1, 1, 0.25]),
}


def scaled_mix(key, c):
    lw, m, s = MIXTURES[key]
    return lw, (m * F32(c)).astype(F32), (s * F32(c)).astype(F32)


# ---- group S: the case table ---------------------------------------------------------------------------------------------
# mode: scalar | per_channel | per_edge1;  log: p1 is a log-scale;  loc, s: numbers (per_channel: s may be "sweep");
# loc = None: loc = s / 4 (relu: about 41 % clipped);  c: the common scale of S3
SCase = namedtuple("SCase", "group name mode log relu dn mix loc s c")
VARIANTS = (("scalar", False), ("scalar", True), ("per_channel", False), ("per_edge1", False), ("per_edge1", True))
RATIOS = (2.0 ** -4, 2.0 ** -10, 2.0 ** -14, 2.0 ** -20)


def _s1():
    out = []
    for mode, log in VARIANTS:
        dn = 24 if mode == "per_channel" else 6
        tag = f"{mode}{'_log' if log else ''}"
        for s in RATIOS + (20.0,):
            out.append(SCase("S1", f"{tag} s={s:.3g}", mode, log, False, dn, "mk2", 1.0, s, 1.0))
            out.append(SCase("S1", f"{tag} relu loc=s/4 s={s:.3g}", mode, log, True, dn, "mk2", None, s, 1.0))
        out.append(SCase("S1", f"{tag} relu unclipped", mode, log, True, dn, "mk2", 1.0, 2.0 ** -4, 1.0))
        out.append(SCase("S1", f"{tag} relu all clipped", mode, log, True, dn, "mk2", -3.0, 2.0 ** -23, 1.0))
    for relu in (False, True):
        out.append(SCase("S1", f"per_channel sweep relu={relu}", "per_channel", False, relu, 24, "mk2", 1.0, "sweep", 1.0))
        out.append(SCase("S1", f"per_edge1_log Dn=260 relu={relu}", "per_edge1", True, relu, 260, "mk2",
                         None if relu else 1.0, 2.0 ** -10, 1.0))
    return out


def _s2():
    out = []
    for mode, log in VARIANTS:
        dn = 24 if mode == "per_channel" else 6
        tag = f"{mode}{'_log' if log else ''}"
        for key in ("far2", "far3", "far8", "dom2", "dom3", "twin", "zero2", "zero3"):
            # (the far pairs sit at +-50: a posterior around 2 keeps every sample 100 exponent units from their midpoint,
            #  where the responsibilities would turn over within one rounding of an exponent of 1250)
            loc, s = (2.0, 0.25) if key.startswith("far") else (1.0, 0.5)
            out.append(SCase("S2", f"{tag} {key}", mode, log, False, dn, key, loc, s, 1.0))
        for key in ("spike", "all8"):
            out.append(SCase("S2", f"{tag} {key}", mode, log, False, dn, key, 0.01, 0.005, 1.0))
    return out


def _s3():
    out = []
    for c in (2.0 ** -20, 2.0 ** 20):
        for mode, log in VARIANTS:
            dn = 24 if mode == "per_channel" else 6
            tag = f"{mode}{'_log' if log else ''}"
            out.append(SCase("S3", f"{tag} c={c:.3g}", mode, log, False, dn, "mk2", 1.0, 2.0 ** -4, c))
            out.append(SCase("S3", f"{tag} relu c={c:.3g}", mode, log, True, dn, "mk2", None, 2.0 ** -4, c))
    return out


S_CASES = _s1() + _s2() + _s3()
# what a case is compared against besides its own reference (S2 b, c): the K = 1 mixture, and whether the value joins
S_TWINS = {"dom2": ("dom_alone", False), "dom3": ("dom_alone", False), "twin": ("twin_alone", True)}


def s_cases(group, mode=None, log=None):
    return [c for c in S_CASES if c.group == group and (mode is None or (c.mode, c.log) == (mode, log))]


def s_params(case, E=E_SMALL):
    """(p0, p1) as the descriptor takes them: numbers (scalar), [Dn] (per_channel) or [E, 1] (per_edge1) fp32 arrays; p1
    is the log-scale where case.log.  Per-edge scales differ from edge to edge by up to 25 %."""
    c = F32(case.c)
    if case.s == "sweep":
        s = (2.0 ** -np.arange(case.dn)).astype(F32)                  # s_k = 2^-k: the whole sweep in one row
    elif case.mode == "per_channel":
        s = np.full(case.dn, case.s, F32)
    elif case.mode == "per_edge1":
        s = (F32(case.s) * (1.0 + 0.25 * np.random.default_rng(11).random((E, 1)))).astype(F32)
    else:
        s = F32(case.s)
    s = (s * c).astype(F32) if isinstance(s, np.ndarray) else F32(s * c)
    p1 = np.log(s).astype(F32) if case.log else s
    s_eff = np.exp(p1.astype(np.float64)).astype(F32) if case.log else s
    loc = (s_eff / F32(4)) if case.loc is None else (np.zeros_like(s_eff) + F32(case.loc) * c)
    if case.mode == "scalar":
        return float(loc), float(p1)
    return np.asarray(loc, F32), np.asarray(p1, F32)


def s_mixture(case):
    return scaled_mix(case.mix, case.c)


def relu_margin_ok(z, p0, p1, log):
    """No element has |loc + s z| below 2^-18 (|loc| + |s z|), in float64: the clip decision and w's relative accuracy
    are then the same in fp32 and float64."""
    a = np.asarray(p0, np.float64)
    s = np.exp(np.asarray(p1, np.float64)) if log else np.asarray(p1, np.float64)
    sz = s * np.asarray(z, np.float64)
    return bool((np.abs(a + sz) >= RELU_MARGIN * (np.abs(a) + np.abs(sz))).all())


# ---- group S: float64 reference and float32 restatement -------------------------------------------------------------------
def sample_kl_ref(z, p0, p1, log, relu, mix, p1_shift=0.0):
    """(kl, d kl / d p0, d kl / d p1) in float64 torch from the fp32 parameter values, autograd through the
    reparameterised draw: q.log_prob(w).sum(-1).mean() - mix.log_prob(w).sum(-1).mean() (the 1/2 log 2 pi cancel).
    p1_shift: added to p1 in float64 (device_exp_terms)."""
    z = torch.as_tensor(np.asarray(z), dtype=torch.float64)
    a = torch.tensor(np.asarray(p0, F32).astype(np.float64), requires_grad=True)
    b = torch.tensor(np.asarray(p1, F32).astype(np.float64) + p1_shift, requires_grad=True)
    lw, m, sj = (torch.tensor(np.asarray(t, F32).astype(np.float64)) for t in mix)
    s = b.exp() if log else b
    w = a + s * z
    if relu:
        w = w.relu()
    lq = -torch.log(s) - 0.5 * ((w - a) / s) ** 2
    lp = torch.logsumexp(lw - torch.log(sj) - 0.5 * ((w.unsqueeze(-1) - m) / sj) ** 2, -1)
    kl = (lq - lp).sum(-1).mean()
    kl.backward()
    return kl.detach().numpy(), a.grad.numpy(), b.grad.numpy()


def sample_kl_f32(z, p0, p1, log, relu, mix, mode):
    """stag_sample_kl's arithmetic in numpy float32 (libm for the hardware exp / log / rcp): per element
        w = fma(s, z, loc), clipped to exactly 0 under relu
        unclipped: u = z, g0 = R/S, g1 = (R/S) dw/dp1 - 1/s (- 1 for a log-scale), dw/dp1 = z (z s)
        clipped:   u = (0 - loc)/s, g0 = u/s, g1 = (u^2 - 1)/s (u^2 - 1)
        t = (-log s - u^2/2) - (mx + log S),  S, R: the shifted mixture sums
    then the sums of the parameter mode.  Returns (kl, d p0, d p1) in the descriptor's layout."""
    with np.errstate(all="ignore"):
        z = np.asarray(z, F32)
        E, dn = z.shape
        loc = np.broadcast_to(np.asarray(p0, F32), (E, dn))
        p1 = np.asarray(p1, F32)
        s = np.broadcast_to(np.exp(p1) if log else p1, (E, dn)).astype(F32)
        w = (loc.astype(np.float64) + s.astype(np.float64) * z.astype(np.float64)).astype(F32)
        clip = ~(w > 0) if relu else np.zeros((E, dn), bool)
        w = np.where(clip, F32(0), w)
        inv = F32(1) / s
        u = np.where(clip, (w - loc) * inv, z)
        lw, m, sj = (np.asarray(t, F32) for t in mix)
        mc, mi = lw - np.log(sj), F32(1) / sj
        d = [(w - m[j]) * mi[j] for j in range(len(m))]
        e = [mc[j] - F32(0.5) * (d[j] * d[j]) for j in range(len(m))]
        mx = np.maximum.reduce(e)
        S, R = np.zeros((E, dn), F32), np.zeros((E, dn), F32)
        for j in range(len(m)):
            x = np.exp(e[j] - mx)
            S = S + x
            R = R + x * (d[j] * mi[j])
        t = (-np.log(s) - F32(0.5) * (u * u)) - (mx + np.log(S))
        rs = R / S
        one = F32(1) if log else inv
        g0 = np.where(clip, u * inv, rs)
        g1 = np.where(clip, (u * u - F32(1)) * one, rs * (z * s if log else z) - one)
        kl = t.sum(1, dtype=F32).astype(np.float64).sum() / E
        if mode == "scalar":
            return kl, g0.sum(dtype=F32) / F32(E), g1.sum(dtype=F32) / F32(E)
        if mode == "per_channel":
            return kl, g0.sum(0, dtype=F32) / F32(E), g1.sum(0, dtype=F32) / F32(E)
        return kl, g0.sum(1, dtype=F32, keepdims=True) / F32(E), g1.sum(1, dtype=F32, keepdims=True) / F32(E)


def sample_kl_parent_f32(z, p0, p1, log, relu, mix, mode):
    """The arithmetic this pull request replaces, for the record: u rebuilt from the rounded sample, g0 = A + (R/S - A) d0,
    g1 = B + (R/S - A) d1.  The host test shows that it misses the bar from s / |loc| = 2^-10 on."""
    with np.errstate(all="ignore"):
        z = np.asarray(z, F32)
        E, dn = z.shape
        loc = np.broadcast_to(np.asarray(p0, F32), (E, dn))
        p1 = np.asarray(p1, F32)
        s = np.broadcast_to(np.exp(p1) if log else p1, (E, dn)).astype(F32)
        w = (loc.astype(np.float64) + s.astype(np.float64) * z.astype(np.float64)).astype(F32)
        mask = (w > 0).astype(F32) if relu else np.ones((E, dn), F32)
        w = np.maximum(w, F32(0)) if relu else w
        inv = F32(1) / s
        u = (w - loc) * inv
        lw, m, sj = (np.asarray(t, F32) for t in mix)
        mc, mi = lw - np.log(sj), F32(1) / sj
        d = [(w - m[j]) * mi[j] for j in range(len(m))]
        e = [mc[j] - F32(0.5) * (d[j] * d[j]) for j in range(len(m))]
        mx = np.maximum.reduce(e)
        S, R = np.zeros((E, dn), F32), np.zeros((E, dn), F32)
        for j in range(len(m)):
            x = np.exp(e[j] - mx)
            S, R = S + x, R + x * (d[j] * mi[j])
        A = u * inv
        G = R * (F32(1) / S) - A
        B = (u * u - F32(1)) * (F32(1) if log else inv)
        g0, g1 = A + G * mask, B + G * ((z * s if log else z) * mask)
        t = (-np.log(s) - F32(0.5) * (u * u)) - (mx + np.log(S))
        kl = t.sum(1, dtype=F32).astype(np.float64).sum() / E
        if mode == "scalar":
            return kl, g0.sum(dtype=F32) / F32(E), g1.sum(dtype=F32) / F32(E)
        if mode == "per_channel":
            return kl, g0.sum(0, dtype=F32) / F32(E), g1.sum(0, dtype=F32) / F32(E)
        return kl, g0.sum(1, dtype=F32, keepdims=True) / F32(E), g1.sum(1, dtype=F32, keepdims=True) / F32(E)


# A per-edge log-scale is exponentiated ON THE DEVICE, by exp_scale = v_exp_f32(l log2 e): the product is rounded to fp32
# (|l| log2 e 2^-24 of the exponent, |l| 2^-24 of s) and the instruction is good to one ulp (2^-23 of s), so the device's
# s — the one the forward pass drew its weights with, which is the sample the estimate is about — is the reference's
# within (|l| + 2) 2^-24.  Nearly everywhere that is far inside the bar.  Under the spike-and-slab priors (S2 e, f) it is
# not: the spike (e^-6) is half as wide as the posterior (0.005), dt/dw = R/S turns over across it with slope
# 1 / s_spike^2 = 1.6e5, and a relative error d of s moves w by s z d — at l = -5.2 up to 4e-9, 7e-4 of one channel's
# gradient.  Those cases therefore add what that uncertainty of the INPUT amounts to, measured on the reference itself.
DEVICE_EXP_CASES = ("spike", "all8")


def device_exp_rel_error(l):
    return (np.abs(np.asarray(l, np.float64)) + 2.0) * 2.0 ** -24


def device_exp_terms(z, p0, p1, relu, mix, ref):
    """How far the float64 reference's (kl, d p0, d p1) move when every [E, 1] log-scale moves by
    +-device_exp_rel_error: the larger of the two one-sided differences, element by element."""
    d = device_exp_rel_error(p1)
    lo, hi = (sample_kl_ref(z, p0, p1, True, relu, mix, p1_shift=sg * d) for sg in (-1.0, 1.0))
    return tuple(np.maximum(np.abs(l - r), np.abs(h - r)) for l, h, r in zip(lo, hi, ref))


def s_grad_scale(mode, E):
    """What a gradient of group S is multiplied by before the comparison: E where it is one edge's (it carries 1 / E)."""
    return float(E) if mode == "per_edge1" else 1.0


# ---- group N: normal_kl_mean ---------------------------------------------------------------------------------------------
PRIOR_SCALES = (1e-3, 1.0, 1e3)
PRIOR_LOC = 0.5
N_KINDS = ("wide", "near", "equal")


def n_inputs(kind, p_scale, n=N_LONG):
    """(loc, log_scale) fp32 [n] and the prior's (loc, scale) as fp32 numbers."""
    rng = np.random.default_rng(5)
    m2, s2 = F32(PRIOR_LOC), F32(p_scale)
    if kind == "wide":          # (i) log-scales over [-16, 8], locations N(0, 100)
        return (100.0 * rng.standard_normal(n)).astype(F32), rng.uniform(-16.0, 8.0, n).astype(F32), m2, s2
    if kind == "near":          # (ii) within 1e-3 of the prior
        return ((m2 + 1e-3 * rng.uniform(-1, 1, n)).astype(F32),
                (np.log(np.float64(s2)) + 1e-3 * rng.uniform(-1, 1, n)).astype(F32), m2, s2)
    return np.full(n, m2, F32), np.full(n, np.log(np.float64(s2)), F32), m2, s2       # (iii) the prior itself


def normal_kl_ref(loc, ls, m2, s2):
    """(kl mean, d loc, d log_scale, d prior loc, d prior scale) in float64 torch (torch's _kl_normal_normal)."""
    a = torch.tensor(loc.astype(np.float64), requires_grad=True)
    b = torch.tensor(ls.astype(np.float64), requires_grad=True)
    pm = torch.tensor(float(m2), dtype=torch.float64, requires_grad=True)
    ps = torch.tensor(float(s2), dtype=torch.float64, requires_grad=True)
    vr = (b.exp() / ps) ** 2
    kl = (0.5 * (vr + ((a - pm) / ps) ** 2 - 1 - vr.log())).mean()
    kl.backward()
    return tuple(t.numpy() for t in (kl.detach(), a.grad, b.grad, pm.grad, ps.grad))


def normal_kl_f32(loc, ls, m2, s2):
    """normal_kl_fwd / bwd_kernel per element in float32; the sums pairwise in float32."""
    with np.errstate(all="ignore"):
        n = F32(loc.size)
        inv, lg2 = F32(1) / s2, np.log(s2)
        r, d = np.exp(ls) * inv, (loc - m2) * inv
        kl = (F32(0.5) * (r * r + d * d - F32(1) - F32(2) * (ls - lg2))).sum(dtype=F32) / n
        cg = F32(1) / n
        vr, t1 = r * r, d * d
        return (kl, cg * (d * inv), cg * (vr - F32(1)), -(d * inv).sum(dtype=F32) / n,
                ((F32(1) - vr - t1) * inv).sum(dtype=F32) / n)


def prior_grad_units(s2):
    """The KL sees the prior only through (m1 - m2) / s2 and s1 / s2, so d / d m2 and d / d s2 are 1 / s2 times a
    function of those ratios: at s2 = 1e-3 one fp32 rounding of s1 / s2 (6e-8) is 6e-5 of d / d s2 whatever the kernel
    does.  The prior's gradients are therefore compared times s2 — the gradients w.r.t. m2 / s2 and log s2 — which is
    the same comparison at s2 = 1."""
    return float(s2)


# ---- groups M, C: the per-edge heads and the contrastive term -----------------------------------------------------------------
HIDDENS = (1, 3, 8)
N_NODES = 300
SATURATED = (100.0, -100.0, 1000.0, -1000.0)      # pre-activations planted on the first edges
NAN_NODE = 17


def m_inputs(hidden, n_par=2, E=N_LONG):
    """src, dst [E] int32 on N_NODES nodes; P [N, 2 hidden]; wh [hidden, n_par]; bh [n_par]; g [n_par, E].  Nodes 0-3 send
    an edge to nodes 4-7 whose pre-activations are SATURATED in every hidden column."""
    rng = np.random.default_rng(100 + hidden)
    src = rng.integers(8, N_NODES, E).astype(np.int32)
    dst = rng.integers(8, N_NODES, E).astype(np.int32)
    P = rng.standard_normal((N_NODES, 2 * hidden)).astype(F32)
    for i, v in enumerate(SATURATED):
        src[i], dst[i] = i, 4 + i
        P[i, :hidden], P[4 + i, hidden:] = F32(v), F32(0)
    src[-1], dst[-2] = NAN_NODE, NAN_NODE             # the last trip of the stride meets the planted node too
    wh = rng.standard_normal((hidden, n_par)).astype(F32)
    bh = rng.standard_normal(n_par).astype(F32)
    g = rng.standard_normal((n_par, E)).astype(F32)
    return src, dst, P, wh, bh, g


def _silu64(pre):
    sg = torch.sigmoid(pre)
    return pre * sg, sg * (1 + pre * (1 - sg))


def edge_mlp_ref(src, dst, P, wh, bh, g):
    """(par [n_par, E], d pre [E, hidden], d wh, d bh) in float64 for the loss sum(g * par)."""
    hidden = wh.shape[0]
    P64, wh64, g64 = (torch.tensor(t.astype(np.float64)) for t in (P, wh, g))
    pre = P64[src.astype(np.int64), :hidden] + P64[dst.astype(np.int64), hidden:]
    h, dh = _silu64(pre)
    par = (h @ wh64 + torch.tensor(bh.astype(np.float64))).T
    dpre = (g64.T @ wh64.T) * dh
    return par.numpy(), dpre.numpy(), (h.T @ g64.T).numpy(), g64.sum(1).numpy()


def _silu32(pre):
    sg = F32(1) / (F32(1) + np.exp(-pre))
    return pre * sg, sg * (F32(1) + pre * (F32(1) - sg))


def edge_mlp_f32(src, dst, P, wh, bh, g):
    with np.errstate(all="ignore"):
        hidden = wh.shape[0]
        pre = P[src, :hidden] + P[dst, hidden:]
        h, dh = _silu32(pre)
        par = np.broadcast_to(bh, (src.size, bh.size)).astype(F32)
        for j in range(hidden):
            par = (h[:, j:j + 1] * wh[j] + par).astype(F32)
        dpre = np.zeros_like(pre)
        for p in range(wh.shape[1]):
            dpre = (g[p][:, None] * wh[:, p] + dpre).astype(F32)
        dwh = np.stack([[(h[:, j] * g[p]).sum(dtype=F32) for p in range(wh.shape[1])] for j in range(hidden)])
        return par.T, dpre * dh, dwh, np.ascontiguousarray(g).sum(1, dtype=F32)


C_KINDS = ("on_target", "wide")
POS, NEG = 1.0, 0.0


def c_inputs(kind, hidden, E=N_LONG):
    """loc, log_scale [E]; fake_src, fake_dst [E] int32; P [N, 2 hidden]; wh [hidden, 2]; bh [2]."""
    rng = np.random.default_rng(200 + hidden)
    fsrc = rng.integers(0, N_NODES, E).astype(np.int32)
    fdst = rng.integers(0, N_NODES, E).astype(np.int32)
    fsrc[-1] = NAN_NODE
    P = rng.standard_normal((N_NODES, 2 * hidden)).astype(F32)
    # mild heads: the fake edges' term goes through exp(-2 l'), which multiplies the roundings of l' (group M has the MLP)
    wh = (0.3 * rng.standard_normal((hidden, 2))).astype(F32)
    bh = (0.1 * rng.standard_normal(2)).astype(F32)
    if kind == "on_target":     # within 2^-20 of the positive target under the narrowest pinned scale
        loc = (POS + 2.0 ** -20 * rng.uniform(-1, 1, E)).astype(F32)
        ls = np.full(E, -16.0, F32)
    else:
        loc = rng.standard_normal(E).astype(F32)
        ls = rng.uniform(-16.0, 8.0, E).astype(F32)
    return loc, ls, fsrc, fdst, P, wh, bh


def contrastive_ref(loc, ls, fsrc, fdst, P, wh, bh):
    """(nll mean, d loc, d log_scale, d pre [E, hidden], d wh, d bh) in float64 torch, autograd."""
    hidden, E = wh.shape[0], loc.size
    a, b = (torch.tensor(t.astype(np.float64), requires_grad=True) for t in (loc, ls))
    P64 = torch.tensor(P.astype(np.float64))
    pre = (P64[fsrc.astype(np.int64), :hidden] + P64[fdst.astype(np.int64), hidden:]).requires_grad_(True)
    w, bb = (torch.tensor(t.astype(np.float64), requires_grad=True) for t in (wh, bh))
    par = torch.nn.functional.silu(pre) @ w + bb
    nlp = lambda v, m, l: 0.5 * ((v - m) * torch.exp(-l)) ** 2 + l + 0.5 * np.log(2 * np.pi)
    nll = (nlp(POS, a, b) + nlp(NEG, par[:, 0], par[:, 1])).mean()
    nll.backward()
    return tuple(t.numpy() for t in (nll.detach(), a.grad, b.grad, pre.grad, w.grad, bb.grad))


def contrastive_f32(loc, ls, fsrc, fdst, P, wh, bh):
    with np.errstate(all="ignore"):
        hidden, E = wh.shape[0], F32(loc.size)
        pre = P[fsrc, :hidden] + P[fdst, hidden:]
        h, dh = _silu32(pre)
        mf, lf = np.full(loc.size, bh[0], F32), np.full(loc.size, bh[1], F32)
        for j in range(hidden):
            mf, lf = h[:, j] * wh[j, 0] + mf, h[:, j] * wh[j, 1] + lf
        ir, irf = np.exp(-ls), np.exp(-lf)
        zr, zf = (F32(POS) - loc) * ir, (F32(NEG) - mf) * irf
        k = F32(0.918938533204672742)
        nll = (((F32(0.5) * (zr * zr) + ls) + k) + ((F32(0.5) * (zf * zf) + lf) + k)).astype(np.float64).sum() / loc.size
        g0, g1 = -(zf * irf), F32(1) - zf * zf
        dpre = ((g1[:, None] * wh[:, 1] + g0[:, None] * wh[:, 0]) * dh) / E
        dwh = np.stack([(h * g0[:, None]).astype(np.float64).sum(0), (h * g1[:, None]).astype(np.float64).sum(0)], 1) / loc.size
        dbh = np.array([g0.astype(np.float64).sum(), g1.astype(np.float64).sum()]) / loc.size
        return nll, -(zr * ir) / E, (F32(1) - zr * zr) / E, dpre, dwh, dbh


# ---- group P: node_project and head_dot -----------------------------------------------------------------------------------
P_ROWS = (5, 1001)                 # partial row teams
P_KS = (9, 128)                    # scalar loads | vector loads
P_COLS = (1, 3, 8, 16)             # the four column tiles: 2, 4, 8, 16
HD_SHAPES = ((3, 40), (4, 8), (1, 256))      # (heads, F): idle lanes | packed heads | the widest head
POW2 = (2.0 ** 60, 2.0 ** -60)


def p_inputs(n, K, C):
    rng = np.random.default_rng(1000 * C + K + n)
    return (rng.standard_normal((n, K)).astype(F32), rng.standard_normal((K, C)).astype(F32),
            rng.standard_normal(C).astype(F32), rng.standard_normal((n, C)).astype(F32))


def node_project_ref(x, w, b, gy):
    x, w, gy = (t.astype(np.float64) for t in (x, w, gy))
    return x @ w + (0 if b is None else b.astype(np.float64)), gy @ w.T, x.T @ gy, gy.sum(0)


def _colsum(a):
    """The sum over axis 0 in float32, pairwise (numpy adds a contiguous last axis as a tree, like the kernels' stages)."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(a, F32), 0, -1)).sum(-1, dtype=F32)


def node_project_f32(x, w, b, gy):
    y = np.zeros((x.shape[0], w.shape[1]), F32)
    for k in range(x.shape[1]):
        y = (x[:, k:k + 1] * w[k] + y).astype(F32)
    dx = np.zeros_like(x)
    for c in range(w.shape[1]):
        dx = (gy[:, c:c + 1] * w[:, c] + dx).astype(F32)
    dw = np.stack([[(x[:, k] * gy[:, c]).sum(dtype=F32) for c in range(w.shape[1])] for k in range(x.shape[1])])
    return (y + b if b is not None else y), dx, dw, _colsum(gy)


def hd_inputs(n, H, F):
    rng = np.random.default_rng(31 * H + F + n)
    return (rng.standard_normal((n, H, F)).astype(F32), rng.standard_normal((H, F)).astype(F32),
            rng.standard_normal((H, F)).astype(F32), rng.standard_normal((2, n, H)).astype(F32))


def head_dot_ref(ft, al, ar, g):
    ft, al, ar, g = (t.astype(np.float64) for t in (ft, al, ar, g))
    el, er = (ft * al).sum(-1), (ft * ar).sum(-1)
    dft = g[0][..., None] * al + g[1][..., None] * ar
    return el, er, dft, (g[0][..., None] * ft).sum(0), (g[1][..., None] * ft).sum(0)


def head_dot_f32(ft, al, ar, g):
    el, er = (ft * al).sum(-1, dtype=F32), (ft * ar).sum(-1, dtype=F32)
    dft = g[0][..., None] * al + g[1][..., None] * ar
    return el, er, dft, _colsum(g[0][..., None] * ft), _colsum(g[1][..., None] * ft)
