"""Inputs and references of the fused likelihood head (stag_nll_categorical_* / stag_nll_bernoulli_*), no device needed:
the closed forms of include/stag_hip.h in numpy, evaluated in float64 (the reference) or in float32 (what any fp32
implementation of the same formulas can be asked for), and the cases the device tests run.

The generic inputs stay away from the two places where the gradient is ill-conditioned in fp32 whatever computes it:
1 / p_y - 1 / s cancels as q -> 1, and 1 / p_y amplifies a rounding of p_y as p_y -> 0.  The clamp edges have exact
cases of their own (edge_* below)."""
import functools

import numpy as np

EPS = 2.0 ** -23          # torch.finfo(torch.float32).eps
SLAB = 64                 # rows of a forward workgroup up to 131,072 rows

# (rows, channels): every team width (C = 1, 2, 3 .. 8, .. 256), C % 4 != 0, exactly one channel tile (256) and one more
# channel (257), several tiles (1000); rows on both sides of a wave's rows, of the slab and of a multi-slab merge
CAT_SHAPES = [(1, 1), (65, 1), (2, 2), (1000, 2), (63, 3), (4099, 3), (64, 7), (1000, 7), (63, 40), (64, 40), (65, 40),
              (4099, 40), (1, 41), (1000, 41), (2, 64), (4099, 64), (63, 65), (1000, 65), (64, 121), (4099, 121),
              (65, 256), (1000, 256), (1, 257), (4099, 257), (2, 1000), (1000, 1000)]
BERN_SHAPES = [(1, 1), (64, 1), (4099, 1), (2, 5), (63, 5), (1000, 5), (65, 121), (1000, 121), (4099, 121), (1, 260),
               (64, 260), (1000, 260)]
MASKS = ["none", "all", "empty", "single", "ends", "half", "one_slab"]


def mask_of(kind, n, seed=0):
    """None, or a bool [n]."""
    if kind == "none":
        return None
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "single":
        m[n // 2] = True
    elif kind == "ends":
        m[0] = m[-1] = True
    elif kind == "half":
        m[:] = np.random.default_rng(1000 + seed).random(n) < 0.5
    elif kind == "one_slab":                    # every true row inside the second slab (the first where there is one)
        lo = SLAB if n > SLAB else 0
        m[lo:min(lo + SLAB, n):2] = True
    elif kind != "empty":
        raise ValueError(kind)
    return m


def categorical_inputs(n, C, seed=0):
    """(p float32 [n, C] unnormalised probabilities, y int64 [n]): softmax of 2 N(0,1) logits times a per-row factor in
    [0.5, 2], p_y floored at 1e-3 of the row sum."""
    rng = np.random.default_rng(seed * 7919 + n * 31 + C)
    z = 2.0 * rng.standard_normal((n, C))
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    y = rng.integers(0, C, n)
    rows = np.arange(n)
    p[rows, y] = np.maximum(p[rows, y], 1e-3)
    p *= rng.uniform(0.5, 2.0, (n, 1))
    return p.astype(np.float32), y.astype(np.int64)


def bernoulli_inputs(n, C, seed=0):
    """(p float32 [n, C] in [1e-3, 1 - 1e-3], y float32 [n, C] of zeros and ones)"""
    rng = np.random.default_rng(seed * 104729 + n * 17 + C)
    p = 1.0 / (1.0 + np.exp(-2.0 * rng.standard_normal((n, C))))
    p = np.clip(p, 1e-3, 1.0 - 1e-3)
    y = (rng.random((n, C)) < 0.5)
    return p.astype(np.float32), y.astype(np.float32)


def _clamp(q, eps):
    """min(max(q, eps), 1 - eps) as torch.clamp: a NaN stays one"""
    one = q.dtype.type(1)
    return np.where(q < eps, eps, np.where(q > one - eps, one - eps, q))


def categorical_ref(p, y, mask=None, g=1.0, dtype=np.float64):
    """(value, dprobs [n, C]) of the masked mean NLL of Categorical(probs=p) at labels y, upstream gradient g, every
    operation in `dtype`."""
    p = np.asarray(p).astype(dtype)
    n, C = p.shape
    eps, one = dtype(EPS), dtype(1)
    m = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    ok = (y >= 0) & (y < C)
    yy = np.where(ok, y, 0)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        s = p.sum(1, dtype=dtype)
        py = p[rows, yy]
        q = py / s
        nll = -np.log(_clamp(q, eps))
        nll[~ok] = np.nan
        count = dtype(m.sum())
        value = nll[m].sum(dtype=dtype) / count
        live = m & ok & (q >= eps) & (q <= one - eps)
        c0 = -(dtype(g) / count)
        d = np.zeros((n, C), dtype)
        d[live] = (c0 * (dtype(0) - one / s[live]))[:, None]
        d[rows[live], yy[live]] = c0 * (one / py[live] - one / s[live])
    return dtype(value), d


def bernoulli_ref(p, y, mask=None, g=1.0, dtype=np.float64):
    """(value, dprobs [n, C]) of the masked mean NLL of Bernoulli(probs=p) at targets y, every operation in `dtype`."""
    p, y = np.asarray(p).astype(dtype), np.asarray(y).astype(dtype)
    n, C = p.shape
    eps, one = dtype(EPS), dtype(1)
    m = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    with np.errstate(all="ignore"):
        pc = _clamp(p, eps)
        nll = -(y * np.log(pc) + (one - y) * np.log1p(-pc))
        denom = dtype(m.sum()) * dtype(C)
        value = nll[m].sum(dtype=dtype) / denom
        inside = (p >= eps) & (p <= one - eps) & m[:, None]
        d = np.where(inside, (dtype(g) / denom) * (-y / pc + (one - y) / (one - pc)), dtype(0))
    return dtype(value), d.astype(dtype)


@functools.lru_cache(maxsize=None)
def categorical_case(n, C, mask_kind, seed=0):
    """(p, y, mask, value64, dprobs64 at g = 1): computed once, shared by every test that asks; do not write to them"""
    p, y = categorical_inputs(n, C, seed)
    mask = mask_of(mask_kind, n, seed)
    value, d = categorical_ref(p, y, mask)
    for a in (p, y, mask, d):
        if a is not None:
            a.setflags(write=False)
    return p, y, mask, value, d


@functools.lru_cache(maxsize=None)
def bernoulli_case(n, C, mask_kind, seed=0):
    p, y = bernoulli_inputs(n, C, seed)
    mask = mask_of(mask_kind, n, seed)
    value, d = bernoulli_ref(p, y, mask)
    for a in (p, y, mask, d):
        if a is not None:
            a.setflags(write=False)
    return p, y, mask, value, d


def cat_case_list():
    """(n, C, mask kind) of the device tests: every shape with two mask kinds dealt round, every mask kind at two shapes"""
    out = []
    for i, (n, C) in enumerate(CAT_SHAPES):
        out.append((n, C, MASKS[i % len(MASKS)]))
        out.append((n, C, MASKS[(i + 3) % len(MASKS)]))
    for kind in MASKS:
        out += [(4099, 40, kind), (1000, 7, kind)]
    return sorted(set(out))


def bern_case_list():
    out = []
    for i, (n, C) in enumerate(BERN_SHAPES):
        out.append((n, C, MASKS[i % len(MASKS)]))
        out.append((n, C, MASKS[(i + 4) % len(MASKS)]))
    for kind in MASKS:
        out.append((1000, 121, kind))
    return sorted(set(out))


def count_of(mask, n):
    return n if mask is None else int(np.asarray(mask).sum())


# ---- exact edges -----------------------------------------------------------------------------------------------------
def _f32(x):
    return np.float32(x)


def edge_categorical():
    """(p float32 [10, 4], y int64 [10], inside bool [10]: the rows whose q is inside the clamp window): p_y = 0, a
    one-hot row, q at eps, at 1 - eps and at the representable neighbours of both.  Every row has at most two non-zero
    entries besides exact cases, so its fp32 sum is the same in any order; where the sum is not exact (the neighbours
    of eps) fp32 and float64 still put q on the same side of the window."""
    eps = _f32(EPS)
    below, above = np.nextafter(eps, _f32(0)), np.nextafter(eps, _f32(1))
    hi = _f32(1) - eps
    u = _f32(2.0 ** -24)
    rows = [
        ([0.0, 0.5, 0.25, 0.25], 0, False),               # p_y = 0: -log(eps), gradient 0
        ([0.0, 2.0, 0.0, 0.0], 1, False),                 # one-hot (q = 1): -log(1 - eps), gradient 0
        ([below, _f32(1) - u, 0.0, 0.0], 0, False),       # s = 1 in fp32, q = pred(eps): clamped, gradient 0
        ([eps, 0.5, _f32(0.5) - eps, 0.0], 0, True),      # s = 1 exactly, q == eps: inside
        ([above, hi, 0.0, 0.0], 0, True),                 # s = 1 in fp32, q = succ(eps): inside
        ([_f32(1) - 3 * u, 3 * u, 0.0, 0.0], 0, True),    # s = 1 exactly, q = pred(1 - eps): inside
        ([hi, eps, 0.0, 0.0], 0, True),                   # s = 1 exactly, q == 1 - eps: inside
        ([_f32(1) - u, u, 0.0, 0.0], 0, False),           # s = 1 exactly, q = succ(1 - eps): clamped, gradient 0
        ([0.25, 0.25, 0.25, 0.25], 3, True),              # ordinary rows next to them
        ([0.5, 0.25, 0.125, 0.125], 1, True),
    ]
    p = np.array([r for r, _, _ in rows], np.float32)
    y = np.array([c for _, c, _ in rows], np.int64)
    return p, y, np.array([i for _, _, i in rows], bool)


def edge_bernoulli():
    """(p float32 [2, 6], y float32 [2, 6]): p in {0, 1, eps, 1 - eps, 0.5, 0.25} against y = 0 and y = 1"""
    eps = _f32(EPS)
    row = [0.0, 1.0, eps, _f32(1) - eps, 0.5, 0.25]
    p = np.array([row, row], np.float32)
    y = np.array([[0.0] * 6, [1.0] * 6], np.float32)
    return p, y
