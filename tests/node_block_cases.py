"""Inputs and float64 references of the fused node block (tests/test_gpu_node_block.py); no device is used here."""
import numpy as np

# (N, D): N on either side of the 64-row slab (255, 256, 257: four slabs less one row, four, four and one row), one slab
# (2, 3) and many (1000, 4099); D scalar (1, 3, 5, 50, 1433) and 16-byte (4, 128, 132, 260) forms, one channel tile and
# several (260 and 1433: more than the 256 channels of a 64-lane team), and widths that leave lanes of a team idle
# (1, 3, 5, 50, 132)
SHAPES = [(2, 1), (3, 3), (255, 4), (256, 5), (257, 50), (1000, 128), (4099, 132), (257, 260), (3, 1433), (1000, 1433),
          (4099, 128), (2, 260)]
EPS = 1e-5


def inputs(N, D, seed):
    """x = +-1 + 0.1 N(0, 1) per entry, gamma in [0.5, 1.5], beta = 0.05, g ~ N(0, 1): no pre-activation sits near 0, so
    no ReLU decision flips under rounding (a flip moves the column sums by a whole term)."""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1.0, 1.0], size=(N, D))
    sign[0], sign[1] = 1.0, -1.0          # both signs in every column: a one-signed column of 2 or 3 rows has no variance
    x = (sign + 0.1 * rng.standard_normal((N, D))).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, D).astype(np.float32)
    beta = np.full(D, 0.05, np.float32)
    g = rng.standard_normal((N, D)).astype(np.float32)
    return x, gamma, beta, g


def stats(x):
    x = np.asarray(x, np.float64)
    return x.mean(0), x.var(0)


def block(x, mean, var, gamma, beta, relu, mask=None, keep=1.0, g=None, batch_stats=True, eps=EPS):
    """float64: dict(y, pre, xhat, rstd) and, with g, (dx, dgamma, dbeta, abs_dgamma, abs_dbeta: sum |terms|)."""
    x = np.asarray(x, np.float64)
    N, D = x.shape
    gamma = np.ones(D) if gamma is None else np.asarray(gamma, np.float64)
    beta = np.zeros(D) if beta is None else np.asarray(beta, np.float64)
    m = np.ones((N, D)) if mask is None else np.asarray(mask, np.float64)
    rstd = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    xhat = (x - mean) * rstd
    pre = xhat * gamma + beta
    out = {"xhat": xhat, "pre": pre, "rstd": rstd, "y": (np.maximum(pre, 0.0) if relu else pre) * m / keep}
    if g is not None:
        gp = np.asarray(g, np.float64) * m / keep
        if relu:
            gp = gp * (pre > 0)
        dbeta, dgamma = gp.sum(0), (gp * xhat).sum(0)
        out.update(gp=gp, dbeta=dbeta, dgamma=dgamma, abs_dbeta=np.abs(gp).sum(0), abs_dgamma=np.abs(gp * xhat).sum(0))
        out["dx"] = gamma * rstd * ((gp - dbeta / N - xhat * dgamma / N) if batch_stats else gp)
    return out
