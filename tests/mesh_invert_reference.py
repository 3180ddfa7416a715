"""aq_mesh_invert restated in numpy (one IEEE operation per step: numpy fuses nothing, np.sqrt is correctly rounded,
np.fmin / np.fmax are C's), the meshes its tests run on, and the query sets. Shares nothing with the code under test;
the meshes are those of tests/mesh_reference.py."""
import numpy as np

import mesh_reference as mr

# the four monotone cases of mesh_reference.CASES, and a Gaussian far into its tails: 584 leaves, 5 panels of zero
# area (runs of equal cum) and two nodes with F = 0
MONOTONE = [c for c in mr.CASES if c[1] != mr.SIN_RECIP] + [("gauss_-30_30_1e-7", mr.USER, -30.0, 30.0, 1e-7)]
NON_MONOTONE = [c for c in mr.CASES if c[1] == mr.SIN_RECIP][0]


def mesh(case):
    return mr.reference_mesh(*case[1:])


def panel(cum, y):
    """k of aq_mesh_invert: the largest index <= m - 1 with cum_k <= y (cum non-decreasing, cum_0 <= y <= cum_m)."""
    return np.clip(np.searchsorted(cum, y, "right") - 1, 0, cum.size - 2)


def mesh_invert(x, f, cum, y):
    """NaN for y outside [cum_0, cum_m], for NaN, and where the panel found does not hold y."""
    x, f, cum, y = (np.asarray(v, np.float64) for v in (x, f, cum, y))
    m = x.size - 1
    inside = (y >= cum[0]) & (y <= cum[m])
    k = panel(cum, np.where(inside, y, cum[0]))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = x[k + 1] - x[k]
        r = y - cum[k]
        s = (f[k + 1] - f[k]) / w
        disc = np.fmax(f[k] * f[k] + (2 * s) * r, 0.0)
        den = f[k] + np.sqrt(disc)
        h = np.where(r == 0, 0.0, (2 * r) / den)
        h = np.fmin(h, w)
        out = x[k] + h
        out[~(inside & (cum[k] <= y) & (y <= cum[k + 1]))] = np.nan
    return out


def queries(cum, seed, n_random=8192):
    """Every cum node, every panel's midpoint in y, nextafter below every node (but the first), n_random uniform y."""
    rng = np.random.default_rng(seed)
    return np.concatenate([cum, 0.5 * (cum[:-1] + cum[1:]), np.nextafter(cum[1:], -np.inf),
                           rng.uniform(cum[0], cum[-1], n_random)])
