"""Reference walker for the parametrised family (AQ_F_PARAM, default plug-in: the Gaussian {mu, s}).

A numpy level-synchronous walk over a batch of integrals with the reference's task body
(aquadPartA.c:185-191) token for token, one record per task, each record carrying its integral's index.
F(x; mu, s) = exp(-t * t) with t = (x - mu) * s: numpy's subtract / multiply / negate are single IEEE
roundings, and the exponential is the oracle's restated glibc one (oracle.pyoracle.exp), so every value
is the one the reference binary built with that F would compute. At theta = {0, 1} the walk reproduces the
oracle's USER (exp(-x*x)) trees exactly (tests/test_params.py), which the reference binary pins.

A helper module, not a conftest: the CPU and GPU tests import it and share its cached results.
"""
import functools
import math

import numpy as np

MAXLEV = 128


def F(x, mu, s, oracle):
    t = (x - mu) * s
    return oracle.exp(-t * t)


def walk(a, b, theta, eps, oracle, maxlev=MAXLEV):
    """Per-integral tasks, leaves, levels, per-level histograms [n, maxlev] and the math.fsum of the
    accepted areas (larea + rarea, :199) of n integrals [a[i], b[i]] with parameters theta[i] = {mu, s}."""
    a = np.ascontiguousarray(a, np.float64).ravel()
    b = np.ascontiguousarray(b, np.float64).ravel()
    theta = np.ascontiguousarray(theta, np.float64).reshape(a.size, 2)
    n = a.size
    mu, s = theta[:, 0], theta[:, 1]
    idx = np.arange(n)
    l, r = a.copy(), b.copy()
    fl, fr = F(l, mu, s, oracle), F(r, mu, s, oracle)
    tpl = np.zeros((n, maxlev), np.int64)
    lpl = np.zeros((n, maxlev), np.int64)
    leaf_idx, leaf_area = [], []
    for d in range(maxlev):
        if idx.size == 0:
            break
        lrarea = (fl + fr) * (r - l) / 2                 # :185
        mid = (l + r) / 2                                # :187
        fmid = F(mid, mu[idx], s[idx], oracle)           # :188
        larea = (fl + fmid) * (mid - l) / 2              # :189
        rarea = (fmid + fr) * (r - mid) / 2              # :190
        refine = np.abs((larea + rarea) - lrarea) > eps  # :191 (strict >)
        tpl[:, d] = np.bincount(idx, minlength=n)
        lpl[:, d] = np.bincount(idx[~refine], minlength=n)
        leaf_idx.append(idx[~refine])
        leaf_area.append((larea + rarea)[~refine])       # :199
        k = np.nonzero(refine)[0]
        idx = np.repeat(idx[k], 2)
        nl, nr, nfl, nfr = (np.empty(2 * k.size) for _ in range(4))
        nl[0::2], nr[0::2], nfl[0::2], nfr[0::2] = l[k], mid[k], fl[k], fmid[k]     # [l, mid]  (:192-194)
        nl[1::2], nr[1::2], nfl[1::2], nfr[1::2] = mid[k], r[k], fmid[k], fr[k]     # [mid, r]  (:195-197)
        l, r, fl, fr = nl, nr, nfl, nfr
    else:
        if idx.size:
            raise RuntimeError("the walk did not end within maxlev levels")
    li = np.concatenate(leaf_idx)
    la = np.concatenate(leaf_area)
    order = np.argsort(li, kind="stable")
    li, la = li[order], la[order]
    cuts = np.searchsorted(li, np.arange(n + 1))
    area = np.array([math.fsum(la[cuts[i]:cuts[i + 1]]) for i in range(n)])
    return {"tasks": tpl.sum(1), "leaves": lpl.sum(1), "levels": (tpl > 0).sum(1), "tasks_per_level": tpl,
            "leaves_per_level": lpl, "area": area}


def walk_one(a, b, mu, s, eps, oracle):
    """One integral: tasks, leaves, levels, the two histograms as lists, and the area."""
    w = walk([a], [b], [[mu, s]], eps, oracle)
    n = int(w["levels"][0])
    return {"tasks": int(w["tasks"][0]), "leaves": int(w["leaves"][0]), "levels": n,
            "tasks_per_level": [int(v) for v in w["tasks_per_level"][0, :n]],
            "leaves_per_level": [int(v) for v in w["leaves_per_level"][0, :n]], "area": float(w["area"][0])}


DRAW_SEED = 20240607
DRAW_EPS = 1e-6


def draw(n, seed=DRAW_SEED):
    """n integrals whose neighbours differ in theta AND in tree size: mu in [-2, 2], s = e^U(-2, 2),
    bounds mu - U(0, 4)/s .. mu + U(0.1, 4)/s (at DRAW_EPS: trees of tens to about a thousand tasks)."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-2.0, 2.0, n)
    s = np.exp(rng.uniform(-2.0, 2.0, n))
    a = mu - rng.uniform(0.0, 4.0, n) / s
    b = mu + rng.uniform(0.1, 4.0, n) / s
    return a, b, np.ascontiguousarray(np.stack([mu, s], axis=1))


@functools.lru_cache(maxsize=None)
def _draw_reference(n):
    from oracle import pyoracle
    a, b, theta = draw(n)
    w = walk(a, b, theta, DRAW_EPS, pyoracle)
    for v in (a, b, theta, *w.values()):
        v.flags.writeable = False
    return a, b, theta, w


def draw_reference(n=5000):
    """draw(n) and its walk at DRAW_EPS, computed once per process and shared (read-only arrays)."""
    return _draw_reference(n)


# the lone trees of the GPU tests: (a, b, mu, s, eps)
TREE_SHIFTED = (-2.0, 3.0, 0.3, 1.7, 1e-12)        # 42 637 tasks, 17 levels
TREE_WIDE_256 = (-256.0, 256.0, 0.0, 2.0 ** -6, 1e-12)   # 196 795 tasks, 19 levels
# the same Gaussian on [-2^20, 2^20]: 197 487 tasks, 31 levels, all but ~60 of them below two adjacent
# depth-9 positions -- one share of a 24-integral launch's 128, so one wave starts with the whole tree and the
# rest of the machine has to be fed from its ring (on [-256, 256] every wave of that launch got an even
# ~1 500-task share and nothing moved through the pool or the HBM queue: spilled = 0 on the MI355X)
TREE_WIDE = (-2.0 ** 20, 2.0 ** 20, 0.0, 2.0 ** -6, 1e-12)
TREE_UNIT = (0.0, 5.0, 0.0, 1.0, 1e-12)            # theta = {0, 1}: the AQ_F_USER Gaussian's tree


@functools.lru_cache(maxsize=None)
def tree_reference(tree):
    from oracle import pyoracle
    return walk_one(*tree[:4], tree[4], pyoracle)
