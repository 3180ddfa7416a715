"""Reference walker for the error estimate (the _err calls): the level-synchronous numpy walk of
tests/param_reference.py for any integrand, which also keeps every accepted task's difference
d = (larea + rarea) - lrarea -- the quantity the refine test bounds (aquadPartA.c:191).

F comes from the oracle's restated glibc functions (oracle.pyoracle.F for the fixed integrands,
param_reference.F for the AQ_F_PARAM Gaussian; numpy's own cosh is not pinned to glibc), every other
operation is one IEEE rounding in numpy as in the reference, so each d is the reference's own value.
The sums returned are math.fsum's: the correctly rounded exact sums of the leaf areas, of d and of |d|.

A helper module, not a conftest: the CPU and GPU tests import it and share its cached results.
"""
import functools
import math

import numpy as np

import param_reference as pr

MAXLEV = 128
PARAM = 3


def walk(a, b, eps, integrand, oracle, theta=None, maxlev=MAXLEV):
    """Per-integral tasks, leaves, levels and the math.fsum of the accepted areas ("area"), of d
    ("err_signed") and of |d| ("err_abs") over the accepted tasks of n integrals [a[i], b[i]] (theta[i] =
    {mu, s} for integrand PARAM)."""
    a = np.ascontiguousarray(a, np.float64).ravel()
    b = np.ascontiguousarray(b, np.float64).ravel()
    n = a.size
    if integrand == PARAM:
        theta = np.ascontiguousarray(theta, np.float64).reshape(n, 2)

        def F(x, i):
            return pr.F(x, theta[i, 0], theta[i, 1], oracle)
    else:
        assert theta is None

        def F(x, i):
            return oracle.F(x, integrand)
    idx = np.arange(n)
    l, r = a.copy(), b.copy()
    fl, fr = F(l, idx), F(r, idx)
    tasks = np.zeros(n, np.int64)
    leaves = np.zeros(n, np.int64)
    levels = np.zeros(n, np.int64)
    leaf_idx, leaf_area, leaf_d = [], [], []
    for depth in range(maxlev):
        if idx.size == 0:
            break
        lrarea = (fl + fr) * (r - l) / 2                 # :185
        mid = (l + r) / 2                                # :187
        fmid = F(mid, idx)                               # :188
        larea = (fl + fmid) * (mid - l) / 2              # :189
        rarea = (fmid + fr) * (r - mid) / 2              # :190
        d = (larea + rarea) - lrarea
        refine = np.abs(d) > eps                         # :191 (strict >)
        cnt = np.bincount(idx, minlength=n)
        tasks += cnt
        levels[cnt > 0] = depth + 1
        leaves += np.bincount(idx[~refine], minlength=n)
        leaf_idx.append(idx[~refine])
        leaf_area.append((larea + rarea)[~refine])       # :199
        leaf_d.append(d[~refine])
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
    order = np.argsort(li, kind="stable")
    li = li[order]
    la = np.concatenate(leaf_area)[order]
    ld = np.concatenate(leaf_d)[order]
    cuts = np.searchsorted(li, np.arange(n + 1))
    seg = [slice(cuts[i], cuts[i + 1]) for i in range(n)]
    out = {"tasks": tasks, "leaves": leaves, "levels": levels,
           "area": np.array([math.fsum(la[s]) for s in seg]),
           "err_signed": np.array([math.fsum(ld[s]) for s in seg]),
           "err_abs": np.array([math.fsum(np.abs(ld[s])) for s in seg])}
    for v in out.values():
        v.flags.writeable = False
    return out


def one(w, i=0):
    """Integral i of a walk as plain Python numbers."""
    return {k: (int(v[i]) if v.dtype.kind == "i" else float(v[i])) for k, v in w.items()}


def tol(w):
    """The bound on |device sum - walker sum| for either error sum of an integral (or of a walk's row i,
    elementwise): the device adds the walker's own terms in another order, and any order's error is at
    most (leaves - 1) * 2^-53 * err_abs to first order; twice that covers the second-order term and the
    staged partials (lane, wave, workgroup, slot)."""
    return w["leaves"] * 2.0 ** -52 * w["err_abs"]


@functools.lru_cache(maxsize=None)
def lone(integrand, a, b, eps, mu=None, s=None):
    """One integral's walk, computed once per process."""
    from oracle import pyoracle
    theta = None if mu is None else [[mu, s]]
    return one(walk([a], [b], eps, integrand, pyoracle, theta))


def lone_tree(tree):
    """A param_reference tree (a, b, mu, s, eps)."""
    return lone(PARAM, tree[0], tree[1], tree[4], tree[2], tree[3])


@functools.lru_cache(maxsize=None)
def draw_reference(n=5000):
    """param_reference.draw(n) walked at DRAW_EPS with the error sums."""
    from oracle import pyoracle
    a, b, theta = pr.draw(n)
    return a, b, theta, walk(a, b, pr.DRAW_EPS, PARAM, pyoracle, theta)


@functools.lru_cache(maxsize=None)
def batch_reference(n, eps):
    """n cosh^4 integrals on the oracle's batch bounds."""
    from oracle import pyoracle
    a, b = pyoracle.batch_bounds(n)
    return a, b, walk(a, b, eps, 0, pyoracle)


def cosh4_exact(x):
    """The integral of cosh^4 over [0, x]: 3x/8 + sinh(2x)/4 + sinh(4x)/32."""
    return 3.0 * x / 8.0 + math.sinh(2.0 * x) / 4.0 + math.sinh(4.0 * x) / 32.0
