"""The accepted mesh on the CPU, from the oracle alone (no GPU, nothing of the library): what aq_integrate_mesh
must return for a problem, and the numpy restatement of aq_mesh_eval's formula.

The tree is walked level by level with oracle.pyoracle.F and the expressions of oracle.pyoracle.level_step
(aquadPartA.c:185-191), keeping what level_step drops: every accepted record with F(mid) and its depth. Sorted by
l they give x, f and level; the running integral is formed exactly with fractions.Fraction (every double is a
rational) and rounded once per node, so it owes nothing to any summation order."""
import functools
from fractions import Fraction

import numpy as np

from oracle import pyoracle as O

COSH4, SIN_RECIP, USER = O.COSH4, O.SIN_RECIP, O.USER

# (name, integrand, a, b, eps): the smallest trees that reach every path of the mesh code (the sizes: oracle.integrate)
CASES = [
    ("cosh4_0_5_1e-6", COSH4, 0.0, 5.0, 1e-6),        # 34 068 leaves, 19 levels: narrow top + multi-block steps, multi-block scan
    ("cosh4_-3_2_1e-5", COSH4, -3.0, 2.0, 1e-5),      # 1 382 leaves, 14 levels: keys of both signs, one level past the narrow top
    ("sin_recip_1e-3_1_1e-5", SIN_RECIP, 1e-3, 1.0, 1e-5),   # 391 leaves on 14 different levels: a skewed tree
    ("gauss_-4_4_1e-7", USER, -4.0, 4.0, 1e-7),       # 564 leaves, 11 levels: the whole tree inside the narrow kernel
    ("cosh4_root_leaf", COSH4, 0.0, 1e-3, 1.0),       # the root accepts: 3 nodes
]


class Mesh:
    """x, f, cum (float64, 2 * leaves + 1), level (uint8, 2 * leaves), the counts, and the leaves themselves."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def reference_mesh(integrand, a, b, eps, max_depth=96):
    fin = np.array([[a, b, O.F(float(a), integrand), O.F(float(b), integrand)]], np.float64)
    kept, tasks, depth = [], 0, 0
    while fin.shape[0]:
        assert depth + 1 < max_depth, "the reference mesh is for trees that end"
        l, r, fl, fr = fin[:, 0], fin[:, 1], fin[:, 2], fin[:, 3]
        mid = (l + r) / 2                                   # :187
        fmid = O.F(mid, integrand)                          # :188
        lrarea = (fl + fr) * (r - l) / 2                    # :185
        larea = (fl + fmid) * (mid - l) / 2                 # :189
        rarea = (fmid + fr) * (r - mid) / 2                 # :190
        ref = np.abs((larea + rarea) - lrarea) > eps        # :191
        acc = ~ref
        kept.append(np.stack([l, r, fl, fmid, fr, mid, larea, rarea, np.full(l.shape, float(depth))], axis=1)[acc])
        kids = np.empty((2 * int(ref.sum()), 4), np.float64)
        kids[0::2] = np.stack([l[ref], mid[ref], fl[ref], fmid[ref]], axis=1)
        kids[1::2] = np.stack([mid[ref], r[ref], fmid[ref], fr[ref]], axis=1)
        tasks += fin.shape[0]
        fin = kids
        depth += 1
    lv = np.concatenate(kept)
    lv = lv[np.argsort(lv[:, 0], kind="stable")]
    n = lv.shape[0]
    x = np.empty(2 * n + 1)
    f = np.empty(2 * n + 1)
    x[0:-1:2], x[1::2], x[-1] = lv[:, 0], lv[:, 5], lv[-1, 1]
    f[0:-1:2], f[1::2], f[-1] = lv[:, 2], lv[:, 3], lv[-1, 4]
    level = np.repeat(lv[:, 8].astype(np.uint8), 2)
    cum = np.empty(2 * n + 1)
    P = Fraction(0)
    for j in range(n):
        cum[2 * j] = float(P)                               # (Fraction -> float rounds correctly)
        cum[2 * j + 1] = float(P + Fraction(float(lv[j, 6])))
        P += Fraction(float(lv[j, 6] + lv[j, 7]))           # :199: the reference's own double
    cum[2 * n] = float(P)
    for arr in (x, f, cum, level):
        arr.setflags(write=False)
    return Mesh(x=x, f=f, cum=cum, level=level, tasks=tasks, accepted=n, levels=depth, l=lv[:, 0], r=lv[:, 1],
                total=P)


def mesh_eval(x, f, cum, q):
    """aq_mesh_eval restated: one IEEE operation per step (numpy fuses nothing); NaN outside [x_0, x_m] and for NaN."""
    x, f, cum, q = (np.asarray(v, np.float64) for v in (x, f, cum, q))
    m = x.size - 1
    k = np.clip(np.searchsorted(x, q, "right") - 1, 0, m - 1)
    with np.errstate(invalid="ignore"):
        h = q - x[k]
        w = x[k + 1] - x[k]
        fq = f[k] + (f[k + 1] - f[k]) * (h / w)
        out = cum[k] + (f[k] + fq) * h / 2
        out[~((q >= x[0]) & (q <= x[m]))] = np.nan
    return out
