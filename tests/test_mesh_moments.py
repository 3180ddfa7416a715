"""Mesh moments without a GPU: the function declared, bound, exported and refusing a NULL context on the host; and the
CPU reference (tests/mesh_moments_reference.py), which the GPU tests compare with, checked against the exact rational
value of every term's integral, against the leaf areas the meshes were built from, for additivity over a split range
and for the range rules. (On the GPU: tests/test_gpu_mesh_moments.py.)"""
import ctypes
import math
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mesh_batch_reference as mbr
import mesh_moments_reference as mm
import mesh_refine_reference as mrr

AQ_EINVAL = -1
NAME = "aq_mesh_moments_batch"
CASES = ["edges", "param", "sin", "scale"]
K = mm.MAX_ORDER


def test_declared_bound_exported_and_null_context_refused():
    from test_abi import HEADER, header_functions
    from ppls_amd import _lib
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aq_[a-z0-9_]+)$", out, flags=re.M))
    assert NAME in header_functions() and NAME in _lib.EXPORTS and NAME in exported
    assert getattr(lib, NAME).restype is ctypes.c_int
    # (never dereferenced: the context comes first)
    assert lib.aq_mesh_moments_batch(None, 1, 8, 8, 8, 2, None, None, None, 8) == AQ_EINVAL
    assert lib.aq_mesh_moments_batch(None, 0, None, None, None, 2, None, None, None, None) == AQ_EINVAL
    assert _lib.AQ_MESH_MAX_MOMENT == K
    assert re.search(r"#define\s+AQ_MESH_MAX_MOMENT\s+4\b", open(HEADER).read())


def test_python_surface_is_exported():
    import ppls_amd
    for name in ("mesh_moments", "mesh_stats", "mesh_tail_mean"):
        assert hasattr(ppls_amd.Context, name)
    assert ppls_amd.MeshStats._fields == ("mass", "mean", "var", "skew", "kurt")


def test_synthetic_batch_sits_at_the_kernels_edges():
    b = mm.synthetic()
    T, B = mm.MESH_T, mm.BLOCKS_PER_ROW
    leaves = [0 if r is None else (r[0].size - 1) // 2 for r in b.rows]
    assert sorted(leaves) == sorted([0, 1, 2, 63, 64, 65, T - 1, T, T + 1, B * T - 1, B * T, B * T + 1, 2 * B * T + 1])
    for i, r in enumerate(b.rows):
        if r is not None:
            assert r[0].size == 2 * leaves[i] + 1 and np.all(np.diff(r[0]) > 0) and (r[1] > 0).any() and (r[1] < 0).any()
    odd = {leaves[i] for i in range(b.n) if b.offsets[i] % 2 == 1}
    assert {64, T, B * T, 2 * B * T + 1} <= odd


@pytest.mark.parametrize("name", CASES + ["synthetic"])
def test_terms_against_the_exact_integral(name):
    """Every panel's computed t_k against the exact rational value of the same integral: within (3k + 8) 2^-53 T_k,
    the first-order bound of the sequence, for the centres 0 and the row's middle."""
    b = mm.case(name)
    worst = np.zeros(K + 1)
    for i, x, f in mm.rows_of(b):
        if x.size < 3:
            continue
        for c in (0.0, 0.5 * (x[0] + x[-1])):
            r = mm.term_ratios(*mm.panels(x, f), c, K)
            worst = np.maximum(worst, [v.max() if v.size else 0.0 for v in r])
    print(name, "worst |t_k - exact| / (2^-53 T_k), k = 0 .. 4:", " ".join("%.2f" % v for v in worst))
    for k in range(K + 1):
        assert worst[k] <= 3 * k + 8, (k, worst[k])


@pytest.mark.parametrize("name", CASES)
def test_m0_is_the_sum_of_the_leaf_areas(name):
    """Whole-row M_0 sums larea and rarea unrounded, cum sums the one rounding of larea + rarea: the two lie within
    2^-53 sum|larea_j + rarea_j| of each other, plus the half ulp of area_sums's own rounding."""
    ref = mbr.case(name)[5]
    b = mm.case(name)
    area = mrr.area_sums(ref)
    ex = mm.moments_exact(b, 0)
    assert sum(e[0] == mm.NAN for e in ex) == ref.invalid_rows
    for i, (state, S, A, P) in enumerate(ex):
        lv = mrr.leaves_of(ref, i)
        if lv.shape[0] == 0:
            assert state == mm.NAN and np.isnan(area[i])
            continue
        _, larea, rarea = mrr.leaf_d(lv)
        if state == mm.ZERO:                       # the zero-width row [1, 1]
            assert area[i] == 0.0
            continue
        assert P == 2 * lv.shape[0]
        tol = Fraction(2) ** -53 * mm.exact_sum(np.abs(larea + rarea)) + Fraction(float(np.spacing(abs(area[i])))) / 2
        assert abs(S[0] - Fraction(float(area[i]))) <= tol, i


def _term_bound(x0, x1, g0, g1, c, k):
    x0, x1, g0, g1, c = (Fraction(float(v)) for v in (x0, x1, g0, g1, c))
    T = (x1 - x0) * (abs(g0) + abs(g1)) * max(abs(x0 - c), abs(x1 - c)) ** k / 2
    return (3 * k + 8) * Fraction(2) ** -53 * T


@pytest.mark.parametrize("name", CASES + ["synthetic"])
def test_additivity(name):
    """M_k[lo, q] + M_k[q, hi] against M_k[lo, hi], as exact sums of the terms. With q at a node both sides hold the
    same terms: equal. With q inside a panel they differ in that panel's term and its two pieces': within the sum of
    the three term bounds."""
    b = mm.case(name)
    rows = [i for i, x, _ in mm.rows_of(b) if x.size >= 3 and x[0] < x[-1]]
    rows = rows[:: max(1, len(rows) // 6)]
    one = lambda i: mm.sub_batch(b, [i])                                        # noqa: E731
    for i in rows:
        x, f = b.rows[i]
        c = 0.5 * (x[0] + x[-1])
        whole = mm.moments_exact(one(i), K, c)[0]
        for p in {0, (x.size - 1) // 2, x.size - 2}:
            for q, at_node in ((x[p + 1] if p + 1 < x.size - 1 else x[p], True), (x[p] + 0.375 * (x[p + 1] - x[p]), False)):
                if not x[0] < q < x[-1]:
                    continue
                left, right = mm.moments_exact(one(i), K, c, None, q)[0], mm.moments_exact(one(i), K, c, q, None)[0]
                assert left[0] == right[0] == mm.SUM and left[3] + right[3] == whole[3] + (0 if at_node else 1)
                for k in range(K + 1):
                    dev = abs(left[1][k] + right[1][k] - whole[1][k])
                    if at_node:
                        assert dev == 0
                        continue
                    fq = mm.value_at(x, f, p, q)
                    tol = (_term_bound(x[p], q, f[p], fq, c, k) + _term_bound(q, x[p + 1], fq, f[p + 1], c, k) +
                           _term_bound(x[p], x[p + 1], f[p], f[p + 1], c, k))
                    assert dev <= tol, (i, p, k, float(dev), float(tol))


def test_range_rules_on_a_hand_made_batch():
    b = mm.hand_made()
    nan = np.nan

    def M(lo, hi, c=None, order=2):
        return mm.moments(b, order, c, np.array(lo, np.float64), np.array(hi, np.float64))

    def hat(x0, x1, g0, g1, k=0):
        """The exact integral of x^k g over one panel (Fractions)."""
        x0, x1, g0, g1 = (Fraction(v) for v in (x0, x1, g0, g1))
        s0 = sum((k + 1 - j) * x0 ** (k - j) * x1 ** j for j in range(k + 1))
        s1 = sum((j + 1) * x0 ** (k - j) * x1 ** j for j in range(k + 1))
        return (g0 * s0 + g1 * s1) * (x1 - x0) / ((k + 1) * (k + 2))

    # NaN rows: lo < x_0, hi > x_m, lo > hi, NaN; the neighbours are what they are without them
    base = M([0.0, 1.0, -1.0], [4.0, 1.0, 2.0])
    assert np.array_equal(base, mm.moments(b, 2)) and np.all(base[1] == 0.0) and not np.signbit(base[1]).any()
    for lo, hi in (([-0.5, 1, -1], [4, 1, 2]), ([0, 1, -1], [4.5, 1, 2]), ([3, 1, -1], [2, 1, 2]), ([nan, 1, -1], [4, 1, 2]),
                   ([0, 1, -1], [nan, 1, 2])):
        got = M(lo, hi)
        assert np.isnan(got[0]).all() and np.array_equal(got[1:], base[1:])
    # the zero-width row: any range but [1, 1] is invalid
    assert np.isnan(M([0, 0.5, -1], [4, 1, 2])[1]).all() and np.isnan(M([0, 1, -1], [4, 1.5, 2])[1]).all()
    # a row of fewer than 3 nodes
    short = mm.as_batch([(np.array([0.0, 1.0]), np.array([1.0, 1.0])), None])
    assert np.isnan(mm.moments(short, 1)).all()
    # lo == hi: +0.0, at a node and inside a panel
    for q in (0.0, 2.0, 2.5, 4.0):
        got = M([q, 1, 0.5], [q, 1, 0.5])
        assert np.all(got == 0.0) and not np.signbit(got).any()
    # lo and hi at even and odd nodes: the stored f, whole panels. Every value is a small dyadic, so M_0 is exact and
    # M_1, M_2 (a division by 6 or 12 per term, values of a few units) lie within a few ulp of 1
    for lo, hi in ((0, 2), (2, 4), (1, 3), (1, 4), (0, 3)):
        got = M([lo, 1, -1], [hi, 1, 2])[0]
        x, f = b.rows[0]
        for k in range(3):
            want = sum(hat(x[p], x[p + 1], f[p], f[p + 1], k) for p in range(lo, hi))
            assert abs(Fraction(float(got[k])) - want) <= (0 if k == 0 else Fraction(2) ** -48), (lo, hi, k)
    st, x0, x1, g0, g1 = mm.clip(*b.rows[0], 1.0, 3.0)
    assert st == mm.SUM and np.array_equal(x0, [1, 2]) and np.array_equal(x1, [2, 3]) and np.array_equal(g1, [3.0, 0.5])
    # both in one panel: one clipped panel, both ends interpolated from the full panel's nodes
    st, x0, x1, g0, g1 = mm.clip(*b.rows[0], 2.25, 2.75)
    assert st == mm.SUM and (x0, x1) == (2.25, 2.75) and (g0, g1) == (3.0 - 2.5 * 0.25, 3.0 - 2.5 * 0.75)
    assert abs(Fraction(float(M([2.25, 1, -1], [2.75, 1, 2])[0][1])) - hat(2.25, 2.75, g0[0], g1[0], 1)) <= Fraction(2) ** -50
    # lo in the first panel and hi in the last: two clipped panels and the whole ones between
    st, x0, x1, g0, g1 = mm.clip(*b.rows[0], 0.5, 3.5)
    assert np.array_equal(x0, [0.5, 1, 2, 3]) and np.array_equal(x1, [1, 2, 3, 3.5])
    assert np.array_equal(g0, [-0.5, -2, 3, 0.5]) and np.array_equal(g1, [-2, 3, 0.5, -0.5])
    # hi at a node ends the panel before it: no zero-width panel
    assert mm.clip(*b.rows[0], 0.5, 2.0)[1].size == 2 and mm.moments_exact(b, 0, None, np.array([0.5, 1, -1]), np.array([2.0, 1, 2]))[0][3] == 2
    # a centre: M_1 about c is M_1 - c M_0, within a few ulp of 1 here
    c = np.array([2.0, 0.0, 0.5])
    got, about0 = mm.moments(b, 1, c), mm.moments(b, 1)
    assert np.array_equal(got[:, 0], about0[:, 0]) and np.all(np.abs(got[:, 1] - (about0[:, 1] - c * about0[:, 0])) <= 2.0 ** -48)


def test_stats_of_the_reference_on_param():
    """How far mesh_stats of the reference mesh lies from the Gaussian's analytic values -- mass sqrt(pi) / s, mean mu,
    variance 1 / (2 s^2), skew 0, kurtosis 3 -- and, for mass, mean and variance, from those of the same Gaussian cut
    to the row's own [a, b] (every row of the case ends within 4 / s = 5.7 sigma of mu, most much closer, so the cut
    dominates the first figure; the second is the discretisation error of the piecewise-linear interpolant at that
    eps). Printed (DESIGN 2.14 records it), not asserted: no threshold can be derived."""
    integrand, a, b, theta, eps, ref = mbr.case("param")
    st = mm.mesh_stats(mm.case("param"))
    mu, s = theta[:, 0], theta[:, 1]
    full = dict(mass=math.sqrt(math.pi) / np.abs(s), mean=mu, var=1.0 / (2.0 * s * s), skew=np.zeros_like(mu),
                kurt=np.full_like(mu, 3.0))
    erf = np.vectorize(math.erf)
    ta, tb = (a - mu) * s, (b - mu) * s
    i0 = math.sqrt(math.pi) / 2 * (erf(tb) - erf(ta)) / s
    i1 = (np.exp(-ta * ta) - np.exp(-tb * tb)) / (2 * s * s)
    i2 = (math.sqrt(math.pi) / 4 * (erf(tb) - erf(ta)) - (tb * np.exp(-tb * tb) - ta * np.exp(-ta * ta)) / 2) / s ** 3
    cut = dict(mass=i0, mean=mu + i1 / i0, var=i2 / i0 - (i1 / i0) ** 2)
    for k in ("mass", "mean", "var", "skew", "kurt"):
        rel = k in ("mass", "var")
        dev = np.abs(st[k] - full[k]) / (np.abs(full[k]) if rel else 1.0)
        line = "param eps %g, %d rows: %s worst %s deviation from the whole Gaussian %.3g" % (
            eps, a.size, k, "relative" if rel else "absolute", dev.max())
        if k in cut:
            dev = np.abs(st[k] - cut[k]) / (np.abs(cut[k]) if rel else 1.0 / np.abs(s))
            line += "; from the Gaussian cut to [a, b] %.3g%s" % (dev.max(), "" if rel else " / s")
        print(line)
    assert np.all(np.isfinite(st["mass"])) and np.all(st["var"] > 0)
    # the restated formulas on exact inputs: a density that is 1 on [0, 1] (two panels)
    flat = mm.as_batch([(np.array([0.0, 0.5, 1.0]), np.array([1.0, 1.0, 1.0]))])
    got = mm.mesh_stats(flat)
    assert (got["mass"][0], got["mean"][0]) == (1.0, 0.5) and abs(got["var"][0] - 1 / 12) < 1e-16
    assert abs(got["skew"][0]) < 1e-14 and abs(got["kurt"][0] - 1.8) < 1e-13
    assert mm.tail_mean(mm.moments(flat, 1, None, None, 0.25))[0] == 0.125
