"""Mesh moments on the CPU (no GPU, nothing of the library): what aq_mesh_moments_batch must return, restated in
numpy from a batch's node arrays ALONE -- offsets, x, f -- and exact sums of the restated terms as Fractions.

The term of one panel is include/aquad.h's sequence, one IEEE double operation per line (numpy fuses nothing); the
range rule is the header's: NaN rows, +0.0 rows, aq_mesh_eval's panel and value at lo and hi, a q at a node taking the
node's stored f. Also: the exact rational value of a term's integral and its bound (3k + 8) 2^-53 T_k, in integer
arithmetic; the formulas of Context.mesh_stats and Context.mesh_tail_mean; and a synthetic batch whose rows sit at the
wave, chunk and blocks-per-row edges of the kernel.

A helper module, not a conftest: the CPU and GPU tests import it and share its cached results.
"""
import functools
import types
from fractions import Fraction

import numpy as np

MAX_ORDER = 4
MESH_T, BLOCKS_PER_ROW = 256, 8           # the kernel's chunk of leaves and its blocks per row
NAN, ZERO, SUM = 0, 1, 2                  # what a row's outputs are


def terms(x0, x1, g0, g1, c, K):
    """t_0 .. t_K of panels (arrays or scalars): the header's sequence, line for line."""
    x0, x1, g0, g1 = (np.asarray(v, np.float64) for v in (x0, x1, g0, g1))
    c = np.float64(c)
    u0 = x0 - c
    u1 = x1 - c
    w = x1 - x0
    p0, p1 = [np.ones_like(u0)], [np.ones_like(u1)]
    for i in range(1, K + 1):
        p0.append(p0[i - 1] * u0)
        p1.append(p1[i - 1] * u1)
    out = []
    for k in range(K + 1):
        s0, s1 = np.zeros_like(u0), np.zeros_like(u0)
        for j in range(k + 1):
            a = p0[k - j] * p1[j]
            s0 = s0 + np.float64(k + 1 - j) * a
            s1 = s1 + np.float64(j + 1) * a
        out.append((g0 * s0 + g1 * s1) * w / np.float64((k + 1) * (k + 2)))
    return out


def panel_of(x, q):
    """aq_mesh_eval's rule: the largest k <= m - 1 with x_k <= q."""
    return int(np.clip(np.searchsorted(x, q, "right") - 1, 0, x.size - 2))


def value_at(x, f, k, q):
    """The interpolant at q in panel k: the node's stored f at a node, else aq_mesh_eval's expression."""
    if q == x[k]:
        return f[k]
    if q == x[k + 1]:
        return f[k + 1]
    return f[k] + (f[k + 1] - f[k]) * ((q - x[k]) / (x[k + 1] - x[k]))


def clip(x, f, lo=None, hi=None):
    """(state, x0, x1, g0, g1): the panels of one row in the range, clipped, in x order (empty unless state == SUM)."""
    none = (np.empty(0),) * 4
    if x.size < 3:
        return (NAN,) + none
    lo = x[0] if lo is None else np.float64(lo)
    hi = x[-1] if hi is None else np.float64(hi)
    if not (x[0] <= lo and lo <= hi and hi <= x[-1]):
        return (NAN,) + none
    if lo == hi:
        return (ZERO,) + none
    kl, kh = panel_of(x, lo), panel_of(x, hi)
    if kh > kl and hi == x[kh]:
        kh -= 1                            # hi at a node: the panel that ends there
    x0, x1 = x[kl:kh + 1].copy(), x[kl + 1:kh + 2].copy()
    g0, g1 = f[kl:kh + 1].copy(), f[kl + 1:kh + 2].copy()
    flo, fhi = value_at(x, f, kl, lo), value_at(x, f, kh, hi)       # always from the full panel's two nodes
    x0[0], g0[0] = lo, flo
    x1[-1], g1[-1] = hi, fhi
    return SUM, x0, x1, g0, g1


def exact_sum(v):
    """The exact sum of finite doubles, a Fraction (integer arithmetic at the smallest exponent among them)."""
    v = np.asarray(v, np.float64)
    v = v[v != 0.0]
    if v.size == 0:
        return Fraction(0)
    assert np.all(np.isfinite(v))
    m, e = np.frexp(v)
    mi, e = np.ldexp(m, 53).astype(np.int64), e.astype(np.int64) - 53
    emin = int(e.min())
    total = sum(int(a) << int(b - emin) for a, b in zip(mi, e))
    return Fraction(total) * Fraction(2) ** emin


def _arg(v, i):
    return None if v is None else (v[i] if np.ndim(v) else v)


def rows_of(batch):
    for i in range(len(batch.offsets) - 1):
        o0, o1 = int(batch.offsets[i]), int(batch.offsets[i + 1])
        yield i, batch.x[o0:o1], batch.f[o0:o1]


def moments_exact(batch, K, c=None, lo=None, hi=None):
    """Per row (state, S, A, P): S[k] the exact sum of the row's double terms t_k, A[k] the exact sum of |t_k|
    (Fractions), P the panels in range. c, lo, hi: None, a float, or an array (n,)."""
    out = []
    for i, x, f in rows_of(batch):
        state, x0, x1, g0, g1 = clip(x, f, _arg(lo, i), _arg(hi, i))
        if state != SUM:
            out.append((state, [Fraction(0)] * (K + 1), [Fraction(0)] * (K + 1), 0))
            continue
        ci = _arg(c, i)
        with np.errstate(over="raise", invalid="raise", divide="raise"):
            T = terms(x0, x1, g0, g1, 0.0 if ci is None else ci, K)
        out.append((state, [exact_sum(t) for t in T], [exact_sum(np.abs(t)) for t in T], x0.size))
    return out


def moments(batch, K, c=None, lo=None, hi=None):
    """The correctly rounded moments (n, K + 1): NaN rows, +0.0 rows, else the exact sums rounded once."""
    ex = moments_exact(batch, K, c, lo, hi)
    out = np.full((len(ex), K + 1), np.nan)
    for i, (state, S, _, _) in enumerate(ex):
        if state != NAN:
            out[i] = [float(s) for s in S]
    return out


def middles(batch):
    """The middle of every row's [x_0, x_m] (0.0 for a row without nodes)."""
    return np.array([0.5 * (x[0] + x[-1]) if x.size else 0.0 for _, x, _ in rows_of(batch)])


def bound(got, S, A, P):
    """|got - S| <= P 2^-100 sum|t| + ulp(S) / 2: the double-double sum's bound and its one rounding. Returns
    (within, deviation / bound)."""
    b = P * Fraction(2) ** -100 * A + Fraction(float(np.spacing(abs(float(S))))) / 2
    dev = abs(Fraction(float(got)) - S)
    return dev <= b, float(dev / b)


# ---- a term against the exact rational value of its integral ------------------------------------------------------
def _ints(v, s):
    return np.array([int(t) for t in np.ldexp(np.asarray(v, np.float64), s)], dtype=object)


def _scale(*arrays):
    """s such that every value of the arrays times 2^s is an integer."""
    e = [np.frexp(a[a != 0.0])[1] for a in (np.asarray(v, np.float64).ravel() for v in arrays)]
    e = np.concatenate(e) if e else np.empty(0)
    return 53 - int(e.min()) if e.size else 0


def term_ratios(x0, x1, g0, g1, c, K):
    """For panels (arrays) and one centre: per k the array of |t_k - exact| / (2^-53 T_k), T_k = w (|g0| + |g1|)
    max(|u0|, |u1|)^k / 2, the exact value being that of the same integral over the rationals -- (g0 s0 + g1 s1) w /
    ((k + 1)(k + 2)) with exact u0, u1, w -- in integer arithmetic. Panels with T_k == 0 must have t_k == 0 (ratio 0).
    The first-order bound is 3k + 8."""
    x0, x1, g0, g1 = (np.asarray(v, np.float64) for v in (x0, x1, g0, g1))
    T = terms(x0, x1, g0, g1, c, K)
    sx, sf = _scale(x0, x1, np.float64(c)), _scale(g0, g1)
    X0, X1, G0, G1 = _ints(x0, sx), _ints(x1, sx), _ints(g0, sf), _ints(g1, sf)
    C = int(np.ldexp(np.float64(c), sx))
    U0, U1, W = X0 - C, X1 - C, X1 - X0
    UM = np.maximum(abs(U0), abs(U1))
    out = []
    for k in range(K + 1):
        D = (k + 1) * (k + 2)
        S0 = sum((k + 1 - j) * U0 ** (k - j) * U1 ** j for j in range(k + 1))
        S1 = sum((j + 1) * U0 ** (k - j) * U1 ** j for j in range(k + 1))
        N = (G0 * S0 + G1 * S1) * W                      # the exact value is N / (D 2^S)
        TN = W * (abs(G0) + abs(G1)) * UM ** k           # T_k = TN / (2 2^S)
        S = sf + (k + 1) * sx
        assert np.all(np.isfinite(T[k]))
        m, e = np.frexp(T[k])
        mt = [int(v) for v in np.ldexp(m, 53)]
        sh = [int(v) - 53 + S for v in e]                # t_k 2^S = mt 2^sh
        z = max(0, -min(sh)) if sh else 0
        r = np.zeros(x0.size)
        for p in range(x0.size):
            E = abs(((mt[p] * D) << (sh[p] + z)) - (int(N[p]) << z))      # |t_k - exact| D 2^(S + z)
            den = int(TN[p]) * D << z                                      # 2 T_k D 2^(S + z)
            if den == 0:
                assert E == 0
            else:
                r[p] = (E << 54) / den
        out.append(r)
    return out


def panels(x, f):
    return x[:-1], x[1:], f[:-1], f[1:]


# ---- Context.mesh_stats and Context.mesh_tail_mean, restated ------------------------------------------------------
def centre_from(first):
    """Pass 1: c = M_1 / M_0 of an order-1 call about 0."""
    with np.errstate(all="ignore"):
        return first[:, 1] / first[:, 0]


def stats(c, M):
    """Pass 2 from the order-4 moments M (n, 5) about c: (mass, mean, var, skew, kurt), and per output the largest
    absolute intermediate of its formula (NaN rows aside), every operation one float64 operation, left to right."""
    with np.errstate(all="ignore"):
        mass = M[:, 0].copy()
        m1, m2, m3, m4 = (M[:, k] / mass for k in range(1, 5))
        d = m1
        mean = c + d
        dd = d * d
        var = m2 - dd
        a3 = 3.0 * d
        b3 = a3 * m2
        c3 = 2.0 * d
        c3b = c3 * d
        c3c = c3b * d
        e3 = m3 - b3
        mu3 = e3 + c3c
        a4 = 4.0 * d
        b4 = a4 * m3
        c4 = 6.0 * d
        c4b = c4 * d
        c4c = c4b * m2
        d4 = 3.0 * d
        d4b = d4 * d
        d4c = d4b * d
        d4d = d4c * d
        e4 = m4 - b4
        f4 = e4 + c4c
        mu4 = f4 - d4d
        sd = np.sqrt(var)
        v15 = var * sd
        skew = mu3 / v15
        vv = var * var
        kurt = mu4 / vv
    big = lambda *v: np.max(np.abs(np.stack(v)), axis=0)   # noqa: E731
    scale = dict(mass=big(mass), mean=big(c, d, mean), var=big(m2, dd, var),
                 skew=big(m3, a3, b3, c3, c3b, c3c, e3, mu3, var, sd, v15, skew),
                 kurt=big(m4, a4, b4, c4, c4b, c4c, d4, d4b, d4c, d4d, e4, f4, mu4, var, vv, kurt))
    return dict(mass=mass, mean=mean, var=var, skew=skew, kurt=kurt), scale


def mesh_stats(batch, lo=None, hi=None):
    """Context.mesh_stats on correctly rounded moments."""
    c = centre_from(moments(batch, 1, None, lo, hi))
    return stats(c, moments(batch, MAX_ORDER, c, lo, hi))[0]


def tail_mean(M):
    """M_1 / M_0 of an order-1 call about 0 over [x_0, q] or [q, x_m]."""
    with np.errstate(all="ignore"):
        return M[:, 1] / M[:, 0]


# ---- batches -----------------------------------------------------------------------------------------------------
def as_batch(rows):
    """rows: (x, f) pairs, or None for a row without nodes."""
    nodes = [0 if r is None else r[0].size for r in rows]
    offsets = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
    x = np.concatenate([r[0] for r in rows if r is not None] + [np.empty(0)])
    f = np.concatenate([r[1] for r in rows if r is not None] + [np.empty(0)])
    return types.SimpleNamespace(offsets=offsets, x=x, f=f, n_nodes=int(offsets[-1]), n=len(rows),
                                 rows=[None if r is None else (np.asarray(r[0]), np.asarray(r[1])) for r in rows])


def of_reference(batch):
    """A mesh_batch_reference.Batch as a batch of this module (its rows' x and f)."""
    return as_batch([None if r is None else (r.x, r.f) for r in batch.rows])


def sub_batch(batch, rows):
    return as_batch([batch.rows[i] for i in rows])


# leaves per row: the wave (64), the chunk (MESH_T) and one round of a row's blocks (BLOCKS_PER_ROW * MESH_T), each
# with its neighbours; a row without nodes; two rounds and a leaf (4097). A row has an odd node count, so the offsets
# alternate behind the first row's 3 nodes: this order puts the rows of 64, 256, 2048, 4097, 257 and 2049 leaves at
# odd offsets.
SYNTH_LEAVES = (1, 64, 0, 2, 256, 63, 2048, 65, 4097, 255, 257, 2047, 2049)


@functools.lru_cache(maxsize=None)
def synthetic():
    rng = np.random.default_rng(20260521)
    rows = []
    for L in SYNTH_LEAVES:
        if L == 0:
            rows.append(None)
            continue
        m = 2 * L
        w = rng.uniform(0.5, 1.5, m) * (rng.uniform(2.0, 8.0) / m)
        x = rng.uniform(-3.0, 1.0) + np.concatenate([[0.0], np.cumsum(w)])
        assert np.all(np.diff(x) > 0)
        f = rng.standard_normal(m + 1) * np.exp(rng.uniform(-2.0, 2.0))     # both signs
        rows.append((x, f))
    return as_batch(rows)


def hand_made():
    """Three rows for the range rules: 2 leaves with nodes at the integers 0 .. 4; the zero-width row [1, 1]; 1 leaf."""
    return as_batch([(np.array([0.0, 1.0, 2.0, 3.0, 4.0]), np.array([1.0, -2.0, 3.0, 0.5, -1.5])),
                     (np.array([1.0, 1.0, 1.0]), np.array([2.0, 2.0, 2.0])),
                     (np.array([-1.0, 0.5, 2.0]), np.array([0.25, 4.0, -3.0]))])


@functools.lru_cache(maxsize=None)
def case(name):
    """The batch of a named case: mesh_batch_reference's four, or `synthetic`."""
    if name == "synthetic":
        return synthetic()
    import mesh_batch_reference as mbr
    return of_reference(mbr.case(name)[5])


def range_sets(batch, seed=7):
    """Per-row (lo, hi) arrays covering the range rules on any batch, a dict name -> (lo, hi, rows that must be NaN by
    construction): the row's own ends given explicitly; lo / hi at even and at odd nodes; both in one panel; lo in the first panel and hi
    in the last; lo == hi; and the invalid ranges lo < x_0, hi > x_m, lo > hi, NaN on every third row."""
    rng = np.random.default_rng(seed)
    n = batch.n
    x0 = np.array([r[0][0] if r is not None else 0.0 for r in batch.rows])
    xm = np.array([r[0][-1] if r is not None else 0.0 for r in batch.rows])
    none = np.array([r is None for r in batch.rows])

    def per_row(fn):
        lo, hi = x0.copy(), xm.copy()
        for i, r in enumerate(batch.rows):
            if r is not None:
                lo[i], hi[i] = fn(i, r[0])
        return lo, hi

    def node(x, parity, frac):
        k = int(frac * (x.size - 1))
        k -= (k - parity) % 2
        return x[min(max(k, parity), x.size - 1)]

    def inside(x, k, t):
        return x[k] + t * (x[k + 1] - x[k])

    sets = {}
    sets["ends"] = (x0.copy(), xm.copy(), none)
    sets["even_nodes"] = per_row(lambda i, x: (node(x, 0, 0.3), node(x, 0, 0.9))) + (none,)
    sets["odd_nodes"] = per_row(lambda i, x: (node(x, 1, 0.2), node(x, 1, 0.8))) + (none,)
    sets["lo_node_hi_inside"] = per_row(lambda i, x: (node(x, 1, 0.2), inside(x, x.size - 2, 0.4))) + (none,)
    sets["one_panel"] = per_row(lambda i, x: (lambda k: (inside(x, k, 0.25), inside(x, k, 0.75)))(
        int(rng.integers(0, x.size - 1)))) + (none,)
    sets["first_and_last"] = per_row(lambda i, x: (inside(x, 0, 0.5), inside(x, x.size - 2, 0.5))) + (none,)
    sets["empty"] = per_row(lambda i, x: (x[x.size // 2],) * 2) + (none,)
    third = (np.arange(n) % 3 == 1)
    bad = {"below": (lambda a, b: (np.nextafter(a, -np.inf), b)), "above": (lambda a, b: (a, np.nextafter(b, np.inf))),
           "reversed": (lambda a, b: (b, a)), "nan_lo": (lambda a, b: (np.nan, b)), "nan_hi": (lambda a, b: (a, np.nan))}
    for name, fn in bad.items():
        lo, hi = x0.copy(), xm.copy()
        for i in np.nonzero(third)[0]:
            lo[i], hi[i] = fn(x0[i], xm[i])
        sets[name] = (lo, hi, none | (third & (x0 != xm)))
    return sets
