"""The batch of meshes on the CPU, from the oracle alone (no GPU, nothing of the library): what
aq_integrate_mesh_batch must return for a set of rows, and numpy restatements of aq_mesh_eval_batch /
aq_mesh_invert_batch as per-row calls of the single-mesh restatements.

Per-row references: the fixed integrands' from mesh_reference.reference_mesh; AQ_F_PARAM's from a leaf-keeping
variant of param_reference.walk -- the same task body (aquadPartA.c:185-191), F = oracle.exp(-t * t) with
t = (x - mu) * s -- whose cum comes from exact Fraction prefixes rounded once per node. A row outside the domain
(the rule of include/aquad.h, restated here) has no nodes. The rows' nodes are concatenated at `offsets`.
"""
import functools
from fractions import Fraction

import numpy as np

import mesh_invert_reference as mir
import mesh_reference as mr
import param_reference as pr

COSH4, SIN_RECIP, USER, PARAM = mr.COSH4, mr.SIN_RECIP, mr.USER, 3
ROW_DEPTH, ROW_INVALID = 4, 8


def bounds_ok(integrand, a, b):
    """include/aquad.h's domain rule for one integral of a fixed integrand or of the PARAM engine."""
    if not (np.isfinite(a) and np.isfinite(b) and b >= a):
        return False
    m = max(abs(a), abs(b))
    if m > 2.0 ** 900 or (a != 0.0 and abs(a) < 2.0 ** -900) or (b != 0.0 and abs(b) < 2.0 ** -900):
        return False
    if integrand == COSH4:
        return m <= 170.0
    if integrand in (USER, PARAM):
        return a >= -1e150 and b <= 1e150
    return True


def params_ok(a, b, th):
    return bool(bounds_ok(PARAM, a, b) and np.all(np.isfinite(th)) and np.all(np.abs(th) <= 1e150) and th[1] != 0.0)


class Row:
    """One row's mesh: x, f, cum (2 * accepted + 1), level (2 * accepted), tasks, accepted, levels, and
    tasks_per_level (records of the row at every depth)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _levels_histogram(leaf_depths, levels):
    """Records per depth of a binary tree from its leaves' depths: t[0] = 1, t[d + 1] = 2 (t[d] - leaves[d])."""
    lv = np.bincount(leaf_depths, minlength=levels)
    t = np.zeros(levels, np.int64)
    t[0] = 1
    for d in range(levels - 1):
        t[d + 1] = 2 * (t[d] - lv[d])
    assert t[levels - 1] == lv[levels - 1]
    return t


@functools.lru_cache(maxsize=None)
def fixed_row(integrand, a, b, eps):
    m = mr.reference_mesh(integrand, a, b, eps)
    return Row(x=m.x, f=m.f, cum=m.cum, level=m.level, tasks=m.tasks, accepted=m.accepted, levels=m.levels,
               tasks_per_level=_levels_histogram(m.level[::2].astype(np.int64), m.levels))


def walk_leaves(a, b, theta, eps, oracle, maxlev=pr.MAXLEV):
    """param_reference.walk keeping every accepted record: rows of (idx, l, r, fl, fmid, fr, mid, larea, rarea,
    depth) in schedule order, and the per-integral per-level task counts [n, maxlev]."""
    a = np.ascontiguousarray(a, np.float64).ravel()
    b = np.ascontiguousarray(b, np.float64).ravel()
    theta = np.ascontiguousarray(theta, np.float64).reshape(a.size, 2)
    n = a.size
    mu, s = theta[:, 0], theta[:, 1]
    idx = np.arange(n)
    l, r = a.copy(), b.copy()
    fl, fr = pr.F(l, mu, s, oracle), pr.F(r, mu, s, oracle)
    tpl = np.zeros((n, maxlev), np.int64)
    kept = []
    for d in range(maxlev):
        if idx.size == 0:
            break
        lrarea = (fl + fr) * (r - l) / 2                 # :185
        mid = (l + r) / 2                                # :187
        fmid = pr.F(mid, mu[idx], s[idx], oracle)        # :188
        larea = (fl + fmid) * (mid - l) / 2              # :189
        rarea = (fmid + fr) * (r - mid) / 2              # :190
        refine = np.abs((larea + rarea) - lrarea) > eps  # :191 (strict >)
        tpl[:, d] = np.bincount(idx, minlength=n)
        acc = ~refine
        kept.append(np.stack([idx.astype(np.float64), l, r, fl, fmid, fr, mid, larea, rarea,
                              np.full(l.shape, float(d))], axis=1)[acc])
        k = np.nonzero(refine)[0]
        idx = np.repeat(idx[k], 2)
        nl, nr, nfl, nfr = (np.empty(2 * k.size) for _ in range(4))
        nl[0::2], nr[0::2], nfl[0::2], nfr[0::2] = l[k], mid[k], fl[k], fmid[k]     # [l, mid]  (:192-194)
        nl[1::2], nr[1::2], nfl[1::2], nfr[1::2] = mid[k], r[k], fmid[k], fr[k]     # [mid, r]  (:195-197)
        l, r, fl, fr = nl, nr, nfl, nfr
    else:
        if idx.size:
            raise RuntimeError("the walk did not end within maxlev levels")
    return np.concatenate(kept), tpl


def _row_from_leaves(lv, tpl_row):
    """lv: one integral's kept records (columns as walk_leaves), any order."""
    lv = lv[np.argsort(lv[:, 1], kind="stable")]
    n = lv.shape[0]
    x, f, cum = np.empty(2 * n + 1), np.empty(2 * n + 1), np.empty(2 * n + 1)
    x[0:-1:2], x[1::2], x[-1] = lv[:, 1], lv[:, 6], lv[-1, 2]
    f[0:-1:2], f[1::2], f[-1] = lv[:, 3], lv[:, 4], lv[-1, 5]
    level = np.repeat(lv[:, 9].astype(np.uint8), 2)
    P = Fraction(0)
    for j in range(n):
        cum[2 * j] = float(P)
        cum[2 * j + 1] = float(P + Fraction(float(lv[j, 7])))
        P += Fraction(float(lv[j, 7] + lv[j, 8]))        # :199: the reference's own double
    cum[2 * n] = float(P)
    levels = int((tpl_row > 0).sum())
    return Row(x=x, f=f, cum=cum, level=level, tasks=int(tpl_row.sum()), accepted=n, levels=levels,
               tasks_per_level=tpl_row[:levels].copy())


def param_rows(a, b, theta, eps):
    """The rows of a PARAM batch (every row valid)."""
    from oracle import pyoracle
    lv, tpl = walk_leaves(a, b, theta, eps, pyoracle)
    order = np.argsort(lv[:, 0], kind="stable")
    lv = lv[order]
    cuts = np.searchsorted(lv[:, 0], np.arange(len(a) + 1))
    return [_row_from_leaves(lv[cuts[i]:cuts[i + 1]], tpl[i]) for i in range(len(a))]


class Batch:
    """The concatenation aq_integrate_mesh_batch returns: offsets (n + 1), x, f, cum, level (n_nodes; level at a
    row's last node unspecified: `level_known` is False there), per-row area (NaN for an invalid row), accepted,
    tasks, status, and the run's leaves, tasks_total, levels, widest_level, invalid_rows, tasks_per_level."""

    def __init__(self, rows):
        """rows: a Row, or None for a row outside the domain."""
        n = len(rows)
        nodes = np.array([0 if r is None else r.x.size for r in rows], np.int64)
        self.rows = rows
        self.offsets = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
        self.n_nodes = int(self.offsets[-1])
        self.x, self.f, self.cum = (np.empty(self.n_nodes) for _ in range(3))
        self.level = np.zeros(self.n_nodes, np.uint8)
        self.level_known = np.zeros(self.n_nodes, bool)
        self.area = np.full(n, np.nan)
        self.accepted, self.tasks = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.status = np.zeros(n, np.int64)
        depth = max([r.levels for r in rows if r is not None], default=0)
        self.tasks_per_level = np.zeros(depth, np.int64)
        for i, r in enumerate(rows):
            if r is None:
                self.status[i] = ROW_INVALID
                continue
            o0, o1 = self.offsets[i], self.offsets[i + 1]
            self.x[o0:o1], self.f[o0:o1], self.cum[o0:o1] = r.x, r.f, r.cum
            self.level[o0:o1 - 1] = r.level
            self.level_known[o0:o1 - 1] = True
            self.area[i], self.accepted[i], self.tasks[i] = r.cum[-1], r.accepted, r.tasks
            self.tasks_per_level[:r.levels] += r.tasks_per_level
        self.leaves = int(self.accepted.sum())
        self.tasks_total = int(self.tasks.sum())
        self.levels = depth
        self.widest_level = int(self.tasks_per_level.max()) if depth else 0
        self.invalid_rows = int(sum(r is None for r in rows))
        for arr in (self.offsets, self.x, self.f, self.cum, self.level, self.area, self.accepted, self.tasks, self.status):
            arr.setflags(write=False)

    def depth_status(self, max_depth):
        """The status words of a run capped at max_depth: AQ_ROW_DEPTH on the rows with more levels than that."""
        st = self.status.copy()
        for i, r in enumerate(self.rows):
            if r is not None and r.levels > max_depth:
                st[i] |= ROW_DEPTH
        return st


def fixed_batch(integrand, a, b, eps):
    return Batch([fixed_row(integrand, float(x), float(y), eps) if bounds_ok(integrand, x, y) else None
                  for x, y in zip(a, b)])


# ---- the cases of tests/mesh_batch_cases.py (their shapes are asserted in tests/test_mesh_batch.py) -------------
EDGES_EPS = 1e-5
ONE_LEAF = 300                      # cosh^4 on [k 1e-3, (k + 1) 1e-3], k < 300: one leaf each
EDGES_TAIL = [(-3.0, 2.0), (1.0, 1.0), (2.0, 1.0), (0.0, 171.0), (0.0, 5.0), (-1.0, 0.5), (0.0, 0.25)]
SCALE_EPS = 1e163
SCALE_ROWS = [(100.0, 100.5), (0.0, 1.0), (-0.5, 0.25)]
SIN_EPS = 1e-5
SIN_ROWS = [(1e-3, 1.0), (0.01, 1.0), (0.5, 1.0)]
PARAM_N = 64


def edges_bounds():
    k = np.arange(ONE_LEAF, dtype=np.float64)
    a = np.concatenate([k * 1e-3, [r[0] for r in EDGES_TAIL]])
    b = np.concatenate([(k + 1) * 1e-3, [r[1] for r in EDGES_TAIL]])
    return a, b


@functools.lru_cache(maxsize=None)
def case(name):
    """(integrand, a, b, theta or None, eps, Batch) of a named case."""
    if name == "edges":
        a, b = edges_bounds()
        return COSH4, a, b, None, EDGES_EPS, fixed_batch(COSH4, a, b, EDGES_EPS)
    if name == "scale":
        a, b = (np.array(v) for v in zip(*SCALE_ROWS))
        return COSH4, a, b, None, SCALE_EPS, fixed_batch(COSH4, a, b, SCALE_EPS)
    if name == "sin":
        a, b = (np.array(v) for v in zip(*SIN_ROWS))
        return SIN_RECIP, a, b, None, SIN_EPS, fixed_batch(SIN_RECIP, a, b, SIN_EPS)
    if name == "param":
        a, b, theta = pr.draw(PARAM_N)
        return PARAM, a, b, theta, pr.DRAW_EPS, Batch(param_rows(a, b, theta, pr.DRAW_EPS))
    if name == "param_unit":   # the same bounds, every theta {0, 1}: the USER Gaussian's rows
        a, b, _ = pr.draw(PARAM_N)
        theta = np.tile([0.0, 1.0], (PARAM_N, 1))
        return PARAM, a, b, theta, pr.DRAW_EPS, Batch(param_rows(a, b, theta, pr.DRAW_EPS))
    if name == "param_one":
        ta, tb, mu, s, eps = pr.TREE_SHIFTED
        a, b, theta = np.array([ta]), np.array([tb]), np.array([[mu, s]])
        return PARAM, a, b, theta, eps, Batch(param_rows(a, b, theta, eps))
    raise KeyError(name)


# ---- the query calls, restated ----------------------------------------------------------------------------------
def _per_row(one, batch_offsets, x, f, cum, q):
    q = np.asarray(q, np.float64)
    out = np.full(q.shape, np.nan)
    for i in range(q.shape[0]):
        o0, o1 = int(batch_offsets[i]), int(batch_offsets[i + 1])
        if o1 - o0 >= 3:
            out[i] = one(x[o0:o1], f[o0:o1], cum[o0:o1], q[i])
    return out


def mesh_eval_batch(offsets, x, f, cum, q):
    """aq_mesh_eval_batch: row i's queries q[i] through mesh_reference.mesh_eval on the row's slice; NaN for a row of
    fewer than 3 nodes."""
    return _per_row(mr.mesh_eval, offsets, x, f, cum, q)


def mesh_invert_batch(offsets, x, f, cum, y):
    """aq_mesh_invert_batch: the same through mesh_invert_reference.mesh_invert (monotone rows)."""
    return _per_row(mir.mesh_invert, offsets, x, f, cum, y)


def queries(row_x, nq=257):
    """nq eval queries of one row: nodes, midpoints, both ends, two points outside and a NaN."""
    m = row_x.size
    take = (nq - 5) // 2
    k = np.unique(np.linspace(0, m - 2, take).astype(np.int64))
    q = np.concatenate([row_x[k], 0.5 * (row_x[k] + row_x[k + 1]), [row_x[0], row_x[-1]],
                        [row_x[0] - 1e-6, np.nextafter(row_x[-1], np.inf), np.nan]])
    return np.concatenate([q, np.full(nq - q.size, row_x[-1])])
