"""Mesh refinement on the CPU (no GPU, nothing of the library): what aq_mesh_refine_batch must return, restated in
numpy from a reference Batch's node arrays ALONE -- offsets, x, f, level -- as the call itself sees them.

Every leaf (nodes 2j .. 2j + 2 of its row) is retested with the task step's expressions (aquadPartA.c:185-191); a
survivor stays; a failing leaf's two children join the frontier of the next depth, which is walked on with
oracle.pyoracle.F (param_reference.F for PARAM) exactly as mesh_batch_reference walks a tree from its root. cum is
formed with fractions.Fraction and rounded once per node. The run's shape is kept beside the meshes: the failing
leaves, the depths that have seeds, the records of every level of THIS run, the task steps it ran.

Also the error sums of a mesh (aq_mesh_err_batch) as exact Fractions of the recomputed d, and the tolerance loop of
Context.integrate_mesh_batch_tol restated over these two.

A helper module, not a conftest: the CPU and GPU tests import it and share its cached results.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import mesh_batch_reference as mbr
import param_reference as pr

PARAM = mbr.PARAM


def leaves_of(batch, i):
    """Row i's leaves from the node arrays: columns l, r, fl, fmid, fr, mid, depth (none for a row without nodes)."""
    o0, o1 = int(batch.offsets[i]), int(batch.offsets[i + 1])
    if o1 - o0 < 3:
        return np.empty((0, 7))
    x, f, lv = batch.x[o0:o1], batch.f[o0:o1], batch.level[o0:o1]
    return np.stack([x[0:-1:2], x[2::2], f[0:-1:2], f[1::2], f[2::2], x[1::2], lv[0:-1:2].astype(np.float64)], axis=1)


def leaf_d(lv):
    """d = (larea + rarea) - lrarea of leaf records (columns as leaves_of), and larea, rarea."""
    l, r, fl, fmid, fr, mid = (lv[:, k] for k in range(6))
    lrarea = (fl + fr) * (r - l) / 2                     # :185
    larea = (fl + fmid) * (mid - l) / 2                  # :189
    rarea = (fmid + fr) * (r - mid) / 2                  # :190
    return (larea + rarea) - lrarea, larea, rarea        # :191


def _row(lv, with_cum=True):
    """A mesh_batch_reference.Row from leaf records in any order."""
    lv = lv[np.argsort(lv[:, 0], kind="stable")]
    n = lv.shape[0]
    x, f = np.empty(2 * n + 1), np.empty(2 * n + 1)
    x[0:-1:2], x[1::2], x[-1] = lv[:, 0], lv[:, 5], lv[-1, 1]
    f[0:-1:2], f[1::2], f[-1] = lv[:, 2], lv[:, 3], lv[-1, 4]
    level = np.repeat(lv[:, 6].astype(np.uint8), 2)
    _, larea, rarea = leaf_d(lv)
    cum = np.full(2 * n + 1, np.nan)
    if with_cum:
        P = Fraction(0)
        for j in range(n):
            cum[2 * j] = float(P)
            cum[2 * j + 1] = float(P + Fraction(float(larea[j])))
            P += Fraction(float(larea[j] + rarea[j]))    # :199: the reference's own double
        cum[2 * n] = float(P)
    levels = int(lv[:, 6].max()) + 1
    return mbr.Row(x=x, f=f, cum=cum, level=level, tasks=2 * n - 1, accepted=n, levels=levels,
                   tasks_per_level=mbr._levels_histogram(lv[:, 6].astype(np.int64), levels))


class Refined:
    """batch: the output meshes (a mesh_batch_reference.Batch); reseeded: the input leaves that failed; seed_depths:
    the depths at which children of failing leaves enter; level_records: records of every depth of this run;
    widest_level, evaluated: their maximum and sum; changed: the rows whose mesh differs from the input's."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def refine(batch, integrand, theta, eps, active=None, with_cum=True):
    from oracle import pyoracle
    n = len(batch.rows)
    theta = None if theta is None else np.ascontiguousarray(theta, np.float64).reshape(n, 2)

    def F(x, rows):
        if integrand == PARAM:
            return pr.F(x, theta[rows, 0], theta[rows, 1], pyoracle)
        return pyoracle.F(x, integrand)

    kept = [[] for _ in range(n)]
    seeds = {}            # depth -> list of (rows, l, r, fl, fr)
    reseeded, changed = 0, []
    for i in range(n):
        lv = leaves_of(batch, i)
        if lv.shape[0] == 0:
            continue
        d, _, _ = leaf_d(lv)
        fail = (np.abs(d) > eps) if (active is None or active[i]) else np.zeros(lv.shape[0], bool)
        kept[i].append(lv[~fail])
        if fail.any():
            changed.append(i)
            reseeded += int(fail.sum())
            for dep in np.unique(lv[fail, 6]):
                k = fail & (lv[:, 6] == dep)
                l, r, fl, fmid, fr, mid = (lv[k, c] for c in range(6))
                kids = np.empty((2 * int(k.sum()), 5))
                kids[0::2] = np.stack([np.full(l.shape, float(i)), l, mid, fl, fmid], axis=1)    # [l, mid]  (:192-194)
                kids[1::2] = np.stack([np.full(l.shape, float(i)), mid, r, fmid, fr], axis=1)    # [mid, r]  (:195-197)
                seeds.setdefault(int(dep) + 1, []).append(kids)
    seed_depths = sorted(seeds)
    level_records = {}
    front = np.empty((0, 5))
    depth = seed_depths[0] if seed_depths else 0
    while front.shape[0] or any(s >= depth for s in seed_depths):
        front = np.concatenate([front] + seeds.get(depth, []))
        if front.shape[0]:
            level_records[depth] = front.shape[0]
            rows = front[:, 0].astype(np.int64)
            l, r, fl, fr = (front[:, c] for c in range(1, 5))
            mid = (l + r) / 2                                # :187
            fmid = F(mid, rows)                              # :188
            lrarea = (fl + fr) * (r - l) / 2                 # :185
            larea = (fl + fmid) * (mid - l) / 2              # :189
            rarea = (fmid + fr) * (r - mid) / 2              # :190
            ref = np.abs((larea + rarea) - lrarea) > eps     # :191
            acc = np.stack([l, r, fl, fmid, fr, mid, np.full(l.shape, float(depth))], axis=1)[~ref]
            for i in np.unique(rows[~ref]):
                kept[i].append(acc[rows[~ref] == i])
            kids = np.empty((2 * int(ref.sum()), 5))
            kids[0::2] = np.stack([front[ref, 0], l[ref], mid[ref], fl[ref], fmid[ref]], axis=1)
            kids[1::2] = np.stack([front[ref, 0], mid[ref], r[ref], fmid[ref], fr[ref]], axis=1)
            front = kids
        depth += 1
        assert depth < 100, "the reference refinement is for trees that end"
    out = []
    for i in range(n):
        if not kept[i]:
            out.append(None)
        elif i not in changed:
            out.append(batch.rows[i])                        # every leaf kept: the input's row
        else:
            out.append(_row(np.concatenate(kept[i]), with_cum))
    return Refined(batch=mbr.Batch(out), reseeded=reseeded, seed_depths=seed_depths, level_records=level_records,
                   widest_level=max(level_records.values(), default=0), evaluated=sum(level_records.values()),
                   changed=changed)


# ---- the cases: mesh_batch_reference's, each from a coarser eps -------------------------------------------------
COARSE = {"edges": 1e-3, "param": 6.4e-5, "sin": 1e-3, "scale": 1e166}
EDGES_FIRST = 1e-1      # the two-hop test's first mesh


@functools.lru_cache(maxsize=None)
def built(name, eps):
    """The reference Batch of a case's rows built from the roots at `eps`."""
    integrand, a, b, theta, fine_eps, ref = mbr.case(name)
    if eps == fine_eps:
        return ref
    if integrand == PARAM:
        return mbr.Batch(mbr.param_rows(a, b, theta, eps))
    return mbr.fixed_batch(integrand, a, b, eps)


@functools.lru_cache(maxsize=None)
def case(name):
    """(integrand, a, b, theta, coarse eps, fine eps, the coarse Batch, the fine Batch, the Refined coarse -> fine)."""
    integrand, a, b, theta, fine_eps, fine = mbr.case(name)
    coarse = built(name, COARSE[name])
    return integrand, a, b, theta, COARSE[name], fine_eps, coarse, fine, refine(coarse, integrand, theta, fine_eps)


def same_mesh(u, v, cum=True):
    """Two Batches hold the same meshes bit for bit."""
    bits = lambda t: np.ascontiguousarray(t, np.float64).view(np.int64)   # noqa: E731
    ok = np.array_equal(u.offsets, v.offsets) and np.array_equal(bits(u.x), bits(v.x)) and np.array_equal(bits(u.f), bits(v.f))
    ok = ok and np.array_equal(u.level[u.level_known], v.level[v.level_known])
    ok = ok and np.array_equal(u.accepted, v.accepted) and np.array_equal(u.tasks, v.tasks) and np.array_equal(u.status, v.status)
    return ok and (not cum or np.array_equal(bits(u.cum), bits(v.cum)))


# ---- aq_mesh_err_batch --------------------------------------------------------------------------------------------
def err_exact(batch):
    """Per row the exact Σ|d| and Σd (Fractions; None for a row without nodes) and the leaf count."""
    out = []
    for i in range(len(batch.offsets) - 1):
        lv = leaves_of(batch, i)
        if lv.shape[0] == 0:
            out.append((None, None, 0))
            continue
        d, _, _ = leaf_d(lv)
        out.append((sum((Fraction(float(abs(v))) for v in d), Fraction(0)), sum((Fraction(float(v)) for v in d), Fraction(0)),
                    lv.shape[0]))
    return out


def err_sums(batch):
    """err_abs, err_signed as correctly rounded doubles (math.fsum; NaN for a row without nodes)."""
    n = len(batch.offsets) - 1
    ea, es = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        lv = leaves_of(batch, i)
        if lv.shape[0]:
            d, _, _ = leaf_d(lv)
            ea[i], es[i] = math.fsum(np.abs(d)), math.fsum(d)
    return ea, es


def area_sums(batch):
    """Per row the correctly rounded sum of the leaf areas (larea + rarea, :199); NaN without nodes."""
    n = len(batch.offsets) - 1
    out = np.full(n, np.nan)
    for i in range(n):
        lv = leaves_of(batch, i)
        if lv.shape[0]:
            _, larea, rarea = leaf_d(lv)
            out[i] = math.fsum(larea + rarea)
    return out


# ---- Context.integrate_mesh_batch_tol -----------------------------------------------------------------------------
def tol_loop(first, integrand, theta, epsabs, epsrel, eps0, shrink, max_rounds):
    """The loop restated: `first` is the reference Batch at eps0. Returns rounds, eps_used, the final Batch (cum not
    formed) and the task steps of all rounds together."""
    n = len(first.rows)
    batch, eps, r = first, float(eps0), 1
    evaluated = first.tasks_total
    rounds, eps_used = np.zeros(n, np.int32), np.zeros(n)
    invalid = first.status != 0
    live = np.ones(n, bool)
    while True:
        ea, _ = err_sums(batch)
        with np.errstate(invalid="ignore"):
            conv = (ea <= np.fmax(epsabs, epsrel * np.abs(area_sums(batch)))) & ~invalid
        retire = live & (conv | invalid | (r == max_rounds))
        rounds[retire] = np.where(conv[retire], r, -r)
        eps_used[retire] = eps
        live &= ~retire
        if not live.any():
            break
        eps, r = eps / float(shrink), r + 1
        step = refine(batch, integrand, theta, eps, active=live, with_cum=False)
        batch, evaluated = step.batch, evaluated + step.evaluated
    return rounds, eps_used, batch, evaluated
