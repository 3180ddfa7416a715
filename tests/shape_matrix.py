"""The launch-shape matrix: every integrand through every instance of the persistent kernel that plan_launch
(ppls_amd/csrc/aq_launch_plan.h) can choose for it, as data. One list of cases for the CPU test that proves the
matrix reaches every instance (tests/test_shape_matrix.py, through the planner itself) and for the GPU test that
runs every case against the oracle (tests/test_gpu_matrix.py).

A case names an entry point of ppls_amd.Context, an integrand, the launches' sizes as functions of W (the
context's worker count: "1" .. "16", "W-1", "W+64"), the shard arguments, the first slot, and whether the
context collects diagnostics or the launch is an error-estimate (ERR) launch. Its launches run in order on one
context, behind a launch of another workload (BREAKER) that leaves the job-size hint stale: a case therefore
meets the plans a fresh context would give it, whatever ran before.

Bounds are deterministic: the oracle's batch_bounds mapped affinely into DOMAIN (param_reference.draw for the
parametrised family), with the degenerate rows of DEGENERATE written over the rows DEG_AT. One oracle run per
integrand covers the W + 64 rows; a launch of k rows takes rows(fid, k) of it.

A helper module, not a conftest: no GPU import, the CPU and GPU tests share its cached results.
"""
import functools
import time
from collections import namedtuple

import numpy as np

import err_reference as er
import param_reference as pr

COSH4, SIN_RECIP, USER, PARAM = 0, 1, 2, 3
FIDS = (COSH4, SIN_RECIP, USER, PARAM)
FID_NAME = {COSH4: "cosh4", SIN_RECIP: "sin_recip", USER: "user", PARAM: "param"}
AQ_EINVAL = -1
GRID, NW, ERR_NW = 256, 12, 8          # the planner's grid of the CPU test; waves per workgroup (aq_shape.h, aq_launch_plan.h)
SYNC_SLOT = 1 << 18                    # aq_shape.h: the synchronous calls' internal slot
BATCH_FIRST, BATCH_SORT_MIN, PCU_MAXK = 131072, 64, 12   # aq_abi.inc AQ_BATCH_FIRST, aq_batch_plan.h, aq_shape.h
MAXLEV = 128
VARIANTS = ("PLAIN", "PCU", "DIAG", "DIAG_PCU", "LONE", "HEAP")   # aq_launch_plan.h Variant

KSYMS = ("1", "2", "4", "5", "11", "12", "16", "W-1", "W+64")
# one eps per integrand: the oracle's W + 64 rows take well under a second (at W = 3072: cosh4 5.4e6 tasks in 0.38 s,
# sin(1/x) 1.2e6 in 0.07 s, Gaussian 3.5e6 in 0.16 s; cosh4 at 1e-4, 1.2e7 tasks, took 0.87 s of the budget)
EPS = {COSH4: 1e-3, SIN_RECIP: 1e-7, USER: 1e-8, PARAM: pr.DRAW_EPS}
DOMAIN = {COSH4: (-5.0, 5.0), SIN_RECIP: (1e-3, 1.0), USER: (-6.0, 6.0)}
# the degenerate rows, in the order of DEG_AT: b = a | b = nextafter(a) | the width scaled by 2^-30 | [0, 2^-900] | an
# interval straddling 0. sin(1/x) has the first three (its rows stay at x >= 1e-8, the header's bit-exact range).
DEGENERATE = ("empty", "ulp", "narrow", "zero_tiny", "straddle")
DEG_AT = (1, 3, 5, 7, 9)               # below 11: every launch of k >= 11 rows holds them all
ORACLE_BUDGET_S = 1.0


def degenerate_kinds(fid):
    return DEGENERATE[:3] if fid == SIN_RECIP else DEGENERATE


def k_of(sym, W):
    return {"W-1": W - 1, "W+64": W + 64}.get(sym) or int(sym)


def _degenerate(kind, a, b, h):
    """The degenerate row written over the row [a, b]; h: the scale of the straddling interval."""
    w = b - a
    return {"empty": (a, a), "ulp": (a, np.nextafter(a, np.inf)), "narrow": (a, a + w * 2.0 ** -30),
            "zero_tiny": (0.0, 2.0 ** -900), "straddle": (-0.25 * h, 0.35 * h)}[kind]


@functools.lru_cache(maxsize=None)
def master(fid, n):
    """The integrand's n rows (a, b, theta or None), degenerate rows included; read-only arrays."""
    if fid == PARAM:
        a, b, theta = pr.draw(n)
        a, b = a.copy(), b.copy()
    else:
        from oracle import pyoracle
        u, v = pyoracle.batch_bounds(n)
        lo, hi = DOMAIN[fid]
        a, b, theta = lo + (hi - lo) * (u / 5.0), lo + (hi - lo) * (v / 5.0), None
    for kind, i in zip(degenerate_kinds(fid), DEG_AT):
        # (the straddling interval: a quarter of the domain's upper bound to the left of 0 and 0.35 of it to the
        # right -- a tree of many tasks at EPS; the parametrised rows scale their own width)
        a[i], b[i] = _degenerate(kind, a[i], b[i], DOMAIN[fid][1] if fid in DOMAIN else b[i] - a[i])
    assert (b >= a).all()
    for x in (a, b) + (() if theta is None else (theta,)):
        x.flags.writeable = False
    return a, b, theta


def rows(fid, k):
    """The master rows of a launch of k integrals: the first k, and for k = 2, 4, 5 the degenerate rows first."""
    if k in (2, 4, 5):
        deg = list(DEG_AT[:len(degenerate_kinds(fid))])
        return np.array((deg + [i for i in range(k) if i not in deg])[:k])
    return np.arange(k)


@functools.lru_cache(maxsize=None)
def reference(fid, n):
    """The oracle on master(fid, n), once per process: tasks, leaves, levels, area (the rounded quad sum) per row,
    the two per-level histograms [n, MAXLEV], and "seconds", the run's wall time."""
    from oracle import pyoracle
    a, b, theta = master(fid, n)
    t0 = time.perf_counter()
    if fid == PARAM:
        w = pr.walk(a, b, theta, EPS[fid], pyoracle, maxlev=MAXLEV)
        out = {"tasks": w["tasks"], "leaves": w["leaves"], "levels": w["levels"], "area": w["area"],
               "tasks_per_level": w["tasks_per_level"], "leaves_per_level": w["leaves_per_level"]}
    else:
        out = {"tasks": np.zeros(n, np.int64), "leaves": np.zeros(n, np.int64), "levels": np.zeros(n, np.int64),
               "area": np.zeros(n), "tasks_per_level": np.zeros((n, MAXLEV), np.int64),
               "leaves_per_level": np.zeros((n, MAXLEV), np.int64)}
        for i in range(n):
            r = pyoracle.integrate(fid, float(a[i]), float(b[i]), EPS[fid], maxlev=MAXLEV)
            out["tasks"][i], out["leaves"][i], out["levels"][i], out["area"][i] = r.tasks, r.leaves, r.levels, r.area
            out["tasks_per_level"][i, :r.levels] = r.tasks_per_level
            out["leaves_per_level"][i, :r.levels] = r.leaves_per_level
    seconds = time.perf_counter() - t0
    for v in out.values():
        v.flags.writeable = False
    out["seconds"] = seconds
    return out


@functools.lru_cache(maxsize=None)
def err_walk(fid, n):
    """err_reference.walk on master(fid, n): the ERR cases' sums (and its own counts and math.fsum areas)."""
    from oracle import pyoracle
    a, b, theta = master(fid, n)
    return er.walk(a, b, EPS[fid], fid, pyoracle, theta, maxlev=MAXLEV)


# ---- the cases --------------------------------------------------------------------------------------------
# entry: a method of ppls_amd.Context. ks: the sizes of the case's launches, in order (an adaptive launch --
# unsharded, 12 integrals or more -- runs twice: first, then hinted). nshards > 1: launch j gives row i shard
# (i + j) % nshards, so the case's nshards launches hold every shard of every row. env: the batch front end's
# environment. refused: the code the entry point returns by design (include/aquad.h: AQ_F_PARAM goes through the
# _params and _err entry points only), else None.
Case = namedtuple("Case", "id entry fid ks nshards first_slot diag err env refused")

PLAIN_ENTRY = {"sync": "integrate", "many": "integrate_many_async", "batch": "integrate_batch"}
PARAM_ENTRY = {"sync": "integrate_params", "many": "integrate_many_params_async", "batch": "integrate_batch_params"}
ERR_ENTRY = {"sync": "integrate_err", "many": "integrate_many_err_async", "batch": "integrate_batch_err"}
SYNC_ENTRIES = ("integrate", "integrate_params", "integrate_err")
BATCH_ENTRIES = ("integrate_batch", "integrate_batch_params", "integrate_batch_err")


def _adaptive(k, nshards):
    return nshards == 1 and k not in ("1", "2", "4", "5", "11")


def _case(kind, fid, ks, nshards=1, first_slot=0, diag=False, err=False, env=(), refused=None, entry=None, tag=""):
    if isinstance(ks, str):
        ks = (ks, ks) if _adaptive(ks, nshards) else (ks,) * nshards
    entry = entry or (ERR_ENTRY if err else PARAM_ENTRY if fid == PARAM else PLAIN_ENTRY)[kind]
    name = "-".join([entry, FID_NAME[fid], "_".join(ks)] + (["N%d" % nshards] if nshards > 1 else []) +
                    (["slot%d" % first_slot] if first_slot else []) + (["diag"] if diag else []) +
                    ["%s=%s" % kv for kv in env] + ([tag] if tag else []) + (["refused"] if refused else []))
    return Case(name, entry, fid, tuple(ks), nshards, first_slot, diag, err, tuple(env), refused)


def _build():
    c = []
    for fid in FIDS:
        c.append(_case("sync", fid, "1"))
        c += [_case("many", fid, k) for k in KSYMS]
        # the bulk instance, the few-integral instance, the bulk instance again: HEAP behind a hint that holds no
        # per-integral count (adaptive 3) and PLAIN behind one that does (7)
        c.append(_case("many", fid, ("W+64", "16", "W+64"), tag="switch"))
        # few integrals whose slots lie past the per-workgroup words: the heap instance with the static deal
        c.append(_case("many", fid, "5", first_slot=20000))
        c.append(_case("many", fid, "5", nshards=3))          # sharded per-CU launches: the oracle's partition
        c.append(_case("batch", fid, "W+64"))
        c.append(_case("batch", fid, "W+64", env=(("AQ_BATCH_SORT", "0"),)))
        # chunks of 64, 128 .. 1024 and the rest, all sorted; then an unsorted first chunk of 32, sorted ones, and
        # a short unsorted last chunk of 40 -- every chunk holds the degenerate rows (case_rows)
        c.append(_case("batch", fid, "W+64", env=(("AQ_BATCH_FIRST", "64"),)))
        c.append(_case("batch", fid, "W+64", env=(("AQ_BATCH_FIRST", "32"), ("AQ_BATCH_LAST", "40"))))
        for k in ("1", "5", "16", "W+64"):
            c.append(_case("sync" if k == "1" else "many", fid, k, diag=True))
        c += [_case("many", fid, k, err=True) for k in ("5", "16", "W+64")]
        c.append(_case("batch", fid, "W+64", err=True))
    for fid in (COSH4, SIN_RECIP, USER):
        for k in ("5", "12", "16"):
            c.append(_case("many", fid, k, nshards=2, entry="integrate_mixed_async"))
        c.append(_case("many", fid, "16", entry="integrate_mixed_async"))   # nshards == 1: an unsharded launch
    for kind in ("sync", "many", "batch"):
        c.append(_case(kind, PARAM, "W+64" if kind == "batch" else "1" if kind == "sync" else "5",
                       entry=PLAIN_ENTRY[kind], refused=AQ_EINVAL))
    c.append(_case("many", PARAM, "5", nshards=2, entry="integrate_mixed_async", refused=AQ_EINVAL))
    assert len({x.id for x in c}) == len(c)
    return tuple(c)


CASES = _build()

# what the matrix must reach: (integrand, variant, err)
REQUIRED = (
    {(f, v, False) for f in FIDS for v in ("PCU", "HEAP", "PLAIN", "DIAG", "DIAG_PCU")} |
    {(f, "LONE", False) for f in (COSH4, USER, PARAM)} |
    {(f, v, True) for f in FIDS for v in ("PCU", "HEAP", "PLAIN")})


# ---- a case's launches as the planner sees them (aq_abi.inc: many_args, sync_args, batch_run's launch_chunk) -----
def batch_chunks(n, first, last=0):
    """aq_host_args.h batch_chunks: `first`, then doubling up to MAXK, the remainder last -- split so that the last
    chunk is `last` when the remainder is more than twice that."""
    c, done, nxt = [], 0, min(first, 1 << 18)
    while n - done > nxt:
        c.append(nxt)
        done += nxt
        nxt = min(2 * nxt, 1 << 18)
    rem = n - done
    return c + ([rem - last, last] if last and rem > 2 * last else [rem])


def case_chunks(case, k):
    """The launches of one call of the case's entry point on k rows: (k, sorted, first row) per launch."""
    if case.entry not in BATCH_ENTRIES:
        return [(k, False, 0)]
    env = dict(case.env)
    sort = env.get("AQ_BATCH_SORT", "1") != "0"
    out, off = [], 0
    for m in batch_chunks(k, int(env.get("AQ_BATCH_FIRST", BATCH_FIRST)), int(env.get("AQ_BATCH_LAST", 0))):
        out.append((m, sort and m >= BATCH_SORT_MIN, off))
        off += m
    return out


def case_rows(case, k):
    """The master rows of one call of the case on k rows: rows(fid, k), and for a batch call of several chunks the
    degenerate rows again at DEG_AT of every chunk, so that each chunk's launch holds them."""
    idx = rows(case.fid, k).copy()
    for m, _, off in case_chunks(case, k)[1:]:
        for d in DEG_AT[:len(degenerate_kinds(case.fid))]:
            if d < m:
                idx[off + d] = d
    return idx


# the launch before every case: 12 empty cosh^4 intervals at eps = 1 (12 tasks), an unsharded launch that leaves
# the hint valid for a workload no case has -- the next launch plans as on a fresh context
BREAKER = {"fid": COSH4, "k": 12, "eps": 1.0}


def requests(case, W=GRID * NW, grid=GRID):
    """The case's plan_launch requests in order, the breaker first: dicts of the `--plan` row's fields. hint_valid
    0: a fresh hint; -1: the hint the previous row left."""
    def row(fid, k, eps, **kw):
        r = dict(fid=fid, grid=grid, k=k, shard_array=0, nshards=1, first_slot=0, diag=int(case.diag), batch_heap=0,
                 gsplit_env=0, eps=eps, err=0, hint_valid=-1, preset=0)
        r.update(kw)
        return r
    out = [row(BREAKER["fid"], BREAKER["k"], BREAKER["eps"], hint_valid=0)]
    batch = case.entry in BATCH_ENTRIES
    for j, sym in enumerate(case.ks):
        fresh = batch and j == 0   # (batch_run: no measured hint for this workload yet; the second call has one)
        for m, srt, _ in case_chunks(case, k_of(sym, W)):
            out.append(row(case.fid, m, EPS[case.fid], err=int(case.err), batch_heap=int(batch),
                           shard_array=int(case.entry == "integrate_mixed_async" and case.nshards > 1),
                           nshards=case.nshards, preset=int(srt and fresh),
                           first_slot=SYNC_SLOT if case.entry in SYNC_ENTRIES else case.first_slot))
            fresh = fresh and m < PCU_MAXK
    return out


def plan_rows(reqs):
    """The requests as the text `launch_plan_check --plan` reads."""
    def line(r):
        return "%d %d %d %d %d %d %d %d %d %s %d %d %d 0 -1 0 0x0p+0" % (
            r["fid"], r["grid"], r["k"], r["shard_array"], r["nshards"], r["first_slot"], r["diag"], r["batch_heap"],
            r["gsplit_env"], float(r["eps"]).hex(), r["err"], r["hint_valid"], r["preset"])
    return "".join(line(r) + "\n" for r in reqs)


PLAN_FIELDS = ("rc", "variant", "nwt", "shares", "D", "tail_from", "tail_mult", "per_cu", "static_jobs", "adaptive",
               "err", "deeper")


def parse_plans(text):
    out = []
    for ln in text.splitlines():
        f = ln.split()
        d = dict(zip(PLAN_FIELDS, (int(x) for x in f[:len(PLAN_FIELDS)])))
        d["variant"] = VARIANTS[d["variant"]]
        out.append(d)
    return out
