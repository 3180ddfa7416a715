"""GPU parity over the launch-shape matrix (tests/shape_matrix.py; tests/test_shape_matrix.py proves on the CPU
that its cases reach every instance of the persistent kernel) and over the trees at the edges of the documented
domain (tests/golden/edges.json).

Per integral: tasks, accepted and levels equal the oracle's; with histograms on, both per-level histograms are
equal. The area lies within 1 ulp of the oracle's rounded quad sum where include/aquad.h promises it (the
synchronous calls and per-CU launches: fewer than 12 integrals in slots below 16384), elsewhere within
max(1e-12 |want|, ulp(want)); an area of 0 must be exactly 0. ERR launches: both sums within err_reference.tol of
the walker's on the same rows, and exactly 0 for the empty interval. A context that collects diagnostics returns
one record per workgroup whose task fields sum to the launch's tasks.

Every case runs behind shape_matrix.BREAKER, a 12-task launch of another workload, so that its launches meet the
job-size hint the CPU test planned them with."""
import json
import os

import numpy as np
import pytest
from conftest import GOLDEN, device_seed_S

import shape_matrix as sm

pytestmark = pytest.mark.gpu

AREA_RTOL = 1e-12   # the suite's (tests/test_gpu.py, BASELINE.json north_star)
NPARTS = 16384      # slots whose per-CU launches keep per-workgroup words (aq_shape.h)
GSPLIT = 192        # waves per share and shard of a launch with a shard array (aq_shape.h AQ_GSPLIT_DEFAULT)


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dctx():
    """A context that collects diagnostics: its launches run the DIAG instances."""
    from ppls_amd import Context
    c = Context(0)
    c.set_diagnostics(True)
    yield c
    c.close()


def _area_tol(want, one_ulp):
    ulp = np.spacing(np.abs(want))
    return ulp if one_ulp else np.maximum(AREA_RTOL * np.abs(want), ulp)


def _check_area(got, want, one_ulp, what):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    zero = want == 0.0
    assert (got[zero] == 0.0).all(), (what, got[zero][:8])
    bad = np.nonzero(np.abs(got - want) > _area_tol(want, one_ulp))[0]
    assert bad.size == 0, (what, one_ulp, [(int(i), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:8]], bad.size)


def _check_counts(got, ref, idx, what):
    """got: rows of (tasks, accepted, levels) -- levels None where the entry point reports none."""
    for j, name in enumerate(("tasks", "leaves", "levels")):
        if got[j] is None:
            continue
        g, w = np.asarray(got[j], np.int64), np.asarray(ref[name])[idx]
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, name, [(int(i), int(idx[i]), int(g[i]), int(w[i])) for i in bad[:8]], bad.size)


def _breaker(c):
    b = sm.BREAKER
    c.integrate_many_async(np.ones(b["k"]), np.ones(b["k"]), b["eps"], first_slot=0, integrand=b["fid"])
    assert c.fetch(b["k"] - 1).tasks == 1


def _launch(c, case, j, a, b, theta):
    """Launch j of the case on the rows (a, b, theta): the batch entry points return their arrays, the synchronous
    ones their Result, the asynchronous ones None (their slots are fetched)."""
    from ppls_amd import Problem
    fid, eps, N, e = case.fid, sm.EPS[case.fid], case.nshards, case.entry
    if e == "integrate":
        return c.integrate(Problem(fid, float(a[0]), float(b[0]), eps))
    if e == "integrate_params":
        return c.integrate_params(Problem(fid, float(a[0]), float(b[0]), eps), theta[0])
    if e == "integrate_many_async":
        return c.integrate_many_async(a, b, eps, first_slot=case.first_slot, integrand=fid, shard=j if N > 1 else 0,
                                      nshards=N)
    if e == "integrate_many_params_async":
        return c.integrate_many_params_async(a, b, theta, eps, first_slot=case.first_slot, shard=j if N > 1 else 0,
                                             nshards=N)
    if e == "integrate_mixed_async":
        shards = (np.arange(a.size) + j) % N
        return c.integrate_mixed_async(a, b, shards, N, eps, first_slot=case.first_slot, integrand=fid)
    if e == "integrate_many_err_async":
        return c.integrate_many_err_async(a, b, eps, first_slot=case.first_slot, integrand=fid, theta=theta)
    if e == "integrate_batch":
        return c.integrate_batch(a, b, eps, integrand=fid)
    if e == "integrate_batch_params":
        return c.integrate_batch_params(a, b, theta, eps)
    if e == "integrate_batch_err":
        return c.integrate_batch_err(a, b, eps, integrand=fid, theta=theta)
    raise AssertionError(e)


def _fetch_all(c, case, k, hist):
    """The k slots of an asynchronous launch: area, tasks, accepted, levels, the two histograms (hist), the two
    error sums (ERR cases), spilled, n_cu."""
    out = {"area": np.empty(k), "tasks": np.empty(k, np.int64), "accepted": np.empty(k, np.int64),
           "levels": np.empty(k, np.int64), "n_cu": np.empty(k, np.int64), "tpl": [], "lpl": [], "err": np.zeros((k, 2))}
    for i in range(k):
        r = c.fetch(case.first_slot + i, detail=hist)
        out["area"][i], out["tasks"][i], out["accepted"][i], out["levels"][i], out["n_cu"][i] = \
            r.area, r.tasks, r.accepted, r.levels, r.n_cu
        if hist:
            out["tpl"].append(r.tasks_per_level)
            out["lpl"].append(r.leaves_per_level)
        if case.err:
            out["err"][i] = c.fetch_err(case.first_slot + i)
    return out


def _check_hist(tpl, lpl, ref, idx, what):
    for i, m in enumerate(idx):
        n = int(ref["levels"][m])
        assert tpl[i] == ref["tasks_per_level"][m, :n].tolist(), (what, i, int(m))
        assert lpl[i] == ref["leaves_per_level"][m, :n].tolist(), (what, i, int(m))


def _check_err(ea, es, w, idx, fid, what):
    t = (w["leaves"] * 2.0 ** -52 * w["err_abs"])[idx]   # err_reference.tol, row by row
    for name, got in (("err_abs", ea), ("err_signed", es)):
        dev = np.abs(np.asarray(got) - w[name][idx])
        bad = np.nonzero(dev > t)[0]
        assert bad.size == 0, (what, name, [(int(i), float(got[i]), float(w[name][idx][i]), float(t[i])) for i in bad[:8]])
    empty = np.nonzero(idx == sm.DEG_AT[0])[0]
    assert empty.size >= 1 and (np.asarray(ea)[empty] == 0.0).all() and (np.asarray(es)[empty] == 0.0).all(), what


def _run_unsharded(c, case, hist, oracle):
    W = c.num_workers
    n = W + 64
    a, b, theta = sm.master(case.fid, n)
    ref = sm.reference(case.fid, n)
    w = sm.err_walk(case.fid, n) if case.err else None
    for j, sym in enumerate(case.ks):
        k = sm.k_of(sym, W)
        idx = sm.case_rows(case, k)
        what = (case.id, hist, j)
        got = _launch(c, case, j, a[idx], b[idx], None if theta is None else theta[idx])
        one_ulp = case.entry in sm.SYNC_ENTRIES or (k < sm.PCU_MAXK and case.first_slot + k <= NPARTS)
        if case.entry in sm.SYNC_ENTRIES:
            _check_counts(([got.tasks], [got.accepted], [got.levels]), ref, idx, what)
            _check_area(got.area, ref["area"][idx], True, what)
            if hist:
                _check_hist([got.tasks_per_level], [got.leaves_per_level], ref, idx, what)
            assert sum(got.tasks_per_cu.values()) == got.tasks and got.n_cu == len(got.tasks_per_cu) >= 1
            total = got.tasks
        elif case.entry in sm.BATCH_ENTRIES:
            _check_counts((got[1], got[2], None), ref, idx, what)
            _check_area(got[0], (w if case.err else ref)["area"][idx], False, what)
            if case.err:
                _check_err(got[3], got[4], w, idx, case.fid, what)
            total = int(got[1].sum())
        else:
            r = _fetch_all(c, case, k, hist)
            _check_counts((r["tasks"], r["accepted"], r["levels"]), ref, idx, what)
            _check_area(r["area"], (w if case.err else ref)["area"][idx], one_ulp, what)
            if hist:
                _check_hist(r["tpl"], r["lpl"], ref, idx, what)
            if case.err:
                _check_err(r["err"][:, 0], r["err"][:, 1], w, idx, case.fid, what)
            # per-CU counts are kept exactly where the header says (n_cu = 0 elsewhere)
            assert ((r["n_cu"] >= 1) == one_ulp).all(), what
            total = int(r["tasks"].sum())
        print(case.id, "hist" if hist else "nohist", "launch", j, "W", W, "k", k, "tasks", total)
        assert total == int(ref["tasks"][idx].sum())
        if case.diag:
            d, names = c.diagnostics()
            assert d.shape == (c.num_cus, c.DIAG_WORDS), what
            assert int(d[:, list(names).index("tasks")].sum()) == total, what


def _run_sharded(c, case, hist, oracle):
    """The case's nshards launches hold every shard of every row: each entry equals the oracle's shard (the fixed
    integrands), the shards' counts add up to the tree's and their exact rows round to its area."""
    from ppls_amd import exact_round
    W, N = c.num_workers, case.nshards
    k = sm.k_of(case.ks[0], W)
    assert len(case.ks) == N and len(set(case.ks)) == 1
    a, b, theta = sm.master(case.fid, W + 64)
    ref = sm.reference(case.fid, W + 64)
    idx = sm.case_rows(case, k)
    mixed = case.entry == "integrate_mixed_async"
    G = W // (GSPLIT * N) if mixed else W
    tot = np.zeros((k, 72), np.int64)
    levels = np.zeros(k, np.int64)
    for j in range(N):
        _launch(c, case, j, a[idx], b[idx], None if theta is None else theta[idx])
        for i, m in enumerate(idx):
            s = (i + j) % N if mixed else j
            r = c.fetch(case.first_slot + i, detail=hist)
            if case.fid != sm.PARAM:
                o = oracle.integrate_shard(s, N, G=G, S=device_seed_S(G, N), integrand=case.fid, a=float(a[m]),
                                           b=float(b[m]), eps=sm.EPS[case.fid], maxlev=sm.MAXLEV)
                assert (r.tasks, r.accepted) == (o.tasks, o.leaves), (case.id, hist, j, i, int(m))
                if hist:
                    assert r.tasks_per_level == o.tasks_per_level[:len(r.tasks_per_level)], (case.id, j, i)
                    assert r.leaves_per_level == o.leaves_per_level[:len(r.leaves_per_level)], (case.id, j, i)
            row = c.fetch_exact(case.first_slot + i)
            assert row[71] >> 32 == 0 and (int(row[68]), int(row[69])) == (r.tasks, r.accepted)
            tot[i, :71] += row[:71]
            levels[i] = max(levels[i], r.levels)
    _check_counts((tot[:, 68], tot[:, 69], levels), ref, idx, (case.id, hist))
    _check_area([exact_round(t) for t in tot], ref["area"][idx], False, (case.id, hist))


def _run(c, case, hist, oracle):
    c.set_level_histograms(hist)
    try:
        _breaker(c)
        (_run_sharded if case.nshards > 1 else _run_unsharded)(c, case, hist, oracle)
    finally:
        c.set_level_histograms(True)


PLAIN_CASES = [c for c in sm.CASES if not (c.refused or c.diag or c.err)]


@pytest.mark.parametrize("hist", [True, False], ids=["hist", "nohist"])
@pytest.mark.parametrize("case", PLAIN_CASES, ids=[c.id for c in PLAIN_CASES])
def test_matrix(ctx, oracle, monkeypatch, case, hist):
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    _run(ctx, case, hist, oracle)


ERR_CASES = [c for c in sm.CASES if c.err]


@pytest.mark.parametrize("case", ERR_CASES, ids=[c.id for c in ERR_CASES])
def test_matrix_err(ctx, oracle, case):
    _run(ctx, case, False, oracle)


DIAG_CASES = [c for c in sm.CASES if c.diag]


@pytest.mark.parametrize("case", DIAG_CASES, ids=[c.id for c in DIAG_CASES])
def test_matrix_diag(dctx, oracle, case):
    _run(dctx, case, True, oracle)


REFUSED_CASES = [c for c in sm.CASES if c.refused]


@pytest.mark.parametrize("case", REFUSED_CASES, ids=[c.id for c in REFUSED_CASES])
def test_matrix_refused(ctx, case):
    """AQ_F_PARAM through an entry point that takes no theta: refused with the header's code, nothing enqueued,
    and the context goes on."""
    from ppls_amd import AquadError, Problem
    k = sm.k_of(case.ks[0], ctx.num_workers)
    a, b, theta = sm.master(case.fid, ctx.num_workers + 64)
    with pytest.raises(AquadError) as e:
        _launch(ctx, case, 0, a[:k], b[:k], theta[:k])
    assert e.value.code == case.refused
    assert ctx.integrate(Problem(eps=1e-3)).tasks == 6567


# ---- the edges of the documented domain ---------------------------------------------------------------------
with open(os.path.join(GOLDEN, "edges.json")) as _f:
    EDGES = json.load(_f)
EDGE_FID = {"cosh4": sm.COSH4, "sin_recip": sm.SIN_RECIP, "gauss": sm.USER}
# every leaf area of this tree is a multiple of 2^-1074 and the total is below 2^-1022: every partial sum, in any
# order, is exact in double, so every path must give the oracle's rounded sum bit for bit
EXACT_AREA = ("user_tail_eps0",)


def _edge_area(name, got, want, one_ulp, path):
    print(name, path, "area", float(got).hex(), "want", want.hex())
    if name in EXACT_AREA or want == 0.0:
        assert got == want, (name, path, float(got).hex(), want.hex())
    else:
        assert abs(got - want) <= float(_area_tol(want, one_ulp)), (name, path, float(got).hex(), want.hex())


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_tree(ctx, name):
    """One tree of tests/golden/edges.json through five paths: the synchronous call, the level path, three shards'
    exact rows (most of the 3 W virtual workers own nothing in a tree of a few hundred tasks), 16 copies in one
    launch of the heap instance without histograms, and -- the Gaussian's trees -- the same rows as theta = {0, 1}
    of the parametrised family."""
    from ppls_amd import Problem, exact_round
    g = EDGES[name]
    fid = EDGE_FID[g["integrand"]]
    a, b, eps = float.fromhex(g["a_hex"]), float.fromhex(g["b_hex"]), g["eps"]
    want = float.fromhex(g["area_hex"])
    counts = (g["tasks"], g["leaves"], g["levels"])
    p = Problem(fid, a, b, eps)
    ctx.set_level_histograms(True)
    r = ctx.integrate(p)
    assert (r.tasks, r.accepted, r.levels) == counts, (name, "sync")
    assert r.tasks_per_level == g["tasks_per_level"] and r.leaves_per_level == g["leaves_per_level"], (name, "sync")
    _edge_area(name, r.area, want, True, "sync")
    assert sum(r.tasks_per_cu.values()) == r.tasks
    r = ctx.integrate_levels(p)
    assert (r.tasks, r.accepted, r.levels) == counts, (name, "levels")
    assert r.tasks_per_level == g["tasks_per_level"] and r.leaves_per_level == g["leaves_per_level"], (name, "levels")
    _edge_area(name, r.area, want, False, "levels")
    tot = np.zeros(72, np.int64)
    levels = 0
    for s in range(3):
        row = ctx.integrate_shard_exact(p, s, 3)
        assert row[71] >> 32 == 0, (name, "shard", s)
        tot[:71] += row[:71]
        levels = max(levels, int(row[71] & 0xffffffff))
    assert (int(tot[68]), int(tot[69]), levels) == counts, (name, "shards")
    # the summed limbs hold the waves' partial sums exactly and are rounded once: held to the synchronous area's
    # target and bound (include/aquad.h: the lanes' own double sums leave the last bit schedule-dependent)
    _edge_area(name, exact_round(tot), want, True, "shards")
    ctx.set_level_histograms(False)
    try:
        _breaker(ctx)
        ctx.integrate_many_async(np.full(16, a), np.full(16, b), eps, first_slot=0, integrand=fid)
        for i in range(16):
            r = ctx.fetch(i)
            assert (r.tasks, r.accepted, r.levels) == counts, (name, "heap", i)
            _edge_area(name, r.area, want, False, "heap %d" % i)
        if fid == sm.USER:
            theta = np.tile([0.0, 1.0], (16, 1))
            r = ctx.integrate_params(Problem(sm.PARAM, a, b, eps), theta[0])
            assert (r.tasks, r.accepted, r.levels) == counts, (name, "param sync")
            _edge_area(name, r.area, want, True, "param sync")
            ctx.integrate_many_params_async(np.full(16, a), np.full(16, b), theta, eps, first_slot=0)
            for i in range(16):
                r = ctx.fetch(i)
                assert (r.tasks, r.accepted, r.levels) == counts, (name, "param heap", i)
                _edge_area(name, r.area, want, False, "param heap %d" % i)
    finally:
        ctx.set_level_histograms(True)
