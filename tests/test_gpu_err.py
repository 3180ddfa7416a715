"""The error estimate on the GPU (the _err calls): err_abs = Σ|d| and err_signed = Σd over the accepted
tasks, d = (larea + rarea) - lrarea (aquadPartA.c:191), from the same tree as the plain calls, against the
numpy / oracle walker of tests/err_reference.py.

Counts and levels are compared exactly; an area must lie within 1 ulp of the walker's math.fsum of the leaf
areas (the bound of test_gpu_params.py). Either error sum must lie within leaves * 2^-52 * err_abs of the
walker's math.fsum: the device adds the walker's own terms in another order, any order's error is at most
(leaves - 1) * 2^-53 * Σ|d| to first order, and twice that covers the second-order term and the staged
partials (err_reference.tol)."""
import math
import subprocess

import numpy as np
import pytest

import err_reference as er
import param_reference as pr

pytestmark = pytest.mark.gpu

COSH4, SIN_RECIP, USER, PARAM = 0, 1, 2, 3
EXACT = er.cosh4_exact(5.0)


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


def _check_sums(err_abs, err_signed, w, what):
    """One integral's two sums against its walk (a dict of plain numbers)."""
    t = er.tol(w)
    print(what, "err_abs", err_abs, w["err_abs"], "err_signed", err_signed, w["err_signed"], "tol", t)
    assert abs(err_abs - w["err_abs"]) <= t, (what, err_abs, w["err_abs"], t)
    assert abs(err_signed - w["err_signed"]) <= t, (what, err_signed, w["err_signed"], t)


def _check_lone(r, w, what):
    assert (r.tasks, r.accepted, r.levels) == (w["tasks"], w["leaves"], w["levels"]), what
    assert abs(r.area - w["area"]) <= math.ulp(w["area"]), (what, r.area.hex(), w["area"].hex())
    _check_sums(r.err_abs, r.err_signed, w, what)
    assert r.area_extrapolated == r.area + r.err_signed / 3.0, what


def _rows(ctx, n, first=0):
    """Rows {area, tasks, accepted, levels, err_abs, err_signed} of slots first..first+n-1, slot by slot."""
    ctx.synchronize()
    out = np.empty((n, 6))
    for i in range(n):
        r = ctx.fetch(first + i)
        out[i] = (r.area, r.tasks, r.accepted, r.levels) + ctx.fetch_err(first + i)
    return out


def _check_rows(area, tasks, acc, err_abs, err_signed, w, sel, what, levels=None):
    """Every integral of `sel` against the walk: counts exact, area within 1 ulp, both sums within tol."""
    bad = np.nonzero((np.asarray(tasks, np.int64) != w["tasks"][sel]) | (np.asarray(acc, np.int64) != w["leaves"][sel]))[0]
    assert bad.size == 0, (what, [(int(i), int(tasks[i]), int(w["tasks"][sel][i])) for i in bad[:8]], bad.size)
    if levels is not None:
        assert np.array_equal(np.asarray(levels, np.int64), w["levels"][sel]), what
    want = w["area"][sel]
    off = np.nonzero(np.abs(np.asarray(area) - want) > np.spacing(np.abs(want)))[0]
    assert off.size == 0, (what, [(int(i), float(area[i]).hex(), float(want[i]).hex()) for i in off[:8]], off.size)
    t = w["leaves"][sel] * 2.0 ** -52 * w["err_abs"][sel]
    for name, got in (("err_abs", err_abs), ("err_signed", err_signed)):
        dev = np.abs(np.asarray(got) - w[name][sel])
        print(what, name, "worst deviation / tol", float(np.max(dev / t)))
        off = np.nonzero(dev > t)[0]
        assert off.size == 0, (what, name, [(int(i), float(got[i]), float(w[name][sel][i]), float(t[i])) for i in off[:8]],
                               off.size)


@pytest.mark.parametrize("eps", [1e-3, 1e-10])
def test_lone_cosh4(ctx, eps):
    """cosh^4 on [0, 5]: the reference's tree and both sums; err_abs bounds the true error, which EPSILON does
    not, and the extrapolated area is closer to the integral than the area."""
    from ppls_amd import Problem
    w = er.lone(COSH4, 0.0, 5.0, eps)
    r = ctx.integrate_err(Problem(COSH4, 0.0, 5.0, eps))
    _check_lone(r, w, eps)
    assert abs(r.area - EXACT) <= r.err_abs
    assert abs(r.area_extrapolated - EXACT) < abs(r.area - EXACT)


def test_lone_sin_recip(ctx):
    """sin(1/x) on [1e-4, 1] at 1e-9: the signs are mixed, err_abs is about 50 x |err_signed| -- a swapped or
    un-abs'ed sum fails."""
    from ppls_amd import Problem
    w = er.lone(SIN_RECIP, 1e-4, 1.0, 1e-9)
    assert w["tasks"] == 56357 and w["err_abs"] > 30.0 * abs(w["err_signed"])
    _check_lone(ctx.integrate_err(Problem(SIN_RECIP, 1e-4, 1.0, 1e-9)), w, "sin_recip")


def test_lone_user_gaussian(ctx):
    """The AQ_F_USER plug-in (plain, not doubled, areas in the rounds) at 1e-10."""
    from ppls_amd import Problem
    w = er.lone(USER, 0.0, 5.0, 1e-10)
    assert w["tasks"] == 5359
    _check_lone(ctx.integrate_err(Problem(USER, 0.0, 5.0, 1e-10)), w, "user")


def test_lone_param(ctx):
    from ppls_amd import Problem
    t = pr.TREE_SHIFTED
    w = er.lone_tree(t)
    assert w["tasks"] == 42637
    _check_lone(ctx.integrate_err(Problem(PARAM, t[0], t[1], t[4]), [t[2], t[3]]), w, "param")


@pytest.mark.parametrize("which", ["param", "cosh4"])
def test_three_shards_add_up(ctx, which):
    """The same tree as 3 shards of the many-call: the shards' sums add to the walker's within the tolerance
    (of the whole tree), the counts add exactly."""
    if which == "param":
        t = pr.TREE_SHIFTED
        w = er.lone_tree(t)
        args = dict(integrand=PARAM, theta=[[t[2], t[3]]])
        a, b, eps = t[0], t[1], t[4]
    else:
        a, b, eps = 0.0, 5.0, 1e-8
        w = er.lone(COSH4, a, b, eps)
        assert w["tasks"] == 319295
        args = dict(integrand=COSH4)
    for s in range(3):
        ctx.integrate_many_err_async([a], [b], eps, first_slot=20 + s, shard=s, nshards=3, **args)
    rows = _rows(ctx, 3, first=20)
    assert np.all(rows[:, 1] > 0) and np.all(rows[:, 1] < w["tasks"])
    assert (int(rows[:, 1].sum()), int(rows[:, 2].sum()), int(rows[:, 3].max())) == (w["tasks"], w["leaves"], w["levels"])
    _check_sums(float(rows[:, 4].sum()), float(rows[:, 5].sum()), w, which)


@pytest.mark.parametrize("k", [2, 11, 13, 17, 300, 5000])
def test_many_integrals(ctx, k):
    """Launches of k integrals whose neighbours differ in theta and in size: the per-CU instance (below 12),
    the static stride, and jobs claimed from the counter. Every integral's sums are checked."""
    a, b, theta, w = er.draw_reference()
    ctx.integrate_many_err_async(a[:k], b[:k], pr.DRAW_EPS, integrand=PARAM, theta=theta[:k], first_slot=0)
    rows = _rows(ctx, k)
    _check_rows(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4], rows[:, 5], w, slice(0, k), k, levels=rows[:, 3])


def test_sums_follow_the_tag(ctx):
    """The 24-integral launch of test_sharing_between_waves_and_cus at eps = 1e-12 (every third the wide tree
    that starts in one wave): waves take other integrals' pairs from the pool and the HBM queue, and a partial
    carried across such a switch would land in the wrong integral's sums."""
    trees_ = [pr.TREE_WIDE if i % 3 == 0 else (pr.TREE_SHIFTED if i % 2 else pr.TREE_UNIT) for i in range(24)]
    a = [t[0] for t in trees_]
    b = [t[1] for t in trees_]
    theta = [[t[2], t[3]] for t in trees_]
    ctx.integrate_many_err_async(a, b, 1e-12, integrand=PARAM, theta=theta, first_slot=0)
    spilled = 0
    for i, t in enumerate(trees_):
        r = ctx.fetch(i)
        w = er.lone_tree(t)
        assert (r.tasks, r.accepted, r.levels) == (w["tasks"], w["leaves"], w["levels"]), i
        assert abs(r.area - w["area"]) <= math.ulp(w["area"]), i
        _check_sums(*ctx.fetch_err(i), w, i)
        spilled += r.spilled
    assert spilled > 0


def test_batch_params(ctx, monkeypatch):
    """3000 integrals of the draw through aq_integrate_batch_err in chunks of 1024 and 1976, size-ordered (the
    sums follow the scatter and the gather) and in input order."""
    n = 3000
    a, b, theta, w = er.draw_reference()
    monkeypatch.setenv("AQ_BATCH_FIRST", "1024")
    area, tasks, acc, ea, es = ctx.integrate_batch_err(a[:n], b[:n], pr.DRAW_EPS, integrand=PARAM, theta=theta[:n])
    _check_rows(area, tasks, acc, ea, es, w, slice(0, n), "sorted")
    monkeypatch.setenv("AQ_BATCH_SORT", "0")
    area, tasks, acc, ea, es = ctx.integrate_batch_err(a[:n], b[:n], pr.DRAW_EPS, integrand=PARAM, theta=theta[:n])
    _check_rows(area, tasks, acc, ea, es, w, slice(0, n), "input order")


def test_batch_every_ring_twice(ctx, monkeypatch):
    """468 integrals of the draw in chunks of 64, 128, 256 and 20: the smallest call in which every device ring
    is written again at both parities (chunks 2 and 3) with theta and error rows travelling, and an unsorted last
    chunk runs behind sorted ones. Twice on one context; then a bad bound in chunk 2 fails the call while chunk 1
    runs, and the context's next call gives the first 64 rows of the earlier result bit for bit, error sums
    included (the draw's trees have at most 945 tasks; 40 repetitions of this sequence gave the same bits every
    time, on this code and on the one before it)."""
    from ppls_amd import AquadError
    n = 468
    a, b, theta, w = er.draw_reference()
    a, b, theta = a[:n].copy(), b[:n], theta[:n]
    monkeypatch.setenv("AQ_BATCH_FIRST", "64")
    for again in range(2):
        area, tasks, acc, ea, es = ctx.integrate_batch_err(a, b, pr.DRAW_EPS, integrand=PARAM, theta=theta)
        _check_rows(area, tasks, acc, ea, es, w, slice(0, n), ("468 rows", again))
    a[64 + 128 + 5] = np.nan
    with pytest.raises(AquadError):
        ctx.integrate_batch_err(a, b, pr.DRAW_EPS, integrand=PARAM, theta=theta)
    area1, tasks1, acc1, ea1, es1 = ctx.integrate_batch_err(a[:64], b[:64], pr.DRAW_EPS, integrand=PARAM, theta=theta[:64])
    assert np.array_equal(tasks1, tasks[:64]) and np.array_equal(acc1, acc[:64])
    assert np.array_equal(area1, area[:64])
    assert np.array_equal(ea1, ea[:64]) and np.array_equal(es1, es[:64])
    _check_rows(area1, tasks1, acc1, ea1, es1, w, slice(0, 64), "64 rows after the failed call")


def test_batch_cosh4(ctx):
    a, b, w = er.batch_reference(2000, 1e-6)
    area, tasks, acc, ea, es = ctx.integrate_batch_err(a, b, 1e-6)
    _check_rows(area, tasks, acc, ea, es, w, slice(0, 2000), "cosh4 batch")


def test_slot_state(ctx, trees):
    """fetch_err wants a slot whose last launch was an _err launch; a slot's sums start from zero at every
    launch into it; a plain launch afterwards is what it always was."""
    from ppls_amd import AquadError
    a, b, theta, w = er.draw_reference()
    ctx.integrate_many_async(np.zeros(16), np.full(16, 5.0), 1e-3, first_slot=0)
    with pytest.raises(AquadError) as e:
        ctx.fetch_err(0)
    assert e.value.code == -1
    for again in range(2):   # the second launch finds the first one's sums in the slots
        ctx.integrate_many_err_async(a[:16], b[:16], pr.DRAW_EPS, integrand=PARAM, theta=theta[:16], first_slot=0)
        rows = _rows(ctx, 16)
        _check_rows(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4], rows[:, 5], w, slice(0, 16), ("launch", again))
    g = trees["cosh4_eps1e-8"]
    ctx.integrate_many_async(np.zeros(16), np.full(16, 5.0), 1e-8, first_slot=0)
    for i in range(16):
        r = ctx.fetch(i)
        assert (r.tasks, r.accepted) == (g["tasks"], g["leaves"]), i
    with pytest.raises(AquadError):
        ctx.fetch_err(3)


def test_cli_err(trees):
    """`aquad --err --eps 1e-10`: the reference's printout, then the two lines."""
    from ppls_amd import build
    g = trees["cosh4_eps1e-10"]
    w = er.lone(COSH4, 0.0, 5.0, 1e-10)
    out = subprocess.run([build.CLI, "--err", "--eps", "1e-10"], capture_output=True, text=True, timeout=120,
                         check=True).stdout
    lines = out.splitlines()
    assert lines[0] == "Area=" + g["reference"]["area_printed"]
    assert lines[2] == "Tasks Per Process" and lines[3] == "0\t1\t"
    assert [int(v) for v in lines[4].split()] == [0, g["tasks"]]
    assert len(lines) == 7 and lines[5].startswith("Error estimate=") and lines[6].startswith("Extrapolated area=")
    assert lines[5] == "Error estimate=%.6e" % w["err_abs"]
    ext = float(lines[6].split("=")[1])
    want = w["area"] + w["err_signed"] / 3.0
    # the device's area (within 1 ulp of the walker's) and its signed sum (within tol / 3 after the division)
    assert abs(ext - want) <= 2.0 * math.ulp(want) + er.tol(w) / 3.0
    # --err on more than one GPU, or with --levels, is refused before any device work
    p = subprocess.run([build.CLI, "--err", "--levels"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and p.stdout == ""


def test_untouched_paths(ctx, trees):
    """After every _err launch above, the plain synchronous call is what it was; and a context that never made
    an _err call holds what a fresh one holds (the error sums' array comes with the first _err call)."""
    from ppls_amd import Context, Problem
    r = ctx.integrate(Problem(eps=1e-10))
    g = trees["cosh4_eps1e-10"]
    assert r.tasks == 1464273 and r.accepted == g["leaves"]
    assert r.tasks_per_level == g["tasks_per_level"]
    assert (r.err_abs, r.err_signed, r.area_extrapolated) == (None, None, None)
    with Context(0) as c, Context(0) as d:
        fresh = c.device_bytes
        assert fresh == d.device_bytes
        c.integrate(Problem(eps=1e-3))
        c.integrate_many_async(np.zeros(4), np.full(4, 5.0), 1e-3, first_slot=0)
        c.synchronize()
        assert c.device_bytes == fresh
        c.integrate_err(Problem(eps=1e-3))
        assert c.device_bytes == fresh + 16 * (c.async_slots + 1)
