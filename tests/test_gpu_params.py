"""Per-integral parameters on the GPU (AQ_F_PARAM): F(x; theta_i) through the persistent kernel and the
batch front end, against the numpy / oracle walker of tests/param_reference.py. Counts are compared
exactly; an area must lie within 1 ulp of the walker's math.fsum of the leaf areas (the bound of the
per-CU tests in test_gpu.py)."""
import math
import subprocess

import numpy as np
import pytest

import param_reference as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


def _problem(tree):
    from ppls_amd import PARAM, Problem
    return Problem(PARAM, tree[0], tree[1], tree[4])


def _gather(ctx, n):
    """Rows {area, tasks, accepted} of slots 0..n-1, fetched slot by slot (aq_fetch reports a slot's error
    bits as a failure)."""
    ctx.synchronize()
    out = np.empty((n, 3))
    for i in range(n):
        r = ctx.fetch(i)
        out[i] = (r.area, r.tasks, r.accepted)
    return out


def _check_rows(area, tasks, acc, w, sel, what):
    """Every integral of `sel` against the walker: counts exact, area within 1 ulp."""
    bad = np.nonzero((np.asarray(tasks, np.int64) != w["tasks"][sel]) | (np.asarray(acc, np.int64) != w["leaves"][sel]))[0]
    assert bad.size == 0, (what, [(int(i), int(tasks[i]), int(w["tasks"][sel][i])) for i in bad[:8]], bad.size)
    want = w["area"][sel]
    off = np.nonzero(np.abs(np.asarray(area) - want) > np.spacing(np.abs(want)))[0]
    assert off.size == 0, (what, [(int(i), float(area[i]).hex(), float(want[i]).hex()) for i in off[:8]], off.size)


def _check_lone(r, w, what):
    assert (r.tasks, r.accepted, r.levels) == (w["tasks"], w["leaves"], w["levels"]), what
    assert abs(r.area - w["area"]) <= math.ulp(w["area"]), (what, r.area.hex(), w["area"].hex())


def test_param_integrand_bit_exact(ctx, oracle, plugin_bits):
    """F(x; mu, s) on the device equals the numpy / oracle expression bit for bit over 200 000 random
    points with (x - mu) * s across +-40 (exp's underflow and subnormal-result paths) and a band of tiny
    arguments (its 1 + x path); at theta = {0, 1} it equals the AQ_F_USER fixture."""
    rng = np.random.default_rng(7)
    n = 200000
    mu = rng.uniform(-2.0, 2.0, n)
    s = np.exp(rng.uniform(-2.0, 2.0, n))
    x = mu + rng.uniform(-40.0, 40.0, n) / s
    x[:2000] = mu[:2000] + rng.uniform(-1.0, 1.0, 2000) * 10.0 ** rng.uniform(-12.0, -7.0, 2000)
    x[2000:2010] = mu[2000:2010]
    theta = np.stack([mu, s], axis=1)
    want = pr.F(x, mu, s, oracle)
    assert (want == 0.0).sum() > 1000 and ((want > 0.0) & (want < 2.2250738585072014e-308)).sum() > 100
    got = ctx.eval_integrand_params(x, theta)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, [(float(x[i]), theta[i].tolist(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:8]]
    xf = plugin_bits["x"].view(np.float64)
    got = ctx.eval_integrand_params(xf, np.tile([0.0, 1.0], (xf.size, 1))).view(np.uint64)
    bad = np.nonzero(got != plugin_bits["F"])[0]
    assert bad.size == 0, [(float(xf[i]), hex(int(got[i])), hex(int(plugin_bits["F"][i]))) for i in bad[:8]]


@pytest.mark.parametrize("name", ["gauss_eps1e-10", "gauss_eps1e-13"])
def test_unit_theta_is_the_reference_pinned_tree(ctx, trees, name):
    """theta = {0, 1} is the AQ_F_USER Gaussian: the reference binary's task total and printed area."""
    from ppls_amd import PARAM, Problem
    g = trees[name]
    r = ctx.integrate_params(Problem(PARAM, g["a"], g["b"], g["eps"]), [0.0, 1.0])
    assert r.tasks == g["reference"]["tasks_total"]
    assert "%f" % r.area == g["reference"]["area_printed"]
    assert (r.accepted, r.levels) == (g["leaves"], g["levels"])
    assert r.tasks_per_level == g["tasks_per_level"] and r.leaves_per_level == g["leaves_per_level"]


def test_lone_integral_and_its_shards(ctx):
    """mu = 0.3, s = 1.7 on [-2, 3] at eps = 1e-12 (42 637 tasks, 17 levels): counts, levels, both
    histograms and the area of the synchronous call; then the same tree as 3 shards of the many-call --
    their exact rows summed limb-wise give the same counts and, rounded once, the same area."""
    from ppls_amd import exact_round
    t = pr.TREE_SHIFTED
    w = pr.tree_reference(t)
    assert (w["tasks"], w["levels"]) == (42637, 17)
    r = ctx.integrate_params(_problem(t), [t[2], t[3]])
    _check_lone(r, w, "lone")
    assert r.tasks_per_level == w["tasks_per_level"] and r.leaves_per_level == w["leaves_per_level"]
    for s in range(3):
        ctx.integrate_many_params_async([t[0]], [t[1]], [[t[2], t[3]]], t[4], first_slot=20 + s, shard=s, nshards=3)
    ctx.synchronize()
    tot = np.zeros(72, np.int64)
    levels = 0
    for s in range(3):
        row = ctx.fetch_exact(20 + s)
        assert row[71] >> 32 == 0   # no error bits
        assert 0 < row[68] < w["tasks"]
        tot[:71] += row[:71]
        levels = max(levels, int(row[71] & 0xffffffff))
    assert (int(tot[68]), int(tot[69]), levels) == (w["tasks"], w["leaves"], w["levels"])
    assert abs(exact_round(tot) - w["area"]) <= math.ulp(w["area"])


@pytest.mark.parametrize("k", [2, 11, 13, 17, 300, 5000])
def test_theta_follows_the_tag(ctx, k):
    """Launches of k integrals whose neighbours differ in theta AND in tree size (a stale theta moves the
    counts): below and above the per-CU instance's 12 and the static-stride 16, and past the 3072 waves
    (jobs claimed from the counter). Every integral is checked."""
    a, b, theta, w = pr.draw_reference()
    ctx.integrate_many_params_async(a[:k], b[:k], theta[:k], pr.DRAW_EPS, first_slot=0)
    rows = _gather(ctx, k)
    _check_rows(rows[:, 0], rows[:, 1], rows[:, 2], w, slice(0, k), k)
    if k <= 17:   # levels and histograms too, slot by slot
        for i in range(k):
            r = ctx.fetch(i, detail=True)
            assert r.levels == w["levels"][i], (k, i)
            assert r.tasks_per_level == [int(v) for v in w["tasks_per_level"][i, :r.levels]], (k, i)
            assert r.leaves_per_level == [int(v) for v in w["leaves_per_level"][i, :r.levels]], (k, i)


def test_sharing_between_waves_and_cus(ctx):
    """One launch of 24 integrals at eps = 1e-12: every third the big tree mu = 0, s = 2^-6 on [-2^20, 2^20]
    (197 487 tasks, 31 levels), the others the tree of test_lone_integral and the theta = {0, 1} tree in
    turn. Each big tree starts in ONE wave (its work lies below two adjacent seed positions of one share),
    whose ring passes the give threshold while the other waves run dry: pool takes and HBM queue chunks
    then carry pairs of another integral than the taker's last. All 24 exact, and the launch moved pairs
    through the HBM queue. (Shape: on [-256, 256], 196 795 tasks, every wave of this launch got an even
    ~1 500-task share and spilled was 0 on the MI355X; the interval was widened until it was not.)"""
    trees_ = [pr.TREE_WIDE if i % 3 == 0 else (pr.TREE_SHIFTED if i % 2 else pr.TREE_UNIT) for i in range(24)]
    assert set(trees_) == {pr.TREE_WIDE, pr.TREE_SHIFTED, pr.TREE_UNIT}
    a = [t[0] for t in trees_]
    b = [t[1] for t in trees_]
    theta = [[t[2], t[3]] for t in trees_]
    assert pr.tree_reference(pr.TREE_WIDE)["tasks"] == 197487
    ctx.integrate_many_params_async(a, b, theta, 1e-12, first_slot=0)
    spilled = 0
    for i, t in enumerate(trees_):
        r = ctx.fetch(i, detail=True)
        w = pr.tree_reference(t)
        _check_lone(r, w, i)
        assert r.tasks_per_level == w["tasks_per_level"] and r.leaves_per_level == w["leaves_per_level"], i
        spilled += r.spilled
    assert spilled > 0


def test_batch_front_end_params(ctx, monkeypatch):
    """3000 integrals of the draw through aq_integrate_batch_params in chunks of 1024 and 1976, both size-
    ordered (theta follows the bounds through the scatter), then in input order (AQ_BATCH_SORT=0): every
    integral equals the walker, in input order."""
    n = 3000
    a, b, theta, w = pr.draw_reference()
    monkeypatch.setenv("AQ_BATCH_FIRST", "1024")
    area, tasks, acc = ctx.integrate_batch_params(a[:n], b[:n], theta[:n], pr.DRAW_EPS)
    _check_rows(area, tasks, acc, w, slice(0, n), "sorted")
    monkeypatch.setenv("AQ_BATCH_SORT", "0")
    area, tasks, acc = ctx.integrate_batch_params(a[:n], b[:n], theta[:n], pr.DRAW_EPS)
    _check_rows(area, tasks, acc, w, slice(0, n), "input order")


def test_interleaved_with_the_fixed_integrands(ctx, trees):
    """A parametrised launch into slots 0-15, then the golden cosh^4 launch into the same slots: the slots
    are reset in between and the second launch gives its golden counts."""
    g = trees["cosh4_eps1e-8"]
    a, b, theta, w = pr.draw_reference()
    ctx.integrate_many_params_async(a[:16], b[:16], theta[:16], pr.DRAW_EPS, first_slot=0)
    ctx.integrate_many_async(np.zeros(16), np.full(16, 5.0), 1e-8, first_slot=0)
    for i in range(16):
        r = ctx.fetch(i)
        assert (r.tasks, r.accepted) == (g["tasks"], g["leaves"]), i
    ctx.integrate_many_params_async(a[:16], b[:16], theta[:16], pr.DRAW_EPS, first_slot=0)
    rows = _gather(ctx, 16)
    _check_rows(rows[:, 0], rows[:, 1], rows[:, 2], w, slice(0, 16), "after cosh4")


def test_param_errors(ctx):
    """AQ_F_PARAM through an entry point that takes no theta is AQ_EINVAL; so are a NaN in theta, s = 0,
    and bounds outside the engine's domain. A theta of the wrong width never reaches the library. The
    context stays usable."""
    from ppls_amd import PARAM, AquadError, Problem
    t = pr.TREE_UNIT
    one = np.array([0.0]), np.array([1.0])
    for call in (lambda: ctx.integrate(Problem(PARAM, 0.0, 1.0, 1e-3)),
                 lambda: ctx.integrate_many_async(*one, 1e-3, integrand=PARAM),
                 lambda: ctx.integrate_batch(*one, 1e-3, integrand=PARAM),
                 lambda: ctx.eval_integrand(one[0], integrand=PARAM),
                 lambda: ctx.integrate_levels(Problem(PARAM, 0.0, 1.0, 1e-3)),
                 lambda: ctx.integrate_params(Problem(2, 0.0, 1.0, 1e-3), [0.0, 1.0]),
                 lambda: ctx.integrate_params(_problem(t), [float("nan"), 1.0]),
                 lambda: ctx.integrate_params(_problem(t), [0.0, 0.0]),
                 lambda: ctx.integrate_params(_problem(t), [0.0, float("inf")]),
                 lambda: ctx.integrate_params(Problem(PARAM, 1.0, 0.0, 1e-3), [0.0, 1.0]),
                 lambda: ctx.integrate_many_params_async(*one, [[0.0, float("nan")]], 1e-3),
                 lambda: ctx.integrate_many_params_async(*one, [[0.0, 1.0]], 1e-3, shard=2, nshards=2),
                 lambda: ctx.integrate_batch_params([0.0, 0.0], [1.0, 1.0], [[0.0, 1.0], [0.0, 0.0]], 1e-3)):
        with pytest.raises(AquadError) as e:
            call()
        assert e.value.code == -1
    for call in (lambda: ctx.integrate_params(_problem(t), [0.0, 1.0, 2.0]),
                 lambda: ctx.integrate_many_params_async(*one, [[0.0]], 1e-3),
                 lambda: ctx.integrate_batch_params(*one, [[0.0, 1.0], [0.0, 1.0]], 1e-3),
                 lambda: ctx.eval_integrand_params(one[0], [[0.0, 1.0, 2.0]])):
        with pytest.raises(ValueError):
            call()
    r = ctx.integrate_params(Problem(PARAM, 0.0, 5.0, 1e-10), [0.0, 1.0])
    assert r.tasks == 5359


def test_cli_param_theta(trees):
    """`aquad --f param --theta 0,1` prints the reference's output for the Gaussian tree (one worker column),
    and a theta of the wrong length is refused before any device work."""
    from ppls_amd import build
    g = trees["gauss_eps1e-10"]
    cmd = [build.CLI, "--f", "param", "--eps", "1e-10"]
    out = subprocess.run(cmd + ["--theta", "0,1"], capture_output=True, text=True, timeout=120, check=True).stdout
    lines = out.splitlines()
    assert lines[0] == "Area=" + g["reference"]["area_printed"]
    assert lines[2] == "Tasks Per Process" and lines[3] == "0\t1\t"
    assert [int(v) for v in lines[4].split()] == [0, g["tasks"]]
    for bad in (["--theta", "0,1,2"], [], ["--theta", "0,x"]):
        p = subprocess.run(cmd + bad, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and p.stdout == ""


def test_param_buffers_are_allocated_on_first_use():
    """A fresh context holds no theta buffer (its footprint is that of any other fresh context); the first
    parametrised call allocates the device theta array, (NSLOTS + 1) x nparams doubles, and a batch call
    its four theta rings of at most MAXK rows each."""
    from ppls_amd import PARAM, Context, Problem, param_count
    with Context(0) as c, Context(0) as d:
        fresh = c.device_bytes
        assert fresh == d.device_bytes
        c.integrate(Problem(eps=1e-3))
        assert c.device_bytes == fresh
        c.integrate_params(Problem(PARAM, 0.0, 5.0, 1e-3), [0.0, 1.0])
        row = 8 * param_count()
        assert fresh < c.device_bytes <= fresh + row * (c.async_slots + 1)
        before = c.device_bytes
        a, b, theta, w = pr.draw_reference()
        c.integrate_batch_params(a[:100], b[:100], theta[:100], pr.DRAW_EPS)
        # the batch's own rings (140 B per row of a chunk, as for aq_integrate_batch, + 8 KiB) and theta's four
        assert c.device_bytes - before <= (140 + 4 * row) * 100 + 8192
