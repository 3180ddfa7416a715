"""Mesh coarsening on the GPU (aq_mesh_thresholds_batch, aq_mesh_budget_batch, aq_mesh_coarsen_batch and
Context.mesh_thresholds / mesh_coarsen) against tests/mesh_coarsen_reference.py and tests/mesh_batch_reference.py,
which share nothing with the code under test, and against the library's own aq_integrate_mesh_batch at the coarser eps.

The bounds: offsets, x, f, level, accepted, tasks, status, the thresholds and the budget's eps bit for bit; every cum
value within one ulp of the correctly rounded exact prefix of its own row (mesh_batch_cases derives it), and bit for bit
what the build from the roots gives whenever every row is coarsened at one eps; every output bit-identical between runs.

The cases are mesh_batch_reference's four, each coarsened to mesh_refine_reference.COARSE, and the synthetic row `comb`
(their shapes are asserted in tests/test_mesh_coarsen.py): at most 17 347 leaves, they reach a wave of 64, a scan chunk
of 256 leaves, several chunks per row, 307 rows of which most have one leaf, rows without nodes, a row at an odd
offset, positions on both sides of bit 64 and a depth of 100.

Not collected by name: tests/test_gpu_mesh_coarsen.py runs this file as one child pytest process that imports torch
before the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import ctypes
import types

import numpy as np
import pytest

import mesh_batch_reference as mbr
import mesh_coarsen_reference as mcr
import mesh_refine_reference as mrr
from mesh_batch_cases import FRONTIER_CAP, POISON, Raw, _bits, _check_against, _dev, _same_outputs

pytestmark = pytest.mark.gpu

AQ_EINVAL, AQ_EOVERFLOW = -1, -4
PARITY = ["edges", "param", "sin", "scale"]
BUDGETS = [1, 2, 64, 257]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


class Src:
    """A mesh on the device, as the coarsening calls read one: from a reference Batch, or a run trimmed to its nodes."""

    def __init__(self, torch, run, n_nodes=None):
        n_nodes = run.n_nodes if n_nodes is None else n_nodes
        self.n, self.n_nodes = run.offsets.shape[0] - 1, n_nodes
        self.offsets = _dev(torch, np.array(run.offsets, np.int64))
        # (a mesh without nodes: one element, so that the pointers are not NULL)
        self.x, self.f, self.level = (_dev(torch, getattr(run, k)[:max(n_nodes, 1)].copy()) for k in ("x", "f", "level"))


def _thresholds(ctx, torch, src, null=()):
    thr = torch.full((max(src.n_nodes, 1),), POISON, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    arg = lambda k, t: None if k in null else t.data_ptr()   # noqa: E731
    rc = ctx.L.aq_mesh_thresholds_batch(ctx._h, src.n, arg("in_offsets", src.offsets), arg("in_x", src.x), arg("in_f", src.f),
                                        arg("in_level", src.level), arg("thr", thr))
    return rc, thr


def _budget(ctx, torch, src, thr, K, null=()):
    eps = torch.full((src.n,), POISON, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    arg = lambda k, t: None if k in null else t.data_ptr()   # noqa: E731
    rc = ctx.L.aq_mesh_budget_batch(ctx._h, src.n, arg("in_offsets", src.offsets), arg("thr", thr), K, arg("eps", eps))
    return rc, eps


class Coarsen:
    """aq_mesh_coarsen_batch itself on fresh output tensors of `alloc` (>= cap_nodes) elements filled with a poison
    value; the arrays whole, on the host. eps: a float, or an array (n,) passed as d_eps; thr: a device tensor or None;
    null: names of arguments / aq_mesh_batch_io pointers to pass as NULL."""

    def __init__(self, ctx, torch, src, eps, cap_nodes, alloc=None, thr=None, null=(), n=None, with_info=True):
        from ppls_amd import _lib
        rows = src.n
        n = rows if n is None else n
        alloc = alloc or cap_nodes
        deps = _dev(torch, np.asarray(eps, np.float64)) if np.ndim(eps) else None
        x, f, cum = (torch.full((alloc,), POISON, dtype=torch.float64, device="cuda:0") for _ in range(3))
        lev = torch.full((alloc,), 201, dtype=torch.uint8, device="cuda:0")
        off = torch.full((rows + 1,), -3, dtype=torch.int64, device="cuda:0")
        area = torch.full((rows,), POISON, dtype=torch.float64, device="cuda:0")
        acc, tasks = (torch.full((rows,), -3, dtype=torch.int64, device="cuda:0") for _ in range(2))
        status = torch.full((rows,), -3, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = dict(a=None, b=None, theta=None, offsets=off, x=x, f=f, cum=cum, level=lev, area=area, accepted=acc,
                    tasks=tasks, status=status)
        io = _lib.aq_mesh_batch_io(*(None if (k in null or t is None) else t.data_ptr() for k, t in ptrs.items()), 0, 0)
        arg = lambda k, t: None if (k in null or t is None) else t.data_ptr()   # noqa: E731
        self.info = _lib.aq_mesh_coarsen_info(12345, 12345, 12345, 12345, 123, 123)
        self.rc = ctx.L.aq_mesh_coarsen_batch(
            ctx._h, n, arg("in_offsets", src.offsets), arg("in_x", src.x), arg("in_f", src.f), arg("in_level", src.level),
            arg("thr", thr), arg("eps", deps), 0.0 if deps is not None else float(eps),
            None if "io" in null else ctypes.byref(io), cap_nodes, ctypes.byref(self.info) if with_info else None)
        torch.cuda.synchronize()
        self.offsets, self.x, self.f, self.cum, self.level, self.area, self.accepted, self.tasks, self.status = (
            t.cpu().numpy() for t in (off, x, f, cum, lev, area, acc, tasks, status))


def _check_coarsened(run, ref, fine, name=""):
    """One successful coarsening against a reference Batch: mesh_batch_cases._check_against's checks (its info words
    that aq_mesh_coarsen_info lacks are taken from the reference), and merged."""
    info = run.info
    shim = types.SimpleNamespace(rc=run.rc, info=types.SimpleNamespace(
        n_nodes=info.n_nodes, leaves=info.leaves, tasks=info.tasks, invalid_rows=ref.invalid_rows, levels=info.levels,
        widest_level=ref.widest_level), **{k: getattr(run, k) for k in (
            "offsets", "x", "f", "cum", "level", "area", "accepted", "tasks", "status")})
    _check_against(shim, ref, name)
    assert info.merged == fine.leaves - ref.leaves and info.reserved == 0
    # the rows with nodes, from the call's own words (the shim's invalid_rows is the reference's)
    assert info.n_nodes - 2 * info.leaves == len(ref.rows) - ref.invalid_rows == 2 * info.leaves - info.tasks


def _arrays(m):
    """A MeshBatch's arrays on the host; level at a row's last node is unspecified, so it is zeroed here."""
    off, x, f, cum, level, area, acc, tasks, status = (
        t.cpu().numpy().copy() for t in (m.offsets, m.x, m.f, m.cum, m.level, m.area, m.accepted, m.tasks, m.status))
    level[off[1:][off[1:] > off[:-1]] - 1] = 0
    return off, x, f, cum, level, area, acc, tasks, status


def _fine(ctx, torch, name):
    """The library's own mesh of a case at its fine eps (checked against the reference), on the device."""
    integrand, a, b, theta, feps, fine = mbr.case(name)
    run = Raw(ctx, torch, integrand, a, b, theta, feps, fine.n_nodes)
    _check_against(run, fine, "%s built at %g" % (name, feps))
    return run, Src(torch, run, fine.n_nodes)


@pytest.mark.parametrize("name", PARITY)
def test_parity(ctx, torch, name):
    integrand, a, b, theta, feps, fine = mbr.case(name)
    ceps = mrr.COARSE[name]
    want = mcr.coarsen(fine, ceps)
    _, src = _fine(ctx, torch, name)
    m = want.n_nodes
    built = Raw(ctx, torch, integrand, a, b, theta, ceps, m, alloc=m + 64)
    _check_against(built, want, name + " built at the coarse eps")
    rc, thr = _thresholds(ctx, torch, src)
    assert rc == 0
    runs = [Coarsen(ctx, torch, src, ceps, m, alloc=m + 64, thr=t) for t in (None, None, thr)]
    for run in runs:
        _check_coarsened(run, want, fine, name)
        _same_outputs(run, built)            # one eps for all rows: cum, too, bit for bit the build's
    print(name, "merged", runs[0].info.merged, "leaves", runs[0].info.leaves, "levels", runs[0].info.levels)
    # the input's node count always suffices
    _check_coarsened(Coarsen(ctx, torch, src, ceps, fine.n_nodes), want, fine, name + ", the input's capacity")


@pytest.mark.parametrize("name", PARITY + ["comb"])
def test_thresholds(ctx, torch, name):
    fine = mcr.fine(name)
    src = Src(torch, fine)
    want = mcr.thresholds(fine)
    got = []
    for _ in range(2):
        rc, thr = _thresholds(ctx, torch, src)
        assert rc == 0
        got.append(thr.cpu().numpy())
    assert np.array_equal(_bits(got[0]), _bits(want)) and np.array_equal(_bits(got[0]), _bits(got[1]))
    if name != "comb":
        return
    o0, o1 = int(fine.offsets[1]), int(fine.offsets[2])
    t = want[o0 + 2:o1 - 1:2]
    assert np.all(np.diff(t) > 0)
    for e in (0.5 * (t[2] + t[3]), 0.5 * (t[36] + t[37]), 0.5 * (t[63] + t[64]), float(t[50])):   # the last: the strict >
        ref = mcr.coarsen(fine, e)
        run = Coarsen(ctx, torch, src, e, fine.n_nodes)
        _check_coarsened(run, ref, fine, "comb at %g" % e)
        assert run.accepted[1] == ref.accepted[1] < fine.accepted[1]
        _same_outputs(run, Coarsen(ctx, torch, src, e, fine.n_nodes, thr=thr))


def test_round_trips(ctx, torch):
    integrand, a, b, theta, feps, fine = mbr.case("edges")
    ceps = mrr.COARSE["edges"]
    da, db = _dev(torch, a), _dev(torch, b)
    mesh = ctx.integrate_mesh_batch(da, db, feps, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP)
    same = lambda u, v: all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(_arrays(u), _arrays(v)))   # noqa: E731
    coarse = ctx.mesh_coarsen(mesh, ceps)
    want = mcr.coarsen(fine, ceps)
    assert (coarse.n_nodes, coarse.leaves, coarse.merged, coarse.eps) == (want.n_nodes, want.leaves, fine.leaves - want.leaves, ceps)
    assert (coarse.integrand, coarse.theta, coarse.max_depth, coarse.invalid_rows) == (integrand, None, 0, 2)
    # refine back: the fine mesh bit for bit, and only the tasks that went are evaluated
    back = ctx.mesh_refine(coarse, feps, frontier_cap=FRONTIER_CAP)
    assert same(back, mesh) and back.evaluated == mesh.total_tasks - coarse.total_tasks
    # two hops equal one
    first = ctx.mesh_coarsen(mesh, mrr.EDGES_FIRST)
    assert first.leaves == 1098 and same(ctx.mesh_coarsen(coarse, mrr.EDGES_FIRST), first)
    # nothing merges at the input's eps, at 0 and under the mask
    for eps in (feps, 0.0, -1.0 * torch.ones(a.size, dtype=torch.float64, device="cuda:0")):
        out = ctx.mesh_coarsen(mesh, eps)
        assert out.merged == 0 and same(out, mesh)
    # the result is a MeshBatch like any other
    ea, _ = ctx.mesh_err(coarse)
    assert np.array_equal(np.isnan(ea.cpu().numpy()), want.status != 0)
    q = ctx.mesh_quantiles(coarse, [0.25, 0.5])
    assert q.shape == (a.size, 2)
    with pytest.raises(ValueError):
        ctx.mesh_coarsen(mesh)
    with pytest.raises(ValueError):
        ctx.mesh_coarsen(mesh, eps=1e-3, max_leaves=4)


def test_per_row_eps_and_mask(ctx, torch):
    integrand, a, b, theta, feps, fine = mbr.case("edges")
    assert (a[304], b[304]) == (0.0, 5.0)
    eps = np.full(a.size, -1.0)
    eps[304] = 1e-3
    eps[7] = np.nan                                                   # a NaN masks a row as -1 does
    want = mcr.coarsen(fine, eps)
    coarse = mrr.built("edges", 1e-3)
    run = Coarsen(ctx, torch, Src(torch, fine), eps, fine.n_nodes)
    _check_coarsened(run, want, fine, "row 304 alone")                # cum within 1 ulp of its exact value, every row
    for i in range(a.size):
        ref = coarse if i == 304 else fine
        o0, o1, r0, r1 = run.offsets[i], run.offsets[i + 1], ref.offsets[i], ref.offsets[i + 1]
        assert o1 - o0 == r1 - r0
        assert np.array_equal(_bits(run.x[o0:o1]), _bits(ref.x[r0:r1])) and np.array_equal(_bits(run.f[o0:o1]), _bits(ref.f[r0:r1]))
        assert np.array_equal(run.level[o0:max(o1 - 1, o0)], ref.level[r0:max(r1 - 1, r0)])


@pytest.mark.parametrize("name", ["edges", "param"])
def test_budget(ctx, torch, name):
    integrand, a, b, theta, feps, fine = mbr.case(name)
    src = Src(torch, fine)
    rc, thr = _thresholds(ctx, torch, src)
    assert rc == 0
    da, db, dth = _dev(torch, a), _dev(torch, b), _dev(torch, theta)
    mesh = ctx.integrate_mesh_batch(da, db, feps, integrand=integrand, theta=dth, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP)
    for K in BUDGETS:
        want_eps = mcr.budget_eps(fine, K)
        got = []
        for _ in range(2):
            rc, eps = _budget(ctx, torch, src, thr, K)
            assert rc == 0
            got.append(eps.cpu().numpy())
        assert np.array_equal(_bits(got[0]), _bits(want_eps)) and np.array_equal(_bits(got[0]), _bits(got[1]))
        want = mcr.coarsen(fine, want_eps)
        _check_coarsened(Coarsen(ctx, torch, src, got[0], fine.n_nodes, thr=thr), want, fine, "%s, %d leaves" % (name, K))
        out = ctx.mesh_coarsen(mesh, max_leaves=K)
        assert int(out.accepted.max()) <= K and np.array_equal(out.accepted.cpu().numpy(), want.accepted)
        assert np.array_equal(_bits(out.eps.cpu().numpy()), _bits(want_eps)) and np.array_equal(_bits(out.x.cpu().numpy()), _bits(want.x))
        print(name, "K", K, "leaves", out.leaves, "merged", out.merged)
        if name == "param" and K == 257:
            u = torch.linspace(0.0, 1.0, 33, dtype=torch.float64, device="cuda:0")
            q = ctx.mesh_quantiles(out, u).cpu().numpy()
            assert np.isfinite(q).all() and np.all(np.diff(q, axis=1) >= 0)


def test_capacities_and_arguments(torch):
    from ppls_amd import AquadError, Context
    integrand, a, b, theta, feps, fine = mbr.case("scale")
    ceps = mrr.COARSE["scale"]
    want = mcr.coarsen(fine, ceps)
    m = want.n_nodes
    src = Src(torch, fine)
    with Context(0) as c:
        before = c.device_bytes
        assert Coarsen(c, torch, src, ceps, m, null=("x",)).rc == AQ_EINVAL
        assert _thresholds(c, torch, src, null=("thr",))[0] == AQ_EINVAL
        assert c.device_bytes == before
        base = Coarsen(c, torch, src, ceps, m)
        _check_coarsened(base, want, fine, "scale")
        rc, thr = _thresholds(c, torch, src)
        assert rc == 0 and _budget(c, torch, src, thr, 4)[0] == 0
        after = c.device_bytes
        assert after > before
        assert Coarsen(c, torch, src, ceps, m).rc == 0 and _thresholds(c, torch, src)[0] == 0
        assert _budget(c, torch, src, thr, 4)[0] == 0 and c.device_bytes == after
        # too small a capacity reports the size; nothing is written at or past it
        run = Coarsen(c, torch, src, ceps, m - 1, alloc=m + 64)
        assert run.rc == AQ_EOVERFLOW and run.info.n_nodes == m and run.info.leaves == want.leaves
        for arr in (run.x, run.f, run.cum):
            assert np.all(arr[m - 1:] == POISON)
        assert np.all(run.level[m - 1:] == 201)
        _check_coarsened(Coarsen(c, torch, src, ceps, int(run.info.n_nodes), alloc=m + 64), want, fine, "retry")
        ok = dict(src=src, eps=ceps, cap_nodes=m)
        for name in ("io", "offsets", "x", "f", "cum", "in_offsets", "in_x", "in_f", "in_level"):
            assert Coarsen(c, torch, **ok, null=(name,)).rc == AQ_EINVAL, name
        assert Coarsen(c, torch, **ok, with_info=False).rc == AQ_EINVAL
        for name in ("level", "area", "accepted", "tasks", "status"):   # optional outputs
            run = Coarsen(c, torch, **ok, null=(name,))
            assert run.rc == 0 and np.array_equal(_bits(run.cum[:m]), _bits(base.cum[:m])), name
        assert Coarsen(c, torch, **dict(ok, eps=-1.0)).rc == AQ_EINVAL and Coarsen(c, torch, **dict(ok, eps=np.nan)).rc == AQ_EINVAL
        assert Coarsen(c, torch, **dict(ok, cap_nodes=2), alloc=16).rc == AQ_EINVAL
        assert Coarsen(c, torch, **dict(ok, cap_nodes=(1 << 31) + 1), alloc=16).rc == AQ_EINVAL
        for name in ("in_offsets", "in_x", "in_f", "in_level"):
            assert _thresholds(c, torch, src, null=(name,))[0] == AQ_EINVAL, name
        for name in ("in_offsets", "thr", "eps"):
            assert _budget(c, torch, src, thr, 4, null=(name,))[0] == AQ_EINVAL, name
        assert _budget(c, torch, src, thr, 0)[0] == AQ_EINVAL
        # more rows than 2^31 - 1, and an input of more than 2^31 nodes: refused before anything is allocated or enqueued
        held = c.device_bytes
        assert Coarsen(c, torch, **ok, n=0x80000000).rc == AQ_EINVAL
        call = c.L.aq_mesh_thresholds_batch
        assert call(c._h, 0x80000000, src.offsets.data_ptr(), src.x.data_ptr(), src.f.data_ptr(), src.level.data_ptr(),
                    thr.data_ptr()) == AQ_EINVAL
        one_eps = torch.full((1,), POISON, dtype=torch.float64, device="cuda:0")
        assert c.L.aq_mesh_budget_batch(c._h, 0x80000000, src.offsets.data_ptr(), thr.data_ptr(), 4, one_eps.data_ptr()) == AQ_EINVAL
        huge = types.SimpleNamespace(n=1, n_nodes=1, offsets=_dev(torch, np.array([0, 2 ** 31 + 1], np.int64)),
                                     x=src.x, f=src.f, level=src.level)
        assert Coarsen(c, torch, huge, ceps, m).rc == AQ_EINVAL
        rc, t1 = _thresholds(c, torch, huge)
        assert rc == AQ_EINVAL and np.all(t1.cpu().numpy() == POISON)
        rc, e1 = _budget(c, torch, huge, thr, 4)
        assert rc == AQ_EINVAL and np.all(e1.cpu().numpy() == POISON)
        assert c.device_bytes == held and np.all(one_eps.cpu().numpy() == POISON)
        run = Coarsen(c, torch, **ok, n=0)
        assert run.rc == 0 and np.all(run.x == POISON) and np.all(run.offsets == -3)
        i = run.info
        assert (i.n_nodes, i.leaves, i.tasks, i.merged, i.levels, i.reserved) == (0,) * 6
        assert c.L.aq_mesh_thresholds_batch(c._h, 0, None, None, None, None, None) == 0
        assert c.L.aq_mesh_budget_batch(c._h, 0, None, None, 4, None) == 0
        # every row invalid: a mesh without nodes stays one
        bad = Raw(c, torch, mbr.COSH4, np.array([2.0, 0.0, np.nan]), np.array([1.0, 171.0, 1.0]), None, 1e-3, 16)
        assert bad.rc == 0 and bad.info.n_nodes == 0
        none = Src(torch, bad, 0)
        run = Coarsen(c, torch, none, 1e-1, 16)
        assert run.rc == 0 and (run.info.n_nodes, run.info.leaves, run.info.merged, run.info.levels) == (0, 0, 0, 0)
        assert np.all(run.offsets == 0) and np.all(run.status == mbr.ROW_INVALID) and np.isnan(run.area).all()
        assert np.all(run.accepted == 0) and np.all(run.tasks == 0) and np.all(run.x == POISON)
        rc, t0 = _thresholds(c, torch, none)
        assert rc == 0 and np.all(t0.cpu().numpy() == POISON)
        rc, e0 = _budget(c, torch, none, t0, 4)
        assert rc == 0 and np.all(e0.cpu().numpy() == -1.0)
        # the Python surface reports the size as the other mesh calls do
        mesh = c.integrate_mesh_batch(_dev(torch, a), _dev(torch, b), feps, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP)
        with pytest.raises(AquadError) as e:
            c.mesh_coarsen(mesh, ceps, cap_nodes=16)
        assert e.value.code == AQ_EOVERFLOW and e.value.n_nodes == m


def test_interleaved_on_one_context(torch):
    """build -> coarsen -> refine -> integrate_mesh of one row -> build again -> a budget on ONE context: every result is
    what the same call gives on a fresh context, bit for bit (the coarsen call borrows the builds' leaf buffer and sort
    arrays, the budget their sort arrays)."""
    from ppls_amd import Context, Problem
    integrand, a, b, theta, feps, fine = mbr.case("edges")
    ceps = mrr.COARSE["edges"]
    one = Problem(integrand=integrand, a=0.0, b=5.0, eps=ceps)
    da, db = _dev(torch, a), _dev(torch, b)
    cap_one = 2 * int(mrr.built("edges", ceps).accepted[304]) + 1

    def host(*tensors):
        return [t.cpu().numpy().copy() for t in tensors]

    def build(c):
        return c.integrate_mesh_batch(da, db, feps, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP)

    def single(c):
        r, x, f, cum, level = c.integrate_mesh(one, cap_nodes=cap_one, frontier_cap=FRONTIER_CAP)
        return host(x, f, cum, level)

    def same(got, want):
        assert len(got) == len(want) and all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))

    with Context(0) as fresh:
        mesh = build(fresh)
        want_built = _arrays(mesh)
    with Context(0) as fresh:
        coarse = fresh.mesh_coarsen(mesh, ceps)
        want_coarse = _arrays(coarse)
    with Context(0) as fresh:
        want_refined = _arrays(fresh.mesh_refine(coarse, feps, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP))
    with Context(0) as fresh:
        want_single = single(fresh)
    with Context(0) as fresh:
        want_budget = _arrays(fresh.mesh_coarsen(mesh, max_leaves=64))
    same(want_refined, want_built)

    with Context(0) as c:
        built = build(c)
        same(_arrays(built), want_built)
        got = c.mesh_coarsen(built, ceps)
        same(_arrays(got), want_coarse)
        same(_arrays(c.mesh_refine(got, feps, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP)), want_refined)
        same(single(c), want_single)
        same(_arrays(build(c)), want_built)
        same(_arrays(c.mesh_coarsen(built, max_leaves=64)), want_budget)   # (the budget sorts in the builds' arrays)
