"""Mesh refinement on the GPU (aq_mesh_refine_batch, aq_mesh_err_batch and Context.mesh_refine / mesh_err /
integrate_mesh_batch_tol) against tests/mesh_refine_reference.py and tests/mesh_batch_reference.py, which share
nothing with the code under test, and against the library's own aq_integrate_mesh_batch at the finer eps.

The bounds: offsets, x, f, level, accepted, tasks and status bit for bit; every cum value within one ulp of the
correctly rounded exact prefix of its own row (mesh_batch_cases derives it), and bit for bit what the build from the
roots gives whenever every row was active; the error sums within the bounds include/aquad.h states (derived there, not
measured); the counts -- evaluated, reseeded, widest_level -- exactly the reference's.

The cases are mesh_batch_reference's, each continued from a coarser eps (mesh_refine_reference.COARSE; their shapes
are asserted in tests/test_mesh_refine.py): they reach a wave of 64, a scan block of 256, a level chunk of 1024 and
seeds that arrive at levels the run has already begun.

Not collected by name: tests/test_gpu_mesh_refine.py runs this file as one child pytest process that imports torch
before the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import ctypes
import os
import types
from fractions import Fraction

import numpy as np
import pytest

import mesh_batch_reference as mbr
import mesh_refine_reference as mrr
import param_reference as pr
import tol_reference as tr
from mesh_batch_cases import FRONTIER_CAP, POISON, Raw, _bits, _check_against, _dev, _same_outputs

pytestmark = pytest.mark.gpu

AQ_EINVAL, AQ_EOVERFLOW, AQ_EDEPTH = -1, -4, -5
PARITY = ["edges", "param", "sin", "scale"]


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
    """A mesh on the device, as aq_mesh_refine_batch reads one: from a Raw / Refine run, trimmed to its nodes."""

    def __init__(self, torch, run, n_nodes):
        self.offsets = _dev(torch, run.offsets)
        # (a mesh without nodes: one element, so that the pointers are not NULL)
        self.x, self.f, self.level = (_dev(torch, getattr(run, k)[:max(n_nodes, 1)].copy()) for k in ("x", "f", "level"))


class Refine:
    """aq_mesh_refine_batch itself on fresh output tensors of `alloc` (>= cap_nodes) elements filled with a poison
    value; the arrays whole, on the host. null: names of arguments / aq_mesh_batch_io pointers to pass as NULL."""

    def __init__(self, ctx, torch, src, integrand, theta, eps, cap_nodes, alloc=None, active=None,
                 frontier_cap=FRONTIER_CAP, sync_every=4, max_depth=0, null=(), n=None, with_info=True):
        from ppls_amd import _lib
        rows = src.offsets.shape[0] - 1
        n = rows if n is None else n
        alloc = alloc or cap_nodes
        dth = _dev(torch, theta)
        dact = None if active is None else _dev(torch, np.asarray(active, np.uint8))
        x, f, cum = (torch.full((alloc,), POISON, dtype=torch.float64, device="cuda:0") for _ in range(3))
        lev = torch.full((alloc,), 201, dtype=torch.uint8, device="cuda:0")
        off = torch.full((rows + 1,), -3, dtype=torch.int64, device="cuda:0")
        area = torch.full((rows,), POISON, dtype=torch.float64, device="cuda:0")
        acc, tasks = (torch.full((rows,), -3, dtype=torch.int64, device="cuda:0") for _ in range(2))
        status = torch.full((rows,), -3, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = dict(a=None, b=None, theta=None, offsets=off, x=x, f=f, cum=cum, level=lev, area=area, accepted=acc,
                    tasks=tasks, status=status)
        io = _lib.aq_mesh_batch_io(*(None if (k in null or t is None) else t.data_ptr() for k, t in ptrs.items()),
                                   int(max_depth), 0)
        arg = lambda k, t: None if (k in null or t is None) else t.data_ptr()   # noqa: E731
        self.info = _lib.aq_mesh_refine_info(12345, 12345, 12345, 12345, 12345, 123, 123)
        self.rc = ctx.L.aq_mesh_refine_batch(
            ctx._h, n, arg("in_offsets", src.offsets), arg("in_x", src.x), arg("in_f", src.f), arg("in_level", src.level),
            arg("in_theta", dth), arg("active", dact), float(eps), integrand, None if "io" in null else ctypes.byref(io),
            frontier_cap, sync_every, cap_nodes, ctypes.byref(self.info) if with_info else None)
        torch.cuda.synchronize()
        self.offsets, self.x, self.f, self.cum, self.level, self.area, self.accepted, self.tasks, self.status = (
            t.cpu().numpy() for t in (off, x, f, cum, lev, area, acc, tasks, status))


def _check_refined(run, ref, name=""):
    """One successful refinement against a reference Batch: mesh_batch_cases._check_against's checks (its info words
    that aq_mesh_refine_info lacks or defines otherwise are taken from the reference)."""
    info = run.info
    shim = types.SimpleNamespace(rc=run.rc, info=types.SimpleNamespace(
        n_nodes=info.n_nodes, leaves=info.leaves, tasks=info.tasks, invalid_rows=ref.invalid_rows, levels=info.levels,
        widest_level=ref.widest_level), **{k: getattr(run, k) for k in (
            "offsets", "x", "f", "cum", "level", "area", "accepted", "tasks", "status")})
    _check_against(shim, ref, name)


def _coarse(ctx, torch, name, eps=None):
    """The library's own mesh of a case at its coarse eps (checked), and that mesh on the device."""
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case(name)
    if eps is not None:
        ceps, coarse = eps, mrr.built(name, eps)
    run = Raw(ctx, torch, integrand, a, b, theta, ceps, coarse.n_nodes)
    _check_against(run, coarse, "%s built at %g" % (name, ceps))
    return run, Src(torch, run, coarse.n_nodes)


@pytest.mark.parametrize("name", PARITY)
def test_parity(ctx, torch, name):
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case(name)
    crun, src = _coarse(ctx, torch, name)
    m = fine.n_nodes
    built = Raw(ctx, torch, integrand, a, b, theta, feps, m, alloc=m + 64)
    _check_against(built, fine, name + " built")
    runs = []
    for sync_every in (1, 4, 4):
        run = Refine(ctx, torch, src, integrand, theta, feps, m, alloc=m + 64, sync_every=sync_every)
        _check_refined(run, fine, "%s sync_every %d" % (name, sync_every))
        i = run.info
        print(name, "evaluated", i.evaluated, "reseeded", i.reseeded, "widest level", i.widest_level, "levels", i.levels)
        assert i.evaluated == built.info.tasks - crun.info.tasks == rf.evaluated
        assert (i.reseeded, i.widest_level, i.levels) == (rf.reseeded, rf.widest_level, fine.levels)
        _same_outputs(run, built)            # every row active: cum, too, bit for bit the build's
        runs.append(run)
    for other in runs[1:]:
        _same_outputs(runs[0], other)


def test_two_hops_equal_one_and_the_build(ctx, torch):
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("edges")
    _, src0 = _coarse(ctx, torch, "edges", mrr.EDGES_FIRST)
    hop1 = Refine(ctx, torch, src0, integrand, theta, ceps, coarse.n_nodes)
    _check_refined(hop1, coarse, "1e-1 -> 1e-3")
    m = fine.n_nodes
    hop2 = Refine(ctx, torch, Src(torch, hop1, coarse.n_nodes), integrand, theta, feps, m, alloc=m + 64)
    _check_refined(hop2, fine, "1e-3 -> 1e-5")
    _, src1 = _coarse(ctx, torch, "edges")
    _same_outputs(hop2, Refine(ctx, torch, src1, integrand, theta, feps, m, alloc=m + 64))
    _same_outputs(hop2, Raw(ctx, torch, integrand, a, b, theta, feps, m, alloc=m + 64))
    first = mrr.built("edges", mrr.EDGES_FIRST)
    assert hop1.info.evaluated + hop2.info.evaluated == fine.tasks_total - first.tasks_total


def test_mask_refines_one_row(ctx, torch):
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("edges")
    assert (a[304], b[304]) == (0.0, 5.0)
    active = np.zeros(a.size, np.uint8)
    active[304] = 1
    want = mrr.refine(coarse, integrand, theta, feps, active=active)
    assert want.changed == [304]
    _, src = _coarse(ctx, torch, "edges")
    m = want.batch.n_nodes
    run = Refine(ctx, torch, src, integrand, theta, feps, m, alloc=m + 64, active=active)
    _check_refined(run, want.batch, "mask")       # cum within 1 ulp of its exact value, every row
    assert (run.info.evaluated, run.info.reseeded, run.info.widest_level) == (
        want.evaluated, want.reseeded, want.widest_level)
    assert run.info.evaluated == want.batch.tasks_total - coarse.tasks_total
    for i in range(a.size):
        ref = fine if i == 304 else coarse
        o0, o1, r0, r1 = run.offsets[i], run.offsets[i + 1], ref.offsets[i], ref.offsets[i + 1]
        assert o1 - o0 == r1 - r0
        assert np.array_equal(_bits(run.x[o0:o1]), _bits(ref.x[r0:r1])) and np.array_equal(_bits(run.f[o0:o1]), _bits(ref.f[r0:r1]))
        assert np.array_equal(run.level[o0:max(o1 - 1, o0)], ref.level[r0:max(r1 - 1, r0)])


def test_no_op_at_the_inputs_eps_and_above(ctx, torch):
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("edges")
    crun, src = _coarse(ctx, torch, "edges")
    for eps in (ceps, 4 * ceps, 1e300):
        run = Refine(ctx, torch, src, integrand, theta, eps, coarse.n_nodes)
        _check_refined(run, coarse, "no-op at %g" % eps)
        assert (run.info.evaluated, run.info.reseeded, run.info.widest_level) == (0, 0, 0)
        _same_outputs(run, crun)


def test_edges_when_a_workgroup_takes_several_chunks(torch):
    """AQ_LEVEL_GRID=2 (read when the context is created): two workgroups walk every level's chunks."""
    from ppls_amd import Context
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("edges")
    old = os.environ.get("AQ_LEVEL_GRID")
    os.environ["AQ_LEVEL_GRID"] = "2"
    try:
        c = Context(0)
    finally:
        if old is None:
            del os.environ["AQ_LEVEL_GRID"]
        else:
            os.environ["AQ_LEVEL_GRID"] = old
    with c:
        _, src = _coarse(c, torch, "edges")
        m = fine.n_nodes
        runs = [Refine(c, torch, src, integrand, theta, feps, m, alloc=m + 64, sync_every=s) for s in (1, 4)]
        for run in runs:
            _check_refined(run, fine, "edges, grid 2")
            assert run.info.evaluated == rf.evaluated
        _same_outputs(*runs)


def test_capacities_and_depth(ctx, torch):
    from ppls_amd import AquadError
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("edges")
    _, src = _coarse(ctx, torch, "edges")
    m = fine.n_nodes
    run = Refine(ctx, torch, src, integrand, theta, feps, m - 1, alloc=m + 64)
    assert run.rc == AQ_EOVERFLOW and run.info.n_nodes == m and run.info.leaves == fine.leaves
    for arr in (run.x, run.f, run.cum):
        assert np.all(arr[m - 1:] == POISON)
    assert np.all(run.level[m - 1:] == 201)
    _check_refined(Refine(ctx, torch, src, integrand, theta, feps, int(run.info.n_nodes), alloc=m + 64), fine, "retry")
    assert rf.widest_level == 7790
    run = Refine(ctx, torch, src, integrand, theta, feps, m, frontier_cap=7789)
    assert run.rc == AQ_EOVERFLOW and run.info.n_nodes == 0
    _check_refined(Refine(ctx, torch, src, integrand, theta, feps, m, frontier_cap=7790), fine, "frontier_cap == widest")
    assert fine.rows[304].levels == 18
    run = Refine(ctx, torch, src, integrand, theta, feps, m, max_depth=16)
    assert run.rc == AQ_EDEPTH and run.info.n_nodes == 0
    assert np.array_equal(run.status, fine.depth_status(16)) and run.status[304] == mbr.ROW_DEPTH
    # a failing input leaf that would itself refine at max_depth (the coarse tree of [0, 5] is deeper than 8 levels)
    assert coarse.rows[304].levels > 8
    run = Refine(ctx, torch, src, integrand, theta, feps, m, max_depth=8)
    assert run.rc == AQ_EDEPTH and np.array_equal(run.status, fine.depth_status(8))
    _check_refined(Refine(ctx, torch, src, integrand, theta, feps, m, max_depth=18), fine, "max_depth == the deepest row's levels")
    # the Python surface: 4 x the input's nodes is too few here, so the retry with the reported size runs
    assert 4 * coarse.n_nodes < m
    mesh = ctx.integrate_mesh_batch(_dev(torch, a), _dev(torch, b), ceps, frontier_cap=FRONTIER_CAP)
    assert (mesh.integrand, mesh.theta, mesh.eps, mesh.max_depth) == (integrand, None, ceps, 0)
    out = ctx.mesh_refine(mesh, feps, frontier_cap=FRONTIER_CAP)
    assert (out.n_nodes, out.evaluated, out.reseeded, out.eps, out.invalid_rows) == (m, rf.evaluated, rf.reseeded, feps, 2)
    assert out.total_tasks == fine.tasks_total and np.array_equal(_bits(out.x.cpu().numpy()), _bits(fine.x))
    with pytest.raises(AquadError) as e:
        ctx.mesh_refine(mesh, feps, cap_nodes=1000, frontier_cap=FRONTIER_CAP)
    assert e.value.code == AQ_EOVERFLOW and e.value.n_nodes == m


def test_refused_arguments(ctx, torch):
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("scale")
    _, src = _coarse(ctx, torch, "scale")
    m = fine.n_nodes
    ok = dict(src=src, integrand=integrand, theta=None, eps=feps, cap_nodes=m)
    base = Refine(ctx, torch, **ok)
    _check_refined(base, fine, "scale")
    for name in ("io", "offsets", "x", "f", "cum", "in_offsets", "in_x", "in_f", "in_level"):
        assert Refine(ctx, torch, **ok, null=(name,)).rc == AQ_EINVAL, name
    assert Refine(ctx, torch, **ok, with_info=False).rc == AQ_EINVAL
    for name in ("level", "area", "accepted", "tasks", "status"):   # optional outputs
        run = Refine(ctx, torch, **ok, null=(name,))
        assert run.rc == 0 and np.array_equal(_bits(run.cum[:m]), _bits(base.cum[:m])), name
    th = np.tile([0.0, 1.0], (a.size, 1))
    assert Refine(ctx, torch, **dict(ok, theta=th)).rc == AQ_EINVAL                    # theta with a fixed integrand
    assert Refine(ctx, torch, **dict(ok, integrand=mbr.PARAM)).rc == AQ_EINVAL         # PARAM without theta
    assert Refine(ctx, torch, **dict(ok, integrand=7)).rc == AQ_EINVAL
    assert Refine(ctx, torch, **dict(ok, eps=-1.0)).rc == AQ_EINVAL and Refine(ctx, torch, **dict(ok, eps=np.nan)).rc == AQ_EINVAL
    assert Refine(ctx, torch, **ok, max_depth=-1).rc == AQ_EINVAL and Refine(ctx, torch, **ok, max_depth=128).rc == AQ_EINVAL
    assert Refine(ctx, torch, **ok, sync_every=0).rc == AQ_EINVAL
    assert Refine(ctx, torch, **ok, frontier_cap=1).rc == AQ_EINVAL
    assert Refine(ctx, torch, **ok, frontier_cap=2).rc == AQ_EOVERFLOW                 # accepted: no relation to n = 3
    assert Refine(ctx, torch, **dict(ok, cap_nodes=2), alloc=16).rc == AQ_EINVAL
    assert Refine(ctx, torch, **dict(ok, cap_nodes=(1 << 31) + 1), alloc=16).rc == AQ_EINVAL
    run = Refine(ctx, torch, **ok, n=0)
    assert run.rc == 0 and np.all(run.x == POISON) and np.all(run.offsets == -3)
    i = run.info
    assert (i.n_nodes, i.leaves, i.tasks, i.evaluated, i.reseeded, i.levels, i.widest_level) == (0,) * 7
    d = torch.zeros(16, dtype=torch.float64, device="cuda:0").data_ptr()
    call = ctx.L.aq_mesh_err_batch
    assert call(ctx._h, 1, None, d, d, d, d) == AQ_EINVAL and call(ctx._h, 1, d, None, d, d, d) == AQ_EINVAL
    assert call(ctx._h, 1, d, d, None, d, d) == AQ_EINVAL and call(ctx._h, 0, None, None, None, None, None) == 0


def test_rows_without_nodes_and_device_memory(torch):
    from ppls_amd import Context
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("scale")
    with Context(0) as c:
        crun, src = _coarse(c, torch, "scale")
        before = c.device_bytes
        assert Refine(c, torch, src, integrand, theta, feps, fine.n_nodes, null=("x",)).rc == AQ_EINVAL
        assert c.device_bytes == before
        _check_refined(Refine(c, torch, src, integrand, theta, feps, fine.n_nodes), fine, "scale")
        after = c.device_bytes
        assert after > before
        assert Refine(c, torch, src, integrand, theta, feps, fine.n_nodes).rc == 0
        assert c.device_bytes == after
        # every row invalid: a mesh without nodes stays one
        bad = Raw(c, torch, mbr.COSH4, np.array([2.0, 0.0, np.nan]), np.array([1.0, 171.0, 1.0]), None, 1e-3, 16)
        assert bad.rc == 0 and bad.info.n_nodes == 0
        run = Refine(c, torch, Src(torch, bad, 0), mbr.COSH4, None, 1e-5, 16)
        assert run.rc == 0 and run.info.n_nodes == 0 and run.info.evaluated == 0
        assert np.all(run.offsets == 0) and np.all(run.status == mbr.ROW_INVALID) and np.isnan(run.area).all()
        assert np.all(run.accepted == 0) and np.all(run.tasks == 0) and np.all(run.x == POISON)


def test_walks_interleaved_on_one_context(torch):
    """The frontier walk's callers in turn on ONE context -- aq_frontier_integrate and integrate_mesh of one row,
    integrate_mesh_batch, mesh_refine, then the first two again: every result is what the same call gives on a fresh
    context, the meshes bit for bit. Then one plain aq_level_step on a caller-owned frontier folds at once (its
    accumulator is final once the device is idle, without aq_synchronize): the walks put defer_fold back."""
    from ppls_amd import Context, Problem
    from ppls_amd.frontier import HipStepper
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("edges")
    assert (a[304], b[304]) == (0.0, 5.0)
    one = Problem(integrand=integrand, a=0.0, b=5.0, eps=ceps)
    da, db = _dev(torch, a), _dev(torch, b)

    def host(*tensors):
        return [t.cpu().numpy().copy() for t in tensors]

    def integral(c):
        r = HipStepper(c).integrate_one_gpu(one, FRONTIER_CAP)
        return r.area, r.tasks, r.accepted, r.levels

    def mesh(c):
        r, x, f, cum, level = c.integrate_mesh(one, cap_nodes=2 * coarse.rows[304].accepted + 1, frontier_cap=FRONTIER_CAP)
        return (r.area, r.tasks, r.accepted), host(x, f, cum, level)

    def batch(c):
        return c.integrate_mesh_batch(da, db, ceps, cap_nodes=coarse.n_nodes, frontier_cap=FRONTIER_CAP)

    def arrays(m):
        return host(m.x, m.f, m.cum, m.level, m.offsets)

    def level_step(c):
        fin, out = (torch.zeros((4, 4), dtype=torch.float64, device="cuda:0") for _ in range(2))
        nout = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        acc = torch.zeros(8, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        st = HipStepper(c)
        st.root(integrand, 0.0, 5.0, fin)
        st.step(integrand, fin, 1, out, 4, ceps, 0, 96, nout, acc)
        torch.cuda.synchronize()              # every stream of the device, the context's among them: no fold of its own
        return host(acc, nout, out)

    def same(got, want):
        assert len(got) == len(want) and all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))

    with Context(0) as fresh:
        want_integral = integral(fresh)
    with Context(0) as fresh:
        want_mesh = mesh(fresh)
    with Context(0) as fresh:
        want_batch = batch(fresh)
        want_refined = arrays(fresh.mesh_refine(want_batch, feps, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP))
        want_batch = arrays(want_batch)
    with Context(0) as fresh:
        want_step = level_step(fresh)
    assert want_step[0][2] == 1 and want_step[1][0] == 2      # the root's task, folded; its two children
    assert want_integral[1:] == (coarse.rows[304].tasks, coarse.rows[304].accepted, coarse.rows[304].levels)

    with Context(0) as c:
        assert integral(c) == want_integral
        got = mesh(c)
        assert got[0] == want_mesh[0]
        same(got[1], want_mesh[1])
        built = batch(c)
        same(arrays(built), want_batch)
        refined = c.mesh_refine(built, feps, cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP)
        same(arrays(refined), want_refined)
        assert (refined.evaluated, refined.reseeded) == (rf.evaluated, rf.reseeded)
        assert integral(c) == want_integral
        got = mesh(c)
        assert got[0] == want_mesh[0]
        same(got[1], want_mesh[1])
        same(level_step(c), want_step)


def _err(ctx, torch, off, x, f, n):
    ea, es = (torch.full((n,), POISON, dtype=torch.float64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    assert ctx.L.aq_mesh_err_batch(ctx._h, n, off.data_ptr(), x.data_ptr(), f.data_ptr(), ea.data_ptr(), es.data_ptr()) == 0
    ctx.synchronize()
    return ea.cpu().numpy(), es.cpu().numpy()


@pytest.mark.parametrize("name", ["edges", "param", "sin"])
def test_err_sums(ctx, torch, name):
    """Both bounds are derived: the double-double sum lies within accepted * 2^-100 * Σ|d| of the exact sum before its
    one rounding (include/aquad.h), which adds half an ulp of the exact value. For err_abs, a sum of non-negative
    terms, accepted * 2^-100 is far below half an ulp, so the result is the exact rounding or its neighbour."""
    integrand, a, b, theta, eps, ref = mbr.case(name)
    n = a.size
    off, x, f = _dev(torch, ref.offsets), _dev(torch, ref.x), _dev(torch, ref.f)
    ea, es = _err(ctx, torch, off, x, f, n)
    exact = mrr.err_exact(ref)
    worst_abs = worst_sgn = 0.0
    for i, (A, S, leaves) in enumerate(exact):
        if A is None:
            assert np.isnan(ea[i]) and np.isnan(es[i])
            continue
        assert abs(Fraction(float(ea[i])) - A) <= Fraction(float(np.spacing(float(A))))          # within 1 ulp
        bound = leaves * Fraction(2) ** -100 * A + Fraction(float(np.spacing(abs(float(S))))) / 2
        assert abs(Fraction(float(es[i])) - S) <= bound
        worst_abs = max(worst_abs, float(abs(Fraction(float(ea[i])) - A) / Fraction(float(np.spacing(float(A))))))
        worst_sgn = max(worst_sgn, float(abs(Fraction(float(es[i])) - S) / bound))
    print(name, "err_abs: worst deviation in ulp", worst_abs, "err_signed: worst deviation / bound", worst_sgn)
    assert sum(e[0] is None for e in exact) == ref.invalid_rows
    ea2, es2 = _err(ctx, torch, off, x, f, n)                       # a second run
    assert np.array_equal(_bits(ea), _bits(ea2)) and np.array_equal(_bits(es), _bits(es2))
    # the same rows in another batch: every second row, so every offset moves
    rows = np.arange(0, n, 2)
    sub = mbr.Batch([ref.rows[i] for i in rows])
    sa, ss = _err(ctx, torch, _dev(torch, sub.offsets), _dev(torch, sub.x), _dev(torch, sub.f), rows.size)
    assert np.array_equal(_bits(sa), _bits(ea[rows])) and np.array_equal(_bits(ss), _bits(es[rows]))
    # either output may be NULL
    only = torch.full((n,), POISON, dtype=torch.float64, device="cuda:0")
    assert ctx.L.aq_mesh_err_batch(ctx._h, n, off.data_ptr(), x.data_ptr(), f.data_ptr(), None, only.data_ptr()) == 0
    ctx.synchronize()
    assert np.array_equal(_bits(only.cpu().numpy()), _bits(es))


def _tol_sets():
    a, b, ref = tr.set_c(n=64)
    k = tr.SET_C
    yield "cosh4", 0, a, b, None, dict(epsabs=k["epsabs"], epsrel=k["epsrel"], eps0=k["eps0"], shrink=k["shrink"],
                                       max_rounds=k["max_rounds"]), ref
    k = tr.SET_P
    a, b, theta = pr.draw(64)
    kw = dict(epsabs=k["epsabs"], epsrel=k["epsrel"], eps0=k["eps0"], shrink=k["shrink"], max_rounds=k["max_rounds"])
    yield "param", mbr.PARAM, a, b, theta, kw, tr.run(a, b, mbr.PARAM, theta=theta, **kw)


@pytest.mark.parametrize("which", ["cosh4", "param"])
def test_tolerance_driven_meshes(ctx, torch, which):
    name, integrand, a, b, theta, kw, ref = next(s for s in _tol_sets() if s[0] == which)
    assert ref["ratio_min"] >= tr.SAFE            # before any decision is relied on
    da, db, dth = _dev(torch, a), _dev(torch, b), _dev(torch, theta)
    res = ctx.integrate_mesh_batch_tol(da, db, integrand=integrand, theta=dth, frontier_cap=1 << 16, **kw)
    rounds, eps_used = res.rounds.cpu().numpy(), res.eps_used.cpu().numpy()
    print(which, "rounds", np.bincount(np.abs(rounds)), "evaluated", res.evaluated, "nodes", res.mesh.n_nodes)
    assert np.array_equal(rounds, ref["rounds"]) and np.array_equal(_bits(eps_used), _bits(ref["eps_used"]))
    assert res.converged == bool((ref["rounds"] > 0).all())
    tasks = res.mesh.tasks.cpu().numpy()
    assert np.array_equal(tasks, ref["tasks"]) and np.array_equal(res.mesh.accepted.cpu().numpy(), ref["leaves"])
    assert res.evaluated == int(tasks.sum())      # over all rounds every task of the final trees ran exactly once
    ea, es = res.err_abs.cpu().numpy(), res.err_signed.cpu().numpy()
    assert np.all(np.abs(ea - ref["err_abs"]) <= tr.row_tol(ref)) and np.all(np.abs(es - ref["err_signed"]) <= tr.row_tol(ref))
    off = res.mesh.offsets.cpu().numpy()
    x, f, level = (t.cpu().numpy() for t in (res.mesh.x, res.mesh.f, res.mesh.level))
    for i in range(a.size):                       # row i's mesh is the mesh at eps_used[i], built on that row alone
        one = ctx.integrate_mesh_batch(da[i:i + 1].clone(), db[i:i + 1].clone(), float(eps_used[i]), integrand=integrand,
                                       theta=None if dth is None else dth[i:i + 1].clone(),
                                       cap_nodes=int(off[i + 1] - off[i]), frontier_cap=1 << 16)
        o0, o1 = off[i], off[i + 1]
        assert one.n_nodes == o1 - o0
        assert np.array_equal(_bits(one.x.cpu().numpy()), _bits(x[o0:o1]))
        assert np.array_equal(_bits(one.f.cpu().numpy()), _bits(f[o0:o1]))
        assert np.array_equal(one.level.cpu().numpy()[:-1], level[o0:o1 - 1])
    if which == "cosh4":
        t = ctx.integrate_batch_tol(a, b, **kw)
        assert np.array_equal(t[6], rounds) and np.array_equal(_bits(t[5]), _bits(eps_used))
    for bad in (dict(epsabs=0.0, epsrel=0.0), dict(epsrel=-1.0), dict(epsrel=1e-6, eps0=0.0), dict(epsrel=1e-6, shrink=1.5),
                dict(epsrel=1e-6, max_rounds=65), dict(epsrel=1e-6, eps0=1e-300, max_rounds=12)):
        with pytest.raises(ValueError):
            ctx.integrate_mesh_batch_tol(da, db, integrand=integrand, theta=dth, **bad)


def test_tolerance_with_an_invalid_row(ctx, torch):
    a, b = np.array([0.0, 2.0, 0.0]), np.array([1.0, 1.0, 2.0])
    res = ctx.integrate_mesh_batch_tol(_dev(torch, a), _dev(torch, b), epsrel=1e-6, frontier_cap=1 << 16)
    rounds = res.rounds.cpu().numpy()
    assert rounds[1] == -1 and rounds[0] > 0 and rounds[2] > 0 and not res.converged
    assert np.isnan(res.err_abs.cpu().numpy()[1]) and np.isnan(res.err_signed.cpu().numpy()[1])
    assert res.eps_used.cpu().numpy()[1] == 1e-3 and res.mesh.status.cpu().numpy()[1] == mbr.ROW_INVALID
    want = tr.run(a[[0, 2]], b[[0, 2]], 0, 0.0, 1e-6, 1e-3)
    assert want["ratio_min"] >= tr.SAFE and np.array_equal(want["rounds"], rounds[[0, 2]])
