"""Batched meshes on the GPU (aq_integrate_mesh_batch, aq_mesh_eval_batch, aq_mesh_invert_batch and their Context
methods) against tests/mesh_batch_reference.py, which shares nothing with the code under test.

The bounds: offsets, x, f and level bit for bit; every cum value within one ulp of the correctly rounded exact prefix
of its own row (the double-double prefix errs by <= accepted_i * 2^-100 of the row's sum, include/aquad.h, so both
values lie among the two doubles that bracket the exact prefix -- derived, not measured); every output bit-identical
between sync_every values and between runs; the query calls bit for bit against the single-mesh calls on the rows'
slices and against their numpy restatements.

The cases are the smallest that reach every boundary of the code: a wave of 64, a scan block of 256 leaves, a level
chunk of 1024 records (mesh_batch_reference.case; their shapes are asserted in tests/test_mesh_batch.py).

Not collected by name: tests/test_gpu_mesh_batch.py runs this file as one child pytest process that imports torch
before the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import ctypes
import os

import numpy as np
import pytest

import mesh_batch_reference as mbr
import param_reference as pr

pytestmark = pytest.mark.gpu

AQ_EINVAL, AQ_EOVERFLOW, AQ_EDEPTH = -1, -4, -5
FRONTIER_CAP = 1 << 14   # records per frontier buffer: above every case's widest level (param: 6 306), which
                         # each run's info.widest_level is compared with
POISON = -7.25
PARITY = ["edges", "param", "param_unit", "param_one", "scale", "sin"]


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _dev(torch, a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


class Raw:
    """aq_integrate_mesh_batch itself on fresh tensors of `alloc` (>= cap_nodes) elements filled with a poison value;
    the arrays whole, on the host. null: names of aq_mesh_batch_io pointers to pass as NULL."""

    def __init__(self, ctx, torch, integrand, a, b, theta, eps, cap_nodes, alloc=None, frontier_cap=FRONTIER_CAP,
                 sync_every=4, max_depth=0, null=(), n=None, with_info=True):
        from ppls_amd import _lib
        n = a.size if n is None else n
        alloc = alloc or cap_nodes
        da, db, dth = _dev(torch, a), _dev(torch, b), _dev(torch, theta)
        x, f, cum = (torch.full((alloc,), POISON, dtype=torch.float64, device="cuda:0") for _ in range(3))
        lev = torch.full((alloc,), 201, dtype=torch.uint8, device="cuda:0")
        off = torch.full((a.size + 1,), -3, dtype=torch.int64, device="cuda:0")
        area = torch.full((a.size,), POISON, dtype=torch.float64, device="cuda:0")
        acc, tasks = (torch.full((a.size,), -3, dtype=torch.int64, device="cuda:0") for _ in range(2))
        status = torch.full((a.size,), -3, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = dict(a=da, b=db, theta=dth, offsets=off, x=x, f=f, cum=cum, level=lev, area=area, accepted=acc,
                    tasks=tasks, status=status)
        io = _lib.aq_mesh_batch_io(*(None if (k in null or t is None) else t.data_ptr() for k, t in ptrs.items()),
                                   int(max_depth), 0)
        self.info = _lib.aq_mesh_batch_info(12345, 12345, 12345, 12345, 123, 123)
        self.rc = ctx.L.aq_integrate_mesh_batch(ctx._h, n, None if "io" in null else ctypes.byref(io), float(eps),
                                                integrand, frontier_cap, sync_every, cap_nodes,
                                                ctypes.byref(self.info) if with_info else None)
        torch.cuda.synchronize()
        self.dev = dict(offsets=off, x=x, f=f, cum=cum)
        self.offsets, self.x, self.f, self.cum, self.level, self.area, self.accepted, self.tasks, self.status = (
            t.cpu().numpy() for t in (off, x, f, cum, lev, area, acc, tasks, status))


def _check_against(run, ref, name=""):
    """One successful run against the reference Batch: everything the header promises."""
    info, m = run.info, ref.n_nodes
    assert run.rc == 0
    assert (info.n_nodes, info.leaves, info.tasks, info.invalid_rows, info.levels, info.widest_level) == (
        m, ref.leaves, ref.tasks_total, ref.invalid_rows, ref.levels, ref.widest_level)
    assert np.array_equal(run.offsets, ref.offsets)
    assert np.array_equal(_bits(run.x[:m]), _bits(ref.x)) and np.array_equal(_bits(run.f[:m]), _bits(ref.f))
    assert np.array_equal(run.level[:m][ref.level_known], ref.level[ref.level_known])
    cum = run.cum[:m]
    ulps = np.abs(cum - ref.cum) / np.spacing(np.abs(ref.cum))
    print(name, "cum: worst deviation in ulp", float(ulps.max()) if m else 0.0, "values off the exact rounding",
          int((cum != ref.cum).sum()), "of", m)
    assert np.all(ulps <= 1.0)
    valid = ref.status == 0
    starts, ends = ref.offsets[:-1][valid], ref.offsets[1:][valid] - 1
    assert np.all(_bits(cum[starts]) == 0)                              # +0.0 at every row's start
    assert np.array_equal(_bits(run.area[valid]), _bits(cum[ends]))     # the row's last cum
    assert np.isnan(run.area[~valid]).all()
    assert np.array_equal(run.accepted, ref.accepted) and np.array_equal(run.tasks, ref.tasks)
    assert np.array_equal(run.status, ref.status)
    for arr in (run.x, run.f, run.cum):                                 # nothing past the mesh
        assert np.all(arr[m:] == POISON)
    assert np.all(run.level[m:] == 201)


def _same_outputs(u, v):
    for k in ("offsets", "x", "f", "cum", "level", "area", "accepted", "tasks", "status"):
        assert np.array_equal(_bits(getattr(u, k)), _bits(getattr(v, k))), k


@pytest.mark.parametrize("name", PARITY)
def test_parity(ctx, torch, name):
    from ppls_amd import Problem
    integrand, a, b, theta, eps, ref = mbr.case(name)
    runs = []
    for sync_every in (1, 4, 4):
        run = Raw(ctx, torch, integrand, a, b, theta, eps, ref.n_nodes, alloc=ref.n_nodes + 64, sync_every=sync_every)
        _check_against(run, ref, "%s sync_every %d" % (name, sync_every))
        runs.append(run)
    for other in runs[1:]:   # sync_every 1 against 4, and 4 again
        _same_outputs(runs[0], other)
    run, valid = runs[0], ref.status == 0
    # the persistent kernel's batch counts the same trees
    if theta is None:
        _, tasks, acc = ctx.integrate_batch(a[valid], b[valid], eps, integrand)
    else:
        _, tasks, acc = ctx.integrate_batch_params(a[valid], b[valid], theta[valid], eps)
    assert np.array_equal(tasks.astype(np.int64), run.tasks[valid]) and np.array_equal(acc.astype(np.int64), run.accepted[valid])
    if theta is None:   # every row is the single-mesh call's mesh
        for i in np.flatnonzero(valid):
            res, x, f, cum, level = ctx.integrate_mesh(Problem(integrand, float(a[i]), float(b[i]), eps),
                                                       cap_nodes=2 * int(ref.accepted[i]) + 1, frontier_cap=FRONTIER_CAP)
            o0, o1 = ref.offsets[i], ref.offsets[i + 1]
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(run.x[o0:o1]))
            assert np.array_equal(_bits(f.cpu().numpy()), _bits(run.f[o0:o1]))
            assert np.array_equal(level.cpu().numpy(), run.level[o0:o1 - 1])
    if name == "scale":   # rows 1 and 2 behind the huge one: no summation is involved, so bit for bit
        for i in (1, 2):
            o = ref.offsets[i]
            x, f = run.x[o:o + 3], run.f[o:o + 3]
            larea, rarea = (f[0] + f[1]) * (x[1] - x[0]) / 2, (f[1] + f[2]) * (x[2] - x[1]) / 2
            assert np.array_equal(_bits(run.cum[o:o + 3]), _bits(np.array([0.0, larea, larea + rarea])))
    if name == "param_one":
        t = pr.tree_reference(pr.TREE_SHIFTED)
        assert (int(run.tasks[0]), int(run.accepted[0]), run.info.levels) == (t["tasks"], t["leaves"], t["levels"])


def test_edges_when_a_workgroup_takes_several_chunks(torch):
    """AQ_LEVEL_GRID=2 (read when the context is created): two workgroups walk every level's chunks."""
    from ppls_amd import Context
    integrand, a, b, theta, eps, ref = mbr.case("edges")
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
        runs = [Raw(c, torch, integrand, a, b, theta, eps, ref.n_nodes, alloc=ref.n_nodes + 64, sync_every=s)
                for s in (1, 4)]
        for run in runs:
            _check_against(run, ref, "edges, grid 2")
        _same_outputs(*runs)


def test_cap_nodes_overflow_reports_the_size(ctx, torch):
    from ppls_amd import AquadError
    integrand, a, b, theta, eps, ref = mbr.case("edges")
    m = ref.n_nodes
    run = Raw(ctx, torch, integrand, a, b, theta, eps, m - 1, alloc=m + 64)
    assert run.rc == AQ_EOVERFLOW and run.info.n_nodes == m and run.info.leaves == ref.leaves
    for arr in (run.x, run.f, run.cum):
        assert np.all(arr[m - 1:] == POISON)
    assert np.all(run.level[m - 1:] == 201)
    retry = Raw(ctx, torch, integrand, a, b, theta, eps, int(run.info.n_nodes), alloc=m + 64)
    _check_against(retry, ref, "retry")
    da, db = _dev(torch, a), _dev(torch, b)
    with pytest.raises(AquadError) as e:
        ctx.integrate_mesh_batch(da, db, eps, cap_nodes=1000, frontier_cap=FRONTIER_CAP)
    assert e.value.code == AQ_EOVERFLOW and e.value.n_nodes == m


def test_frontier_and_depth_errors(ctx, torch):
    integrand, a, b, theta, eps, ref = mbr.case("edges")
    m = ref.n_nodes
    run = Raw(ctx, torch, integrand, a, b, theta, eps, m, frontier_cap=ref.widest_level - 1)
    assert run.rc == AQ_EOVERFLOW and run.info.n_nodes == 0
    run = Raw(ctx, torch, integrand, a, b, theta, eps, m, frontier_cap=ref.widest_level)
    _check_against(run, ref, "frontier_cap == widest level")
    assert Raw(ctx, torch, integrand, a, b, theta, eps, m, frontier_cap=a.size - 1).rc == AQ_EINVAL
    run = Raw(ctx, torch, integrand, a, b, theta, eps, m, max_depth=8)
    assert run.rc == AQ_EDEPTH and run.info.n_nodes == 0
    assert np.array_equal(run.status, ref.depth_status(8))
    assert run.status[300] == mbr.ROW_DEPTH and run.status[304] == mbr.ROW_DEPTH and run.status[305] == 0
    run = Raw(ctx, torch, integrand, a, b, theta, eps, m, max_depth=18)   # [0, 5] has exactly 18 levels
    _check_against(run, ref, "max_depth == the deepest row's levels")


def test_refused_arguments(ctx, torch):
    integrand, a, b, theta, eps, ref = mbr.case("scale")
    m = ref.n_nodes
    ok = dict(integrand=integrand, a=a, b=b, theta=None, eps=eps, cap_nodes=m)
    assert Raw(ctx, torch, **ok).rc == 0
    for name in ("io", "a", "b", "offsets", "x", "f", "cum"):
        assert Raw(ctx, torch, **ok, null=(name,)).rc == AQ_EINVAL, name
    assert Raw(ctx, torch, **ok, with_info=False).rc == AQ_EINVAL
    for name in ("level", "area", "accepted", "tasks", "status"):   # optional outputs
        run = Raw(ctx, torch, **ok, null=(name,))
        assert run.rc == 0 and np.array_equal(_bits(run.cum[:m]), _bits(Raw(ctx, torch, **ok).cum[:m])), name
    th = np.tile([0.0, 1.0], (a.size, 1))
    assert Raw(ctx, torch, **dict(ok, theta=th)).rc == AQ_EINVAL                       # theta with a fixed integrand
    assert Raw(ctx, torch, **dict(ok, integrand=mbr.PARAM)).rc == AQ_EINVAL            # PARAM without theta
    assert Raw(ctx, torch, **dict(ok, integrand=7)).rc == AQ_EINVAL
    assert Raw(ctx, torch, **dict(ok, eps=-1.0)).rc == AQ_EINVAL and Raw(ctx, torch, **dict(ok, eps=np.nan)).rc == AQ_EINVAL
    assert Raw(ctx, torch, **ok, max_depth=-1).rc == AQ_EINVAL and Raw(ctx, torch, **ok, max_depth=128).rc == AQ_EINVAL
    assert Raw(ctx, torch, **ok, sync_every=0).rc == AQ_EINVAL
    assert Raw(ctx, torch, **ok, frontier_cap=1).rc == AQ_EINVAL                       # < max(n, 2)
    assert Raw(ctx, torch, **dict(ok, cap_nodes=2), alloc=16).rc == AQ_EINVAL
    assert Raw(ctx, torch, **dict(ok, cap_nodes=(1 << 31) + 1), alloc=16).rc == AQ_EINVAL
    run = Raw(ctx, torch, **ok, n=0)
    assert run.rc == 0 and np.all(run.x == POISON) and np.all(run.offsets == -3)
    assert (run.info.n_nodes, run.info.leaves, run.info.tasks, run.info.levels, run.info.widest_level) == (0,) * 5
    d = torch.zeros(16, dtype=torch.float64, device="cuda:0").data_ptr()
    for call in (ctx.L.aq_mesh_eval_batch, ctx.L.aq_mesh_invert_batch):
        assert call(ctx._h, 1, d, d, d, d, 1, None, d) == AQ_EINVAL and call(ctx._h, 1, None, d, d, d, 1, d, d) == AQ_EINVAL
        assert call(ctx._h, 0, None, None, None, None, 5, None, None) == 0
        assert call(ctx._h, 5, None, None, None, None, 0, None, None) == 0


def test_all_rows_invalid(ctx, torch):
    a, b = np.array([2.0, 0.0, np.nan]), np.array([1.0, 171.0, 1.0])
    run = Raw(ctx, torch, mbr.COSH4, a, b, None, 1e-3, 16)
    assert run.rc == 0 and run.info.n_nodes == 0 and run.info.invalid_rows == 3
    assert np.all(run.offsets == 0) and np.all(run.status == mbr.ROW_INVALID) and np.isnan(run.area).all()
    assert np.all(run.accepted == 0) and np.all(run.tasks == 0) and np.all(run.x == POISON)


def test_device_memory_moves_with_the_first_batch_mesh_call_only(torch):
    from ppls_amd import Context, Problem
    integrand, a, b, theta, eps, ref = mbr.case("scale")
    with Context(0) as c:
        c.integrate(Problem(mbr.COSH4, 0.0, 5.0, 1e-3))
        before = c.device_bytes
        assert Raw(c, torch, integrand, a, b, theta, eps, ref.n_nodes, null=("x",)).rc == AQ_EINVAL
        assert c.device_bytes == before
        assert Raw(c, torch, integrand, a, b, theta, eps, ref.n_nodes).rc == 0
        after = c.device_bytes
        assert after > before
        assert Raw(c, torch, integrand, a, b, theta, eps, ref.n_nodes).rc == 0
        assert c.device_bytes == after


def _query_sets(ref):
    q = np.stack([mbr.queries(r.x) if r is not None else np.linspace(0.0, 1.0, 257) for r in ref.rows])
    return q, mbr.mesh_eval_batch(ref.offsets, ref.x, ref.f, ref.cum, q)


def _same(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (int(np.isnan(got).sum()), int(nan.sum()))
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan])), int((_bits(got[~nan]) != _bits(want[~nan])).sum())


@pytest.mark.parametrize("name", ["edges", "param"])
def test_queries(ctx, torch, name):
    """257 queries a row -- nodes, midpoints, both ends, two points outside and a NaN; the matching cum values for the
    inversion -- on the library's own mesh: row by row what the single-mesh calls give on the row's slice, and the
    numpy restatements."""
    integrand, a, b, theta, eps, ref = mbr.case(name)
    run = Raw(ctx, torch, integrand, a, b, theta, eps, ref.n_nodes)
    assert run.rc == 0
    q, _ = _query_sets(ref)
    n, nq, m = q.shape[0], q.shape[1], ref.n_nodes
    off, x, f, cum = (run.dev[k] for k in ("offsets", "x", "f", "cum"))
    hx, hf, hcum = run.x[:m], run.f[:m], run.cum[:m]
    dq = _dev(torch, q)

    def batch(call, din):
        out = torch.full((n, nq), POISON, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        assert call(ctx._h, n, off.data_ptr(), x.data_ptr(), f.data_ptr(), cum.data_ptr(), nq, din.data_ptr(),
                    out.data_ptr()) == 0
        ctx.synchronize()
        return out

    def single(method, din):
        out = np.full((n, nq), np.nan)
        for i in range(n):
            o0, o1 = int(ref.offsets[i]), int(ref.offsets[i + 1])
            if o1 - o0 >= 3:
                out[i] = method(x[o0:o1].clone(), f[o0:o1].clone(), cum[o0:o1].clone(), din[i].clone()).cpu().numpy()
        return out

    ev = batch(ctx.L.aq_mesh_eval_batch, dq)
    hev = ev.cpu().numpy()
    _same(hev, single(ctx.mesh_eval, dq))
    _same(hev, mbr.mesh_eval_batch(ref.offsets, hx, hf, hcum, q))
    empty = ref.status != 0
    assert np.isnan(hev[empty]).all() and empty.sum() == ref.invalid_rows
    inv = batch(ctx.L.aq_mesh_invert_batch, ev).cpu().numpy()
    _same(inv, single(ctx.mesh_invert, ev))
    _same(inv, mbr.mesh_invert_batch(ref.offsets, hx, hf, hcum, hev))
    assert np.isnan(inv[empty]).all()


def test_queries_on_a_non_monotone_batch(ctx, torch):
    integrand, a, b, theta, eps, ref = mbr.case("sin")
    mesh = ctx.integrate_mesh_batch(_dev(torch, a), _dev(torch, b), eps, integrand=integrand, frontier_cap=FRONTIER_CAP)
    q, y = _query_sets(ref)
    out = ctx.mesh_invert_batch(mesh, _dev(torch, y)).cpu().numpy()
    for i, r in enumerate(ref.rows):
        ok = ~np.isnan(out[i])
        assert np.all((out[i][ok] >= r.x[0]) & (out[i][ok] <= r.x[-1]))
    ev = ctx.mesh_eval_batch(mesh, _dev(torch, q)).cpu().numpy()
    _same(ev, y)


def test_python_surface_and_quantiles(ctx, torch):
    """integrate_mesh_batch with its default sizing, row(i), and the medians of Gaussian rows symmetric about mu."""
    from ppls_amd import PARAM
    rng = np.random.default_rng(5)
    n = 100
    mu, s = rng.uniform(-2.0, 2.0, n), np.exp(rng.uniform(-1.0, 1.0, n))
    half = rng.uniform(0.5, 4.0, n) / s
    a, b, theta = mu - half, mu + half, np.ascontiguousarray(np.stack([mu, s], axis=1))
    mesh = ctx.integrate_mesh_batch(_dev(torch, a), _dev(torch, b), 1e-6, integrand=PARAM, theta=_dev(torch, theta),
                                    frontier_cap=FRONTIER_CAP)
    ref = mbr.Batch(mbr.param_rows(a, b, theta, 1e-6))
    assert len(mesh) == n and mesh.n_nodes == ref.n_nodes == mesh.x.shape[0] and mesh.widest_level == ref.widest_level
    assert np.array_equal(mesh.offsets.cpu().numpy(), ref.offsets)
    assert np.array_equal(_bits(mesh.x.cpu().numpy()), _bits(ref.x))
    x7, f7, cum7, lev7 = mesh.row(7)
    assert np.array_equal(_bits(x7.cpu().numpy()), _bits(ref.rows[7].x)) and lev7.shape[0] == x7.shape[0] - 1
    assert np.array_equal(lev7.cpu().numpy(), ref.rows[7].level)
    med = ctx.mesh_quantiles(mesh, [0.5]).cpu().numpy()[:, 0]
    widest = np.array([np.diff(r.x).max() for r in ref.rows])
    print("medians: worst |out - mu| / widest panel", float((np.abs(med - mu) / widest).max()))
    assert np.all(np.abs(med - mu) <= widest)
    u = np.tile([0.25, 0.5, 0.75], (n, 1))
    qs = ctx.mesh_quantiles(mesh, u).cpu().numpy()
    assert qs.shape == (n, 3) and np.all(np.diff(qs, axis=1) > 0) and np.array_equal(_bits(qs[:, 1]), _bits(med))
    with pytest.raises(ValueError):
        ctx.integrate_mesh_batch(_dev(torch, a), _dev(torch, b), 1e-6, integrand=PARAM)   # PARAM without theta
    with pytest.raises(ValueError):
        ctx.mesh_eval_batch(mesh, torch.zeros(n + 1, 3, dtype=torch.float64, device="cuda:0"))
