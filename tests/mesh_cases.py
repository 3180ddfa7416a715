"""The accepted mesh on the GPU (Context.integrate_mesh / aq_integrate_mesh, Context.mesh_eval / aq_mesh_eval): leaf
for leaf against tests/mesh_reference.py, which shares nothing with the code under test.

The bounds: x, f and level bit for bit; every cum value within one ulp of the correctly rounded exact prefix (the
double-double prefix errs by <= accepted * 2^-100 of the sum, include/aquad.h -- derived, not measured); the outputs
bit-identical between sync_every values and between runs; aq_mesh_eval bit for bit against its numpy restatement.

Not collected by name: tests/test_gpu_mesh.py runs this file as one child pytest process that imports torch before
the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import ctypes

import numpy as np
import pytest

import mesh_reference as mr

pytestmark = pytest.mark.gpu

AQ_EINVAL, AQ_EOVERFLOW, AQ_EDEPTH = -1, -4, -5
FRONTIER_CAP = 1 << 16   # records per frontier buffer: the widest level of the cases holds 17 042


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
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _raw(ctx, torch, problem, cap_nodes, alloc=None, level=True, frontier_cap=FRONTIER_CAP, sync_every=4):
    """aq_integrate_mesh itself on fresh tensors of `alloc` (>= cap_nodes) elements filled with a poison value:
    (rc, result, n_nodes, x, f, cum, level) -- the arrays whole, on the host."""
    from ppls_amd import _lib
    alloc = alloc or cap_nodes
    x, f, cum = (torch.full((alloc,), -7.25, dtype=torch.float64, device="cuda:0") for _ in range(3))
    lev = torch.full((alloc,), 201, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    io = _lib.aq_mesh_io(x.data_ptr(), f.data_ptr(), cum.data_ptr(), lev.data_ptr() if level else None)
    r = _lib.aq_result()
    n = ctypes.c_uint64(12345)
    rc = ctx.L.aq_integrate_mesh(ctx._h, ctypes.byref(problem.c()), frontier_cap, sync_every, cap_nodes,
                                 ctypes.byref(io), ctypes.byref(r), ctypes.byref(n))
    return rc, r, int(n.value), x.cpu().numpy(), f.cpu().numpy(), cum.cpu().numpy(), lev.cpu().numpy()


@pytest.mark.parametrize("name,integrand,a,b,eps", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_mesh_parity(ctx, torch, oracle, name, integrand, a, b, eps):
    from ppls_amd import Problem
    want = oracle.integrate(integrand, a, b, eps)
    m = mr.reference_mesh(integrand, a, b, eps)
    runs = []
    for sync_every in (1, 4, 4):
        res, x, f, cum, level = ctx.integrate_mesh(Problem(integrand, a, b, eps), cap_nodes=2 * m.accepted + 1,
                                                   frontier_cap=FRONTIER_CAP, sync_every=sync_every)
        assert x.is_cuda and x.dtype == torch.float64 and level.dtype == torch.uint8
        x, f, cum, level = (t.cpu().numpy() for t in (x, f, cum, level))
        runs.append((x, f, cum, level))
        assert x.size == f.size == cum.size == 2 * res.accepted + 1 and level.size == 2 * res.accepted
        assert (res.tasks, res.accepted, res.levels) == (want.tasks, want.leaves, want.levels)
        assert np.array_equal(_bits(x), _bits(m.x))
        assert np.array_equal(_bits(f), _bits(m.f))
        assert np.array_equal(level, m.level)
        ulps = np.abs(cum - m.cum) / np.spacing(np.abs(m.cum))
        print(name, "sync_every", sync_every, "cum: worst deviation in ulp", float(ulps.max()),
              "values off the exact rounding", int((cum != m.cum).sum()), "of", cum.size)
        assert cum[0] == 0.0 and np.all(ulps <= 1.0)
        assert abs(cum[-1] - res.area) <= np.spacing(abs(res.area)), (float(cum[-1]).hex(), float(res.area).hex())
    for other in runs[1:]:   # sync_every 1 against 4, and 4 again
        for u, v in zip(runs[0], other):
            assert np.array_equal(_bits(u), _bits(v))


def test_cap_nodes_overflow_reports_the_size(ctx, torch):
    """cosh^4 on [0, 5] at 1e-3: 3 284 leaves, 6 569 nodes. A capacity of 1 000 is told the size and nothing is
    written past it; the same context then succeeds with the size it was told."""
    from ppls_amd import AquadError, Problem
    p = Problem(mr.COSH4, 0.0, 5.0, 1e-3)
    m = mr.reference_mesh(mr.COSH4, 0.0, 5.0, 1e-3)
    assert m.accepted == 3284
    rc, r, n, x, f, cum, lev = _raw(ctx, torch, p, 1000, alloc=4096)
    assert rc == AQ_EOVERFLOW and n == 6569 and (r.accepted, r.tasks) == (3284, m.tasks)
    for arr, poison in ((x, -7.25), (f, -7.25), (cum, -7.25)):
        assert np.all(arr[1000:] == poison)
    assert np.all(lev[999:] == 201)
    with pytest.raises(AquadError) as e:
        ctx.integrate_mesh(p, cap_nodes=1000, frontier_cap=FRONTIER_CAP)
    assert e.value.code == AQ_EOVERFLOW and e.value.n_nodes == 6569
    rc, r, n, x, f, cum, lev = _raw(ctx, torch, p, 6569, alloc=8192)
    assert rc == 0 and n == 6569
    assert np.array_equal(_bits(x[:n]), _bits(m.x)) and np.array_equal(_bits(f[:n]), _bits(m.f))
    assert np.array_equal(lev[:n - 1], m.level)
    assert np.all(np.abs(cum[:n] - m.cum) <= np.spacing(np.abs(m.cum)))
    for arr in (x, f, cum):
        assert np.all(arr[n:] == -7.25)
    assert np.all(lev[n - 1:] == 201)
    # level == NULL: the other three arrays all the same
    rc, r, n, x2, f2, cum2, lev2 = _raw(ctx, torch, p, 6569, level=False)
    assert rc == 0 and np.all(lev2 == 201)
    assert all(np.array_equal(_bits(u[:n]), _bits(v[:n])) for u, v in ((x, x2), (f, f2), (cum, cum2)))
    # the default sizing (a first integrate call) arrives at the same mesh
    res, tx, tf, tcum, tlev = ctx.integrate_mesh(p, frontier_cap=FRONTIER_CAP)
    assert tx.shape[0] == 6569 and np.array_equal(_bits(tcum.cpu().numpy()), _bits(cum[:n]))


def test_depth_and_frontier_errors_leave_no_mesh(ctx, torch):
    from ppls_amd import Problem
    rc, r, n, *_ = _raw(ctx, torch, Problem(mr.COSH4, 0.0, 5.0, 1e-3, max_depth=8), 6569)
    assert rc == AQ_EDEPTH and n == 0
    rc, r, n, *_ = _raw(ctx, torch, Problem(mr.COSH4, 0.0, 5.0, 1e-3), 6569, frontier_cap=64)   # widest level: 1 642
    assert rc == AQ_EOVERFLOW and n == 0


def test_refused_arguments(ctx, torch):
    from ppls_amd import Problem, _lib
    p = Problem(mr.COSH4, 0.0, 5.0, 1e-3)
    rc, r, n, *_ = _raw(ctx, torch, Problem(3, 0.0, 5.0, 1e-3), 6569)   # AQ_F_PARAM: the frontier engine takes no theta
    assert rc == AQ_EINVAL
    t = torch.zeros(16, dtype=torch.float64, device="cuda:0")
    res, n = _lib.aq_result(), ctypes.c_uint64(0)
    ok = _lib.aq_mesh_io(t.data_ptr(), t.data_ptr(), t.data_ptr(), None)

    def call(prob=p, fcap=FRONTIER_CAP, sync=4, cap=16, io=ok, nn=n):
        return ctx.L.aq_integrate_mesh(ctx._h, ctypes.byref(prob.c()) if prob else None, fcap, sync, cap,
                                       ctypes.byref(io) if io else None, ctypes.byref(res),
                                       ctypes.byref(nn) if nn is not None else None)

    assert call(prob=None) == AQ_EINVAL and call(io=None) == AQ_EINVAL and call(nn=None) == AQ_EINVAL
    for k in range(3):
        ptrs = [t.data_ptr()] * 3
        ptrs[k] = None
        assert call(io=_lib.aq_mesh_io(*ptrs, None)) == AQ_EINVAL
    assert call(cap=2) == AQ_EINVAL and call(cap=(1 << 31) + 1) == AQ_EINVAL
    assert call(fcap=1) == AQ_EINVAL and call(sync=0) == AQ_EINVAL
    assert call(prob=Problem(mr.COSH4, 0.0, 5.0, -1.0)) == AQ_EINVAL
    d = t.data_ptr()
    assert ctx.L.aq_mesh_eval(ctx._h, 2, d, d, d, 1, d, d) == AQ_EINVAL
    assert ctx.L.aq_mesh_eval(ctx._h, 3, d, d, d, 1, None, d) == AQ_EINVAL
    assert ctx.L.aq_mesh_eval(ctx._h, 3, None, d, d, 1, d, d) == AQ_EINVAL
    assert ctx.L.aq_mesh_eval(ctx._h, 3, None, None, None, 0, None, None) == 0
    with pytest.raises(ValueError):
        ctx.mesh_eval(t, t, t, t.cpu())


def test_mesh_eval_matches_its_restatement(ctx, torch):
    """4 096 queries on the eps = 1e-6 mesh: every node of the first 1 000 panels, their midpoints, a, b, random
    points, two points outside and a NaN -- bit for bit the numpy restatement, NaN exactly where stated."""
    from ppls_amd import Problem
    _, integrand, a, b, eps = mr.CASES[0]
    res, x, f, cum, level = ctx.integrate_mesh(Problem(integrand, a, b, eps), frontier_cap=FRONTIER_CAP)
    hx, hf, hcum = (t.cpu().numpy() for t in (x, f, cum))
    rng = np.random.default_rng(20260)
    fixed = np.concatenate([hx[:1001], 0.5 * (hx[:1000] + hx[1:1001]), [a, b, a - 1e-6, np.nextafter(b, np.inf), np.nan]])
    q = np.concatenate([fixed, rng.uniform(a, b, 4096 - fixed.size)])
    assert q.size == 4096
    got = ctx.mesh_eval(x, f, cum, torch.as_tensor(q).to("cuda:0")).cpu().numpy()
    want = mr.mesh_eval(hx, hf, hcum, q)
    nan = np.zeros(4096, bool)
    nan[2003:2006] = True   # the two points outside and the NaN
    assert np.array_equal(np.isnan(want), nan) and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan]))
    assert np.array_equal(_bits(got[:1001]), _bits(hcum[:1001]))   # at a node: cum there
    # a 2-d q keeps its shape
    q2 = torch.as_tensor(q[:2000].reshape(40, 50)).to("cuda:0")
    assert np.array_equal(_bits(ctx.mesh_eval(x, f, cum, q2).cpu().numpy().ravel()), _bits(want[:2000]))


def test_device_memory_moves_with_the_first_mesh_call_only(torch):
    """A fresh context: integrate, a frontier run and refused mesh calls leave aq_ctx_device_bytes where the frontier
    run put it; the first mesh call adds the leaf records, the sort's arrays and the scan partials, a second none."""
    from ppls_amd import Context, Problem, _lib
    from ppls_amd.frontier import HipStepper
    p = Problem(mr.COSH4, 0.0, 5.0, 1e-3)
    with Context(0) as c:
        c.integrate(p)
        HipStepper(c).integrate_one_gpu(p, FRONTIER_CAP)
        before = c.device_bytes
        n = ctypes.c_uint64(0)
        assert c.L.aq_integrate_mesh(c._h, ctypes.byref(p.c()), FRONTIER_CAP, 4, 6569, None, None,
                                     ctypes.byref(n)) == AQ_EINVAL
        assert c.device_bytes == before
        c.integrate_mesh(p, cap_nodes=6569, frontier_cap=FRONTIER_CAP)
        after = c.device_bytes
        # 48 bytes a leaf record of the capacity, 24 a sorted leaf (two keys, two indices), scratch and partials
        assert 48 * 3284 <= after - before <= 48 * 3284 + 24 * 3284 + (1 << 20), (before, after)
        c.integrate_mesh(p, cap_nodes=6569, frontier_cap=FRONTIER_CAP)
        assert c.device_bytes == after
