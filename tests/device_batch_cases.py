"""The device-resident batch on the GPU (Context.integrate_batch_device / aq_integrate_batch_device): torch CUDA
tensors in and out, ordered on torch's current stream, against references that share nothing with the code under
test -- tests/err_reference.walk (the numpy / oracle walker, any integrand), tests/param_reference's draw, and the
golden trees.

The bounds are the project's: counts exact; an area within 1 ulp of the walker's math.fsum of the leaf areas (the
bound of test_gpu_params.py); either error sum within leaves * 2^-52 * err_abs of the walker's exact sums (the bound
include/aquad.h states and test_gpu_err.py uses, err_reference.tol).

Not collected by name: tests/test_gpu_device_batch.py runs this file as one child pytest process that imports torch
before the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import ctypes
import math
import time

import numpy as np
import pytest

import err_reference as er
import param_reference as pr

pytestmark = pytest.mark.gpu

COSH4, SIN_RECIP, USER, PARAM = 0, 1, 2, 3
AQ_EINVAL, AQ_EDEPTH = -1, -5
ROW_DEPTH, ROW_INVALID = 4, 8
NPAR = 350   # the parity tests' cosh^4 rows (the oracle's batch bounds, eps = 1e-6)


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


def _dev(torch, x, dtype=None):
    return torch.as_tensor(np.array(x), dtype=dtype or torch.float64).to("cuda:0").contiguous()   # (np.array: a writable copy)


def _host(out):
    """A DeviceBatch as numpy arrays (None stays None); the copies wait for the current stream."""
    return type(out)(*(None if t is None else t.cpu().numpy() for t in out))


def _check(out, w, sel, what, err=False, skip=()):
    """Rows of a DeviceBatch (numpy) against walk w's rows `sel`, but for the rows in `skip`: counts exact, area
    within 1 ulp, both sums within tol, status 0."""
    keep = np.ones(len(out.area), bool)
    keep[list(skip)] = False
    tasks, leaves, want = w["tasks"][sel][keep], w["leaves"][sel][keep], w["area"][sel][keep]
    bad = np.nonzero((out.tasks[keep] != tasks) | (out.accepted[keep] != leaves))[0]
    assert bad.size == 0, (what, [(int(i), int(out.tasks[keep][i]), int(tasks[i])) for i in bad[:8]], bad.size)
    off = np.nonzero(~(np.abs(out.area[keep] - want) <= np.spacing(np.abs(want))))[0]
    assert off.size == 0, (what, [(int(i), float(out.area[keep][i]).hex(), float(want[i]).hex()) for i in off[:8]], off.size)
    assert not out.status[keep].any(), (what, out.status[keep].nonzero())
    if not err:
        assert out.err_abs is None and out.err_signed is None
        return
    t = w["leaves"][sel][keep] * 2.0 ** -52 * w["err_abs"][sel][keep]
    for name, got in (("err_abs", out.err_abs), ("err_signed", out.err_signed)):
        dev = np.abs(got[keep] - w[name][sel][keep])
        print(what, name, "worst deviation / tol", float(np.max(dev / np.maximum(t, 5e-324))))
        off = np.nonzero(~(dev <= t))[0]
        assert off.size == 0, (what, name, [(int(i), float(got[keep][i]), float(t[i])) for i in off[:8]], off.size)


# ---- 1. parity at the shapes where it can go wrong ------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 11, 12, 63, 64, 255, 256, 257])
def test_parity_one_chunk(ctx, torch, n):
    """The per-CU threshold (11 / 12: never taken -- the bounds are not on the host), the sort threshold (63 / 64)
    and the check kernel's block edge (255 / 256 / 257)."""
    a, b, w = er.batch_reference(NPAR, 1e-6)
    out = _host(ctx.integrate_batch_device(_dev(torch, a[:n]), _dev(torch, b[:n]), 1e-6))
    _check(out, w, slice(0, n), n)
    assert ctx.device_batch_check() == 0


@pytest.mark.parametrize("n,sort", [(350, "1"), (305, "1"), (305, "0")])
def test_parity_chunks(ctx, torch, monkeypatch, n, sort):
    """Chunks of 100: four of them with a tail of 50, and a tail of 5 -- the high-slot launch -- behind full
    chunks, every ring used at both parities; in size order and in input order."""
    monkeypatch.setenv("AQ_DEVBATCH_CHUNK", "100")
    monkeypatch.setenv("AQ_BATCH_SORT", sort)
    a, b, w = er.batch_reference(NPAR, 1e-6)
    out = _host(ctx.integrate_batch_device(_dev(torch, a[:n]), _dev(torch, b[:n]), 1e-6))
    _check(out, w, slice(0, n), (n, sort))
    assert ctx.device_batch_check() == 0


# ---- 2. every family, with the error estimate -----------------------------------------------------------------
def _sin_rows():
    """200 intervals inside [1e-4, 1] between consecutive zeros 1 / (k pi) of sin(1/x), k = 1, 16, 31 .. 2986 (7 to
    about 1100 tasks each at eps = 1e-9). Between two zeros the integrand keeps its sign, so the leaf areas of a tree
    share one: the device's area is an exact sum of double partial sums, whose rounding errors are relative to the
    sum of the |leaf areas| -- only where that equals |area| can the 1-ulp bound of the positive integrands be asked
    of it (rows that straddle zeros: max(1e-12 |area|, ulp), test_gpu_matrix.py's bound for launches of this kind)."""
    k = 1.0 + 15.0 * np.arange(200)
    return 1.0 / ((k + 1.0) * np.pi), 1.0 / (k * np.pi)


def _user_rows():
    a = np.linspace(-3.0, 2.5, 200)
    return a, a + np.linspace(0.05, 4.0, 200)


@pytest.fixture(scope="module")
def family_refs(oracle):
    sa, sb = _sin_rows()
    ua, ub = _user_rows()
    return {SIN_RECIP: (sa, sb, 1e-9, er.walk(sa, sb, 1e-9, SIN_RECIP, oracle)),
            USER: (ua, ub, 1e-9, er.walk(ua, ub, 1e-9, USER, oracle))}


@pytest.mark.parametrize("f", [SIN_RECIP, USER])
def test_fixed_families_err(ctx, torch, family_refs, f):
    a, b, eps, w = family_refs[f]
    assert a.size == 200 and w["tasks"].max() > 50 and (f != SIN_RECIP or (a.min() >= 1e-4 and b.max() <= 1.0))
    out = _host(ctx.integrate_batch_device(_dev(torch, a), _dev(torch, b), eps, integrand=f, err=True))
    _check(out, w, slice(0, 200), f, err=True)
    assert ctx.device_batch_check() == 0


@pytest.mark.parametrize("chunk", [None, "300", "333"])
def test_param_family_err(ctx, torch, monkeypatch, chunk):
    """The first 1000 rows of the draw; in chunks of 300 the theta rows travel with sorted chunks across parities;
    in chunks of 333 the last row is a chunk of its own: the ERR launch of few integrals into high slots."""
    if chunk:
        monkeypatch.setenv("AQ_DEVBATCH_CHUNK", chunk)
    n = 1000
    a, b, theta, w = er.draw_reference()
    out = _host(ctx.integrate_batch_device(_dev(torch, a[:n]), _dev(torch, b[:n]), pr.DRAW_EPS, integrand=PARAM,
                                           theta=_dev(torch, theta[:n]), err=True))
    _check(out, w, slice(0, n), ("param", chunk), err=True)
    assert ctx.device_batch_check() == 0


# ---- 3. invalid rows are contained ------------------------------------------------------------------------------
def _invalid(out, rows):
    rows = list(rows)
    assert (out.status[rows] == ROW_INVALID).all(), out.status[rows]
    assert np.isnan(out.area[rows]).all() and not out.tasks[rows].any() and not out.accepted[rows].any()
    if out.err_abs is not None:
        assert np.isnan(out.err_abs[rows]).all() and np.isnan(out.err_signed[rows]).all()


def test_invalid_rows_are_contained(ctx, torch):
    from ppls_amd import AquadError
    n = 300
    a, b, w = er.batch_reference(NPAR, 1e-6)
    a, b = a[:n].copy(), b[:n].copy()
    a[0] = np.nan
    b[63] = np.inf
    a[64], b[64] = b[64], a[64]
    assert b[64] < a[64]
    a[150], b[150] = -171.0, 1.0
    a[299] = 1e-300
    planted = [0, 63, 64, 150, 299]
    da, db = _dev(torch, a), _dev(torch, b)
    out = _host(ctx.integrate_batch_device(da, db, 1e-6))
    _invalid(out, planted)
    _check(out, w, slice(0, n), "cosh4 with invalid rows", skip=planted)
    assert ctx.device_batch_check(raise_on_error=False) == len(planted)
    assert ctx.device_batch_check(raise_on_error=False) == 0
    ctx.integrate_batch_device(da, db, 1e-6)
    with pytest.raises(AquadError) as e:
        ctx.device_batch_check()
    assert e.value.code == AQ_EINVAL
    assert ctx.device_batch_check() == 0
    # the parametrised family: a zero inverse scale, a NaN in theta
    m = 200
    pa, pb, theta, pw = er.draw_reference()
    theta = theta[:m].copy()
    theta[17, 1] = 0.0
    theta[130, 0] = np.nan
    out = _host(ctx.integrate_batch_device(_dev(torch, pa[:m]), _dev(torch, pb[:m]), pr.DRAW_EPS, integrand=PARAM,
                                           theta=_dev(torch, theta), err=True))
    _invalid(out, [17, 130])
    _check(out, pw, slice(0, m), "param with invalid rows", err=True, skip=[17, 130])
    assert ctx.device_batch_check(raise_on_error=False) == 2


# ---- 4. error bits reach the row --------------------------------------------------------------------------------
def test_error_bits_reach_the_row(ctx, torch, trees):
    from ppls_amd import AquadError, Problem
    a = np.zeros(20)
    b = np.full(20, 5.0)
    b[7] = 0.0   # the empty interval: one task, accepted at the root
    out = _host(ctx.integrate_batch_device(_dev(torch, a), _dev(torch, b), 1e-10, max_depth=5))
    rest = [i for i in range(20) if i != 7]
    assert (out.status[rest] == ROW_DEPTH).all() and out.status[7] == 0, out.status
    assert (out.tasks[7], out.accepted[7], out.area[7]) == (1, 1, 0.0)
    with pytest.raises(AquadError) as e:
        ctx.device_batch_check()
    assert e.value.code == AQ_EDEPTH
    assert ctx.device_batch_check() == 0
    g = trees["cosh4_eps1e-3"]
    r = ctx.integrate(Problem(eps=1e-3))
    assert (r.tasks, r.accepted, r.tasks_per_level) == (g["tasks"], g["leaves"], g["tasks_per_level"])
    assert "%f" % r.area == g["reference"]["area_printed"]


# ---- 5. stream order, no synchronisation by the caller ----------------------------------------------------------
def test_stream_order(ctx, torch):
    """Inputs made by torch kernels on a side stream, the call, and torch reductions of its outputs on the same
    stream with nothing in between; two calls back to back, one synchronize. Then the inputs freed right after the
    call and their memory overwritten on the stream."""
    n = 256
    host = [(np.zeros(n), 1.0 + 0.015625 * np.arange(n)), (-(0.5 + 0.0078125 * np.arange(n)), 0.25 + 0.0078125 * np.arange(n))]
    refs = [er.walk(a, b, 1e-6, COSH4, er_oracle()) for a, b in host]
    s = torch.cuda.Stream(device="cuda:0")
    i = torch.arange(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ins = [(torch.zeros(n, dtype=torch.float64, device="cuda:0"), 1.0 + 0.015625 * i),
               (-(0.5 + 0.0078125 * i), 0.25 + 0.0078125 * i)]
        got = []
        for a, b in ins:
            out = ctx.integrate_batch_device(a, b, 1e-6)
            got.append((out, out.tasks.sum(), out.accepted.sum(), out.area.sum()))
        s.synchronize()
    for (a, b), (ha, hb) in zip(ins, host):
        assert np.array_equal(a.cpu().numpy(), ha) and np.array_equal(b.cpu().numpy(), hb)
    for (out, tasks, leaves, area), w in zip(got, refs):
        _check(_host(out), w, slice(0, n), "stream")
        assert (int(tasks), int(leaves)) == (int(w["tasks"].sum()), int(w["leaves"].sum()))
        # each area within 1 ulp, and torch's own f64 sum of n terms: (n - 1) * 2^-53 * sum|x| to first order, doubled
        bound = float(np.spacing(w["area"]).sum()) + n * 2.0 ** -52 * float(np.abs(w["area"]).sum())
        assert abs(float(area) - math.fsum(w["area"])) <= bound
    # free the inputs between the call and the use: the caller's stream waits for the call's last read of them
    with torch.cuda.stream(s):
        a, b = 1.0 * ins[0][0], 1.0 * ins[0][1]
        out = ctx.integrate_batch_device(a, b, 1e-6)
        del a, b
        junk = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0") for _ in range(8)]
        total = out.tasks.sum()
        s.synchronize()
    assert int(total) == int(refs[0]["tasks"].sum()) and len(junk) == 8
    _check(_host(out), refs[0], slice(0, n), "inputs freed")
    assert ctx.device_batch_check() == 0


def er_oracle():
    from oracle import pyoracle
    return pyoracle


# ---- 6. the call does not wait for the device -------------------------------------------------------------------
def test_call_only_enqueues(ctx, torch, trees):
    """4096 cosh^4 [0, 5] integrals at eps = 1e-10 are about 10 ms of kernel; the call returns while they run: an
    event recorded on the caller's stream right behind it has not happened yet. (Meaningful while the device time
    is at least 10x the call's host time -- asserted, so that a faster device fails here, not silently.)"""
    n = 4096
    g = trees["cosh4_eps1e-10"]
    w = er.lone(COSH4, 0.0, 5.0, 1e-10)
    a = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    b = torch.full((n,), 5.0, dtype=torch.float64, device="cuda:0")
    ctx.integrate_batch_device(a[:64], b[:64], 1e-10)   # warm-up: rings, events, the instances' first launch
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    t0 = time.perf_counter()
    out = ctx.integrate_batch_device(a, b, 1e-10)
    host_ms = (time.perf_counter() - t0) * 1e3
    ev1.record()
    pending = not ev1.query()
    torch.cuda.synchronize()
    dev_ms = ev0.elapsed_time(ev1)
    print("host ms", host_ms, "device ms", dev_ms)
    assert pending
    assert dev_ms >= 10.0 * host_ms, (dev_ms, host_ms)
    out = _host(out)
    assert (out.tasks == g["tasks"]).all() and (out.accepted == g["leaves"]).all() and not out.status.any()
    assert (np.abs(out.area - w["area"]) <= math.ulp(w["area"])).all()
    assert ctx.device_batch_check() == 0


# ---- 7. coexistence ---------------------------------------------------------------------------------------------
def test_coexistence(torch, trees):
    from ppls_amd import Context, Problem
    n = 300
    a, b, w = er.batch_reference(NPAR, 1e-6)
    pa, pb, theta, pw = er.draw_reference()
    g = trees["cosh4_eps1e-3"]
    with Context(0) as c:
        fresh = c.device_bytes
        c.integrate(Problem(eps=1e-3))
        c.integrate_batch(a[:n], b[:n], 1e-6)
        assert c.device_bytes > fresh   # (the host batch's rings)
        before = c.device_bytes
        assert c.device_batch_check() == 0 and c.device_bytes == before
        c.cu_task_counters(reset=True)
        da, db = _dev(torch, a[:n]), _dev(torch, b[:n])
        first = c.integrate_batch_device(da, db, 1e-6, err=True)
        assert c.device_bytes > before
        held = c.device_bytes
        area, tasks, acc, ea, es = c.integrate_batch_err(pa[:n], pb[:n], pr.DRAW_EPS, integrand=PARAM, theta=theta[:n])
        r = c.integrate(Problem(eps=1e-3))
        second = c.integrate_batch_device(da, db, 1e-6)
        _check(_host(first), w, slice(0, n), "first device batch", err=True)
        _check(_host(second), w, slice(0, n), "second device batch")
        assert c.device_bytes >= held   # (the host PARAM call's theta rings may have come on top; the device batch's stay)
        assert np.array_equal(tasks.astype(np.int64), pw["tasks"][:n]) and np.array_equal(acc.astype(np.int64), pw["leaves"][:n])
        assert (np.abs(area - pw["area"][:n]) <= np.spacing(np.abs(pw["area"][:n]))).all()
        t = pw["leaves"][:n] * 2.0 ** -52 * pw["err_abs"][:n]
        assert (np.abs(ea - pw["err_abs"][:n]) <= t).all() and (np.abs(es - pw["err_signed"][:n]) <= t).all()
        assert (r.tasks, r.accepted, r.tasks_per_level) == (g["tasks"], g["leaves"], g["tasks_per_level"])
        assert c.device_batch_check() == 0
        total = 2 * int(w["tasks"][:n].sum()) + int(pw["tasks"][:n].sum()) + g["tasks"]
        assert sum(c.cu_task_counters().values()) == total
        # a third call allocates nothing
        third = c.integrate_batch_device(da, db, 1e-6, err=True)
        c.synchronize()
        assert c.device_bytes >= held and third.area.shape == (n,)


# ---- the arguments the host checks, and the Python front's ------------------------------------------------------
def test_host_checked_arguments(ctx, torch):
    from ppls_amd import _lib
    L = ctx.L
    a = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    b = torch.ones(4, dtype=torch.float64, device="cuda:0")
    th = torch.ones((4, 2), dtype=torch.float64, device="cuda:0")

    def call(n=4, a_=a.data_ptr(), b_=b.data_ptr(), theta=None, eps=1e-3, f=COSH4, max_depth=0, io=True):
        s = _lib.aq_device_io(a=a_, b=b_, theta=theta, max_depth=max_depth)
        return L.aq_integrate_batch_device(ctx._h, n, ctypes.byref(s) if io else None, eps, f, None)

    assert call(io=False) == AQ_EINVAL
    assert call(a_=None) == AQ_EINVAL and call(b_=None) == AQ_EINVAL
    assert call(eps=-1.0) == AQ_EINVAL and call(eps=math.nan) == AQ_EINVAL
    assert call(max_depth=-1) == AQ_EINVAL and call(max_depth=128) == AQ_EINVAL
    assert call(f=7) == AQ_EINVAL and call(f=-1) == AQ_EINVAL
    assert call(f=PARAM) == AQ_EINVAL and call(theta=th.data_ptr()) == AQ_EINVAL   # theta exactly with PARAM
    assert call(n=0, a_=None, b_=None) == 0
    assert call() == 0 and call(f=PARAM, theta=th.data_ptr()) == 0   # (no outputs asked for: legal)
    assert ctx.device_batch_check() == 0
    for bad in (dict(a=a.cpu()), dict(a=a.float()), dict(a=torch.zeros(8, dtype=torch.float64, device="cuda:0")[::2]),
                dict(b=b[:3]), dict(a=np.zeros(4)), dict(theta=th), dict(integrand=PARAM), dict(integrand=PARAM, theta=th[:3]),
                dict(out=(a, a, a, None, None, a))):
        kw = dict(a=a, b=b, eps=1e-3)
        kw.update(bad)
        with pytest.raises(ValueError):
            ctx.integrate_batch_device(**kw)
    out = ctx.integrate_batch_device(a, b, 1e-3, err=True)
    again = ctx.integrate_batch_device(a, b, 1e-3, err=True, out=out)
    assert all(x is y for x, y in zip(out, again))
    assert out.tasks.dtype == torch.int64 and out.status.dtype == torch.int32 and int(out.tasks.min()) >= 1
