"""Mesh moments on the GPU (aq_mesh_moments_batch and Context.mesh_moments / mesh_stats / mesh_tail_mean) against
tests/mesh_moments_reference.py, which shares nothing with the code under test.

The bound: for every row and k, |got - S| <= P 2^-100 sum|t_k| + ulp(S) / 2, S the exact sum of the reference's double
terms, P the panels in range -- the double-double sum's stated bound and its one rounding (the shape of
mesh_refine_cases.test_err_sums). It holds only if every term on the GPU is the reference's double, bit for bit. NaN
rows are NaN, lo == hi rows +0.0, and every output is bit-identical between runs, between batches, and between orders.

The cases are mesh_batch_reference's four and the synthetic batch (its shape is asserted in tests/test_mesh_moments.py):
rows of 0 .. 4097 leaves at the wave, chunk and blocks-per-row edges, at even and odd offsets, f of both signs.

Not collected by name: tests/test_gpu_mesh_moments.py runs this file as one child pytest process that imports torch
before the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import numpy as np
import pytest

import mesh_batch_reference as mbr
import mesh_moments_reference as mm
from mesh_batch_cases import FRONTIER_CAP, POISON, _bits, _dev

pytestmark = pytest.mark.gpu

AQ_EINVAL = -1
K = mm.MAX_ORDER
PARITY = ["edges", "param", "sin", "scale", "synthetic"]


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
    """A batch of the reference module on the device (a batch without nodes: one element, so no pointer is NULL)."""

    def __init__(self, torch, batch):
        self.n = batch.n
        self.offsets = _dev(torch, np.array(batch.offsets, np.int64))
        self.x, self.f = (_dev(torch, np.concatenate([v, [0.0]]) if v.size == 0 else v.copy()) for v in (batch.x, batch.f))


def _enqueue(ctx, torch, src, order, c=None, lo=None, hi=None, null=(), n=None):
    """The call itself on an output of n (order + 1) + 1 poisoned elements; returns (rc, the output tensor, the
    per-row argument tensors, which must outlive the kernels)."""
    n = src.n if n is None else n
    out = torch.full((src.n * (min(max(order, 0), K) + 1) + 1,), POISON, dtype=torch.float64, device="cuda:0")
    args = [None if v is None else _dev(torch, np.asarray(v, np.float64)) for v in (c, lo, hi)]
    torch.cuda.synchronize()
    ptr = lambda k, t: None if (k in null or t is None) else t.data_ptr()   # noqa: E731
    rc = ctx.L.aq_mesh_moments_batch(ctx._h, n, ptr("offsets", src.offsets), ptr("x", src.x), ptr("f", src.f), order,
                                     ptr("c", args[0]), ptr("lo", args[1]), ptr("hi", args[2]), ptr("out", out))
    return rc, out, args


def _moments(ctx, torch, src, order, c=None, lo=None, hi=None):
    rc, out, _ = _enqueue(ctx, torch, src, order, c, lo, hi)
    assert rc == 0
    ctx.synchronize()
    out = out.cpu().numpy()
    assert out[-1] == POISON                       # the element past the end
    return out[:-1].reshape(src.n, order + 1)


def _check(got, ex, what):
    """got (n, K' + 1) against moments_exact's rows; returns the worst deviation / bound."""
    worst = 0.0
    for i, (state, S, A, P) in enumerate(ex):
        if state == mm.NAN:
            assert np.isnan(got[i]).all(), (what, i)
        elif state == mm.ZERO:
            assert np.all(_bits(got[i]) == 0), (what, i)           # +0.0
        else:
            for k in range(got.shape[1]):
                ok, r = mm.bound(got[i, k], S[k], A[k], P)
                assert ok, (what, i, k, got[i, k], float(S[k]), r)
                worst = max(worst, r)
    return worst


@pytest.mark.parametrize("name", PARITY)
def test_parity(ctx, torch, name):
    b = mm.case(name)
    src = Src(torch, b)
    rows = np.arange(0, b.n, 2)
    sub = mm.sub_batch(b, rows)
    ssrc = Src(torch, sub)
    for c in (None, mm.middles(b)):
        what = "%s, centre %s" % (name, "0" if c is None else "the middle")
        got = _moments(ctx, torch, src, K, c)
        ex = mm.moments_exact(b, K, c)
        worst = _check(got, ex, what)
        print(what, "rows", b.n, "NaN rows", sum(e[0] == mm.NAN for e in ex), "worst deviation / bound %.3f" % worst)
        assert np.array_equal(_bits(got), _bits(_moments(ctx, torch, src, K, c)))                  # a second run
        # every second row in a batch of its own: every offset moves
        assert np.array_equal(_bits(_moments(ctx, torch, ssrc, K, None if c is None else c[rows])), _bits(got[rows]))
        for order in range(K):                                                                      # the leading columns
            assert np.array_equal(_bits(_moments(ctx, torch, src, order, c)), _bits(got[:, :order + 1])), order
    if name == "edges":
        assert sum(e[0] == mm.NAN for e in ex) == mbr.case("edges")[5].invalid_rows == 2
        assert [e[0] for e in ex].count(mm.ZERO) == 1                  # the zero-width row [1, 1]


@pytest.mark.parametrize("name", ["param", "synthetic"])
def test_ranges(ctx, torch, name):
    b = mm.case(name)
    src = Src(torch, b)
    c = mm.middles(b)
    base = _moments(ctx, torch, src, K, c)
    sets = mm.range_sets(b)
    assert {"ends", "even_nodes", "odd_nodes", "lo_node_hi_inside", "one_panel", "first_and_last", "empty", "below", "above",
            "reversed", "nan_lo", "nan_hi"} == set(sets)
    third = np.arange(b.n) % 3 == 1
    for key, (lo, hi, must_nan) in sets.items():
        got = _moments(ctx, torch, src, K, c, lo, hi)
        ex = mm.moments_exact(b, K, c, lo, hi)
        worst = _check(got, ex, "%s %s" % (name, key))
        print(name, key, "NaN rows", int(np.isnan(got[:, 0]).sum()), "worst deviation / bound %.3f" % worst)
        assert np.isnan(got[must_nan]).all()
        if key == "ends":                          # the row's own ends given explicitly: the bits of NULL
            assert np.array_equal(_bits(got), _bits(base))
            for l, h in ((lo, None), (None, hi)):
                assert np.array_equal(_bits(_moments(ctx, torch, src, K, c, l, h)), _bits(base))
        if key == "empty":
            assert all(e[0] in (mm.NAN, mm.ZERO) for e in ex)
        if key in ("below", "above", "reversed", "nan_lo", "nan_hi"):
            assert must_nan[third].sum() >= 3 and np.array_equal(_bits(got[~third]), _bits(base[~third]))
        if key == "one_panel":
            assert all(e[3] == 1 for e in ex if e[0] == mm.SUM)


def test_arguments_and_memory(torch):
    from ppls_amd import Context
    b = mm.case("scale")
    src = Src(torch, b)
    want = mm.moments_exact(b, K)
    with Context(0) as c:
        before = c.device_bytes
        for name in ("offsets", "x", "f", "out"):
            rc, out, _ = _enqueue(c, torch, src, 2, null=(name,))
            assert rc == AQ_EINVAL, name
        for order in (-1, K + 1, 1 << 20, -(1 << 31)):
            rc, out, _ = _enqueue(c, torch, src, order)
            assert rc == AQ_EINVAL and np.all(out.cpu().numpy() == POISON), order
        assert c.L.aq_mesh_moments_batch(None, src.n, src.offsets.data_ptr(), src.x.data_ptr(), src.f.data_ptr(), 2, None,
                                         None, None, out.data_ptr()) == AQ_EINVAL
        # an n the err call refuses (8 blocks per row: n * 8 must stay below 2^31): before anything is allocated or enqueued
        rc, out, _ = _enqueue(c, torch, src, 2, n=0x7fffffff // 8 + 1)
        assert rc == AQ_EINVAL and np.all(out.cpu().numpy() == POISON)
        d = out.data_ptr()
        assert c.L.aq_mesh_err_batch(c._h, 0x7fffffff // 8 + 1, src.offsets.data_ptr(), src.x.data_ptr(), src.f.data_ptr(), d, d) == AQ_EINVAL
        # n == 0: nothing enqueued, whatever the pointers
        rc, out, _ = _enqueue(c, torch, src, 2, n=0)
        assert rc == 0 and np.all(out.cpu().numpy() == POISON)
        assert c.L.aq_mesh_moments_batch(c._h, 0, None, None, None, 0, None, None, None, None) == 0
        assert c.device_bytes == before
        got = _moments(c, torch, src, K)
        _check(got, want, "scale")
        after = c.device_bytes
        assert after > before
        assert np.array_equal(_bits(_moments(c, torch, src, K)), _bits(got)) and c.device_bytes == after
        assert np.array_equal(_bits(_moments(c, torch, src, 1)), _bits(got[:, :2])) and c.device_bytes == after
        # every row without nodes: NaN everywhere
        none = mm.as_batch([None, None, None])
        assert np.isnan(_moments(c, torch, Src(torch, none), 2)).all()


def test_interleaved_on_one_context(torch):
    """mesh_err, mesh_moments and mesh_err enqueued back to back on one context, no synchronisation between them:
    each gives the bits of its own lone run (the two calls' block partials are separate buffers)."""
    from ppls_amd import Context
    b1, b2 = mm.case("edges"), mm.case("synthetic")
    s1, s2 = Src(torch, b1), Src(torch, b2)
    c2 = mm.middles(b2)

    def err(c, src):
        ea, es = (torch.full((src.n,), POISON, dtype=torch.float64, device="cuda:0") for _ in range(2))
        torch.cuda.synchronize()
        assert c.L.aq_mesh_err_batch(c._h, src.n, src.offsets.data_ptr(), src.x.data_ptr(), src.f.data_ptr(), ea.data_ptr(),
                                     es.data_ptr()) == 0
        return ea, es

    with Context(0) as fresh:
        lone_e1 = err(fresh, s1)
        fresh.synchronize()
        lone_e1 = [t.cpu().numpy() for t in lone_e1]
    with Context(0) as fresh:
        lone_m = _moments(fresh, torch, s2, K, c2)
    with Context(0) as fresh:
        lone_e2 = err(fresh, s2)
        fresh.synchronize()
        lone_e2 = [t.cpu().numpy() for t in lone_e2]
    with Context(0) as c:
        e1 = err(c, s1)
        rc, out, held = _enqueue(c, torch, s2, K, c2)
        e2 = err(c, s2)
        assert rc == 0
        c.synchronize()
        for got, want in zip(e1 + e2, lone_e1 + lone_e2):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
        assert np.array_equal(_bits(out.cpu().numpy()[:-1].reshape(s2.n, K + 1)), _bits(lone_m))
        del held


def _host_batch(mesh):
    """A MeshBatch's own offsets, x and f as a batch of the reference module."""
    off, x, f = (t.cpu().numpy() for t in (mesh.offsets, mesh.x, mesh.f))
    return mm.as_batch([None if off[i + 1] == off[i] else (x[off[i]:off[i + 1]], f[off[i]:off[i + 1]]) for i in range(off.size - 1)])


def test_python_surface(ctx, torch):
    integrand, a, b, theta, feps, fine = mbr.case("param")
    mesh = ctx.integrate_mesh_batch(_dev(torch, a), _dev(torch, b), feps, integrand=integrand, theta=_dev(torch, theta),
                                    cap_nodes=fine.n_nodes, frontier_cap=FRONTIER_CAP)
    hb = _host_batch(mesh)
    n = len(mesh)
    assert np.array_equal(_bits(hb.x), _bits(fine.x)) and np.array_equal(_bits(hb.f), _bits(fine.f))
    # floats for every row, None, and tensors
    got = ctx.mesh_moments(mesh, order=3, center=0.25)
    assert tuple(got.shape) == (n, 4) and got.dtype == torch.float64 and got.is_cuda
    _check(got.cpu().numpy(), mm.moments_exact(hb, 3, 0.25), "center=0.25")
    assert tuple(ctx.mesh_moments(mesh).shape) == (n, 3)
    mid = mm.middles(hb)
    lo, hi = mm.range_sets(hb)["first_and_last"][:2]
    got = ctx.mesh_moments(mesh, 4, _dev(torch, mid), _dev(torch, lo), _dev(torch, hi))
    _check(got.cpu().numpy(), mm.moments_exact(hb, 4, mid, lo, hi), "tensors")
    qlo = float(max(r[0][0] for r in hb.rows))
    got = ctx.mesh_moments(mesh, 1, None, qlo, None).cpu().numpy()      # a float lo: NaN where it lies outside the row
    ex = mm.moments_exact(hb, 1, None, qlo, None)
    _check(got, ex, "float lo")
    assert 0 < sum(e[0] == mm.NAN for e in ex) < n
    for bad in (dict(order=5), dict(order=-1), dict(center=torch.zeros(n, dtype=torch.float64)),
                dict(lo=torch.zeros(n + 1, dtype=torch.float64, device="cuda:0")),
                dict(hi=torch.zeros(n, dtype=torch.float32, device="cuda:0"))):
        with pytest.raises(ValueError):
            ctx.mesh_moments(mesh, **bad)

    # mesh_stats: the numpy restatement on the GPU's own moment tensors; every output within 2^-48 times the largest
    # absolute intermediate of its formula (at most 12 operations, each within one ulp of its own result; torch's
    # division and square root taken as faithful)
    for lo_t, hi_t in ((None, None), (_dev(torch, lo), _dev(torch, hi))):
        st = ctx.mesh_stats(mesh, lo_t, hi_t)
        assert st._fields == ("mass", "mean", "var", "skew", "kurt")
        first = ctx.mesh_moments(mesh, 1, None, lo_t, hi_t)
        c = (first[:, 1] / first[:, 0]).contiguous()
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(mm.centre_from(first.cpu().numpy())))
        M = ctx.mesh_moments(mesh, 4, c, lo_t, hi_t).cpu().numpy()
        want, scale = mm.stats(c.cpu().numpy(), M)
        for k in st._fields:
            g = getattr(st, k).cpu().numpy()
            assert g.shape == (n,) and np.all(np.isfinite(g))
            dev = np.abs(g - want[k])
            assert np.all(dev <= 2.0 ** -48 * scale[k]), (k, float((dev / scale[k]).max()))
            print("mesh_stats", k, "worst deviation / (2^-48 scale) %.3g" % float((dev / (2.0 ** -48 * scale[k])).max()))
        # and against the reference's own moments, loosely: the statistics of the same densities
        ref = mm.mesh_stats(hb, None if lo_t is None else lo, None if hi_t is None else hi)
        assert np.allclose(st.mass.cpu().numpy(), ref["mass"], rtol=1e-13, atol=0) and np.allclose(st.mean.cpu().numpy(), ref["mean"], rtol=1e-9, atol=1e-12)

    # rows without nodes, and a mass of 0, give NaN
    _, ea, eb, _, eeps, efine = mbr.case("edges")
    emesh = ctx.integrate_mesh_batch(_dev(torch, ea), _dev(torch, eb), eeps, cap_nodes=efine.n_nodes, frontier_cap=FRONTIER_CAP)
    est = ctx.mesh_stats(emesh)
    invalid = efine.status != 0
    zero = (ea == eb) & ~invalid
    assert invalid.sum() == 2 and zero.sum() == 1
    mass, mean = est.mass.cpu().numpy(), est.mean.cpu().numpy()
    assert np.isnan(mass[invalid]).all() and np.all(mass[zero] == 0.0) and np.isfinite(mass[~invalid]).all()
    for k in ("mean", "var", "skew", "kurt"):
        g = getattr(est, k).cpu().numpy()
        assert np.isnan(g[invalid | zero]).all() and np.isfinite(g[~(invalid | zero)]).all(), k

    # mesh_tail_mean at u = 0.05, both tails, against the reference's moments over the q the GPU returned. Each GPU
    # moment lies within the parity bound of the exact sum (checked here), so within an ulp of the reference's rounded
    # moment; a quotient of two such values and its own rounding: within (2 + 2 + 1) 2^-53 < 2^-50, relative.
    u = torch.tensor([0.05], dtype=torch.float64, device="cuda:0")
    q = ctx.mesh_quantiles(mesh, u)
    qh = q.cpu().numpy()[:, 0]
    assert np.all(np.isfinite(qh))
    for upper in (False, True):
        got = ctx.mesh_tail_mean(mesh, u, upper=upper)
        assert tuple(got.shape) == (n, 1)
        rlo, rhi = (qh, None) if upper else (None, qh)
        gm = ctx.mesh_moments(mesh, 1, None, None if rlo is None else _dev(torch, rlo), None if rhi is None else _dev(torch, rhi))
        _check(gm.cpu().numpy(), mm.moments_exact(hb, 1, None, rlo, rhi), "tail %s" % upper)
        want = mm.tail_mean(mm.moments(hb, 1, None, rlo, rhi))
        g = got.cpu().numpy()[:, 0]
        assert np.all(np.abs(g - want) <= 2.0 ** -50 * np.abs(want)), float(np.max(np.abs(g - want) / np.abs(want)))
        inside = (g >= qh) if upper else (g <= qh)
        assert inside.all()
    two = ctx.mesh_tail_mean(mesh, [0.05, 0.5])
    assert tuple(two.shape) == (n, 2) and np.array_equal(_bits(two.cpu().numpy()[:, 0]), _bits(ctx.mesh_tail_mean(mesh, u).cpu().numpy()[:, 0]))
