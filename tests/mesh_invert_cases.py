"""Mesh inversion on the GPU (Context.mesh_invert / aq_mesh_invert, Context.mesh_sample) against its numpy restatement
(tests/mesh_invert_reference.py), bit for bit and with NaN exactly where the restatement has it, through both kernel
instances: AQ_MESH_INVERT=0 forces the plain binary search, 1 the search staged through an LDS table, None leaves the
choice to the library. The meshes are uploaded from tests/mesh_reference.py, so only the end-to-end case depends on
integrate_mesh.

Not collected by name: tests/test_gpu_mesh_invert.py runs this file as one child pytest process that imports torch
before the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import os

import numpy as np
import pytest

import mesh_invert_reference as mir
import mesh_reference as mr

pytestmark = pytest.mark.gpu

AQ_EINVAL = -1
FRONTIER_CAP = 1 << 16
INSTANCES = ["0", "1"]
# the staged instance's constants (ppls_amd/csrc/aq_abi.inc MINV_*)
TAB = 2048          # entries of its LDS table: a mesh of n_nodes <= TAB + 1 fits whole, at stride 1
WG_PER_CU = 8       # its grid: at most this many workgroups of 256 threads per CU ...
QPT = 4             # ... and no more than give every thread this many queries
STAGED_MIN_NQ = 1 << 21   # the library's own choice: staged from this many queries
POISON = -7.25


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


class forced:
    """AQ_MESH_INVERT in the environment for the calls inside (the library reads it per call)."""

    def __init__(self, instance):
        self.instance = instance

    def __enter__(self):
        self.old = os.environ.pop("AQ_MESH_INVERT", None)
        if self.instance is not None:
            os.environ["AQ_MESH_INVERT"] = self.instance

    def __exit__(self, *exc):
        os.environ.pop("AQ_MESH_INVERT", None)
        if self.old is not None:
            os.environ["AQ_MESH_INVERT"] = self.old


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


def _same(got, want):
    """Bit for bit, NaN exactly where the restatement has it."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (int(np.isnan(got).sum()), int(nan.sum()))
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan])), int((_bits(got[~nan]) != _bits(want[~nan])).sum())


def _edges(cum):
    return np.array([0.0, cum[-1], -1e-9, np.nextafter(cum[-1], np.inf), np.nan])


@pytest.mark.parametrize("instance", INSTANCES)
@pytest.mark.parametrize("case", mir.MONOTONE, ids=[c[0] for c in mir.MONOTONE])
def test_parity(ctx, torch, case, instance):
    m = mir.mesh(case)
    y = np.concatenate([mir.queries(m.cum, 47), _edges(m.cum)])
    want = mir.mesh_invert(m.x, m.f, m.cum, y)
    assert int(np.isnan(want).sum()) == 3
    x, f, cum, dy = _dev(torch, m.x, m.f, m.cum, y)
    with forced(instance):
        got = ctx.mesh_invert(x, f, cum, dy)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == dy.shape
    _same(got.cpu().numpy(), want)


@pytest.mark.parametrize("instance", INSTANCES)
def test_parity_through_integrate_mesh(ctx, torch, instance):
    """End to end: the mesh integrate_mesh returns (its cum may sit one ulp off the reference's), a 2-d y."""
    from ppls_amd import Problem
    _, integrand, a, b, eps = mr.CASES[0]
    res, x, f, cum, level = ctx.integrate_mesh(Problem(integrand, a, b, eps), frontier_cap=FRONTIER_CAP)
    hx, hf, hcum = (t.cpu().numpy() for t in (x, f, cum))
    y = np.concatenate([mir.queries(hcum, 48), _edges(hcum)])
    want = mir.mesh_invert(hx, hf, hcum, y)
    dy = _dev(torch, y)[0]
    with forced(instance):
        _same(ctx.mesh_invert(x, f, cum, dy).cpu().numpy(), want)
        got = ctx.mesh_invert(x, f, cum, dy[-6000:].reshape(60, 100).contiguous())
    assert tuple(got.shape) == (60, 100)
    _same(got.cpu().numpy().ravel(), want[-6000:])


# n_nodes at which the staged search changes shape: the whole cum fits the table up to TAB + 1 nodes (the search is
# over indices 0 .. n_nodes - 2); the stride doubles past TAB * 2^s + 1 nodes, where the table holds its TAB
# entries, TAB / 2 + 1 of them one node later
PREFIXES = [3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 68137] + \
    [TAB - 1, TAB, TAB + 1, TAB + 2, TAB + 3] + [(TAB << s) + d for s in (1, 2, 3, 4, 5) for d in (0, 1, 2)] + \
    [9, 10, 11, 16, 17, 18]   # the register steps: a run of 8 that ends at, before and after the last node


@pytest.mark.parametrize("instance", INSTANCES)
def test_prefix_sweep(ctx, torch, instance):
    """Any prefix of a mesh with at least 3 nodes is a mesh: every node of the prefix and 1024 random y."""
    m = mir.mesh(mir.MONOTONE[0])
    assert m.x.size == 68137
    x, f, cum = _dev(torch, m.x, m.f, m.cum)
    rng = np.random.default_rng(49)
    with forced(instance):
        for n in PREFIXES:
            y = np.concatenate([m.cum[:n], rng.uniform(0.0, m.cum[n - 1], 1024)])
            got = ctx.mesh_invert(x[:n], f[:n], cum[:n], _dev(torch, y)[0]).cpu().numpy()
            _same(got, mir.mesh_invert(m.x[:n], m.f[:n], m.cum[:n], y))


def test_query_counts(ctx, torch):
    """nq around a workgroup, nq that is no multiple of the grid-stride step (the staged instance: 256 threads times
    min(ceil(nq / (256 * QPT)), WG_PER_CU * CUs) workgroups -- 5000 gives 5 workgroups, the large count a full grid
    and a ragged last pass), and the library's own choice on either side of its switch-over. Nothing is written past
    nq."""
    m = mir.mesh(mir.MONOTONE[1])
    x, f, cum = _dev(torch, m.x, m.f, m.cum)
    step = 256 * WG_PER_CU * ctx.num_cus
    big = max(QPT * step, STAGED_MIN_NQ) + 3 * 256 + 77
    assert big % step
    y = np.random.default_rng(50).uniform(0.0, m.cum[-1], big)
    want = mir.mesh_invert(m.x, m.f, m.cum, y)
    dy = _dev(torch, y)[0]
    for instance in INSTANCES + [None]:
        for nq in (0, 1, 255, 256, 257, 5000, STAGED_MIN_NQ - 1, STAGED_MIN_NQ, big):
            out = torch.full((nq + 512,), POISON, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            with forced(instance):
                assert ctx.L.aq_mesh_invert(ctx._h, m.x.size, x.data_ptr(), f.data_ptr(), cum.data_ptr(), nq,
                                            dy.data_ptr(), out.data_ptr()) == 0
            assert ctx.L.aq_synchronize(ctx._h) == 0
            got = out.cpu().numpy()
            assert np.all(got[nq:] == POISON), (instance, nq)
            assert np.array_equal(_bits(got[:nq]), _bits(want[:nq])), (instance, nq)


@pytest.mark.parametrize("instance", INSTANCES)
def test_non_monotone_mesh_gives_nan_or_a_point_of_the_mesh(ctx, torch, instance):
    """sin(1/x): cum goes down as well as up. Every output is NaN or inside [x_0, x_m], and nothing faults."""
    m = mir.mesh(mir.NON_MONOTONE)
    y = np.concatenate([m.cum, 0.5 * (m.cum[:-1] + m.cum[1:]),
                        np.random.default_rng(51).uniform(m.cum.min() - 0.01, m.cum.max() + 0.01, 4096)])
    x, f, cum, dy = _dev(torch, m.x, m.f, m.cum, y)
    out = torch.empty_like(dy)
    torch.cuda.synchronize()
    with forced(instance):
        assert ctx.L.aq_mesh_invert(ctx._h, m.x.size, x.data_ptr(), f.data_ptr(), cum.data_ptr(), y.size,
                                    dy.data_ptr(), out.data_ptr()) == 0
    assert ctx.L.aq_synchronize(ctx._h) == 0
    got = out.cpu().numpy()
    ok = np.isnan(got) | ((got >= m.x[0]) & (got <= m.x[-1]))
    assert ok.all(), got[~ok][:8]
    assert (~np.isnan(got)).sum() > 0


def test_round_trip_on_the_device(ctx, torch):
    """mesh_invert(mesh_eval(q)) is the restatements' round trip bit for bit. (Inverting x itself is as
    ill-conditioned as 1 / F, so no x tolerance is asserted.)"""
    m = mir.mesh(mir.MONOTONE[1])
    q = np.random.default_rng(52).uniform(m.x[0], m.x[-1], 4096)
    x, f, cum, dq = _dev(torch, m.x, m.f, m.cum, q)
    got = ctx.mesh_invert(x, f, cum, ctx.mesh_eval(x, f, cum, dq)).cpu().numpy()
    _same(got, mir.mesh_invert(m.x, m.f, m.cum, mr.mesh_eval(m.x, m.f, m.cum, q)))


def test_mesh_sample(ctx, torch):
    case = [c for c in mir.MONOTONE if c[0] == "gauss_-4_4_1e-7"][0]
    m = mir.mesh(case)
    x, f, cum = _dev(torch, m.x, m.f, m.cum)
    n = 65536
    gens = [torch.Generator(device="cuda:0").manual_seed(1234) for _ in range(2)]
    s = ctx.mesh_sample(x, f, cum, n, generator=gens[0])
    assert s.is_cuda and s.dtype == torch.float64 and tuple(s.shape) == (n,)
    assert torch.equal(s, ctx.mesh_sample(x, f, cum, n, generator=gens[1]))
    s = s.cpu().numpy()
    assert np.all((s >= -4.0) & (s <= 4.0))
    assert ctx.mesh_sample(x, f, cum, 1000).shape == (1000,)   # the default generator
    # five sigma of a fraction is at most 2.5 / sqrt(n): a correct sampler misses 5 / sqrt(n) about once in a million
    quartiles = mir.mesh_invert(m.x, m.f, m.cum, np.array([0.25, 0.5, 0.75]) * m.cum[-1])
    for p, xq in zip((0.25, 0.5, 0.75), quartiles):
        frac = float((s < xq).mean())
        print("quartile", p, "at", xq, "fraction below", frac)
        assert abs(frac - p) <= 5 / np.sqrt(n)


def test_refused_arguments(ctx, torch):
    t = torch.zeros(16, dtype=torch.float64, device="cuda:0")
    d = t.data_ptr()
    assert ctx.L.aq_mesh_invert(ctx._h, 2, d, d, d, 1, d, d) == AQ_EINVAL
    assert ctx.L.aq_mesh_invert(ctx._h, 3, d, d, d, 1, None, d) == AQ_EINVAL
    assert ctx.L.aq_mesh_invert(ctx._h, 3, d, d, None, 1, d, d) == AQ_EINVAL
    assert ctx.L.aq_mesh_invert(ctx._h, 3, d, d, d, 1, d, None) == AQ_EINVAL
    assert ctx.L.aq_mesh_invert(ctx._h, 3, None, None, None, 0, None, None) == 0
    with pytest.raises(ValueError):
        ctx.mesh_invert(t, t, t, t.cpu())
    with pytest.raises(ValueError):
        ctx.mesh_invert(t, t, t[:8], t)


def test_the_call_owns_no_device_memory(torch):
    from ppls_amd import Context
    m = mir.mesh(mir.MONOTONE[1])
    x, f, cum, y = _dev(torch, m.x, m.f, m.cum, m.cum)
    with Context(0) as c:
        before = c.device_bytes
        for instance in INSTANCES:
            with forced(instance):
                c.mesh_invert(x, f, cum, y)
        assert c.device_bytes == before
