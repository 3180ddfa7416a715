"""The accepted mesh without a GPU: both entry points declared, exported, bound, and refusing on the host what no
context can be given for; and the CPU reference mesh (tests/mesh_reference.py), which the GPU tests compare with bit
for bit, checked against the oracle's own totals. (On the GPU: tests/test_gpu_mesh.py.)"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import mesh_reference as mr

NAMES = ["aq_integrate_mesh", "aq_mesh_eval"]
AQ_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from ppls_amd import _lib
    return _lib.load()


def test_declared_bound_and_exported(lib):
    from test_abi import header_functions
    from ppls_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aq_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert name in header_functions() and name in _lib.EXPORTS and name in exported
        assert getattr(lib, name).restype is ctypes.c_int
    assert [f[0] for f in _lib.aq_mesh_io._fields_] == ["x", "f", "cum", "level"]
    assert ctypes.sizeof(_lib.aq_mesh_io) == 32


def test_null_context_is_refused_on_the_host(lib):
    from ppls_amd import _lib
    p = _lib.aq_problem(0, 0, 0.0, 5.0, 1e-3, 0, 0)
    io = _lib.aq_mesh_io(8, 8, 8, None)   # (never dereferenced: the context is checked first)
    r = _lib.aq_result()
    n = ctypes.c_uint64(7)
    assert lib.aq_integrate_mesh(None, ctypes.byref(p), 1 << 16, 4, 1001, ctypes.byref(io), ctypes.byref(r),
                                 ctypes.byref(n)) == AQ_EINVAL
    assert lib.aq_integrate_mesh(None, None, 1 << 16, 4, 1001, None, None, None) == AQ_EINVAL
    assert n.value == 7
    assert lib.aq_mesh_eval(None, 3, 8, 8, 8, 1, 8, 8) == AQ_EINVAL
    assert lib.aq_mesh_eval(None, 3, None, None, None, 0, None, None) == AQ_EINVAL


SIZES = {"cosh4_0_5_1e-6": (34068, 19), "cosh4_-3_2_1e-5": (1382, 14), "sin_recip_1e-3_1_1e-5": (391, 17),
         "gauss_-4_4_1e-7": (564, 11), "cosh4_root_leaf": (1, 1)}


@pytest.mark.parametrize("name,integrand,a,b,eps", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_reference_mesh_agrees_with_the_oracle(oracle, name, integrand, a, b, eps):
    want = oracle.integrate(integrand, a, b, eps)
    m = mr.reference_mesh(integrand, a, b, eps)
    assert (m.accepted, m.levels) == SIZES[name]
    assert (m.tasks, m.accepted, m.levels) == (want.tasks, want.leaves, want.levels)
    assert m.x.size == m.f.size == m.cum.size == 2 * m.accepted + 1 and m.level.size == 2 * m.accepted
    # contiguous leaves from a to b, nodes strictly increasing
    assert m.l[0] == a and m.r[-1] == b and np.array_equal(m.r[:-1], m.l[1:])
    assert m.x[0] == a and m.x[-1] == b and np.all(np.diff(m.x) > 0)
    assert np.array_equal(m.f, oracle.F(m.x, integrand))
    # the leaves on each level are the oracle's histogram
    assert [int(c) // 2 for c in np.bincount(m.level, minlength=m.levels)] == want.leaves_per_level
    # the exact total, rounded once, against the oracle's quad-precision area
    assert m.cum[0] == 0.0 and m.cum[-1] == float(m.total)
    assert abs(m.cum[-1] - want.area) <= np.spacing(abs(want.area))
    assert np.all(np.diff(m.cum) >= 0) or integrand == mr.SIN_RECIP


def test_mesh_eval_restatement():
    """The formula at nodes, at a panel's end and outside: cum at a node, the full panel at its right end, NaN outside."""
    _, integrand, a, b, eps = mr.CASES[1]
    m = mr.reference_mesh(integrand, a, b, eps)
    out = mr.mesh_eval(m.x, m.f, m.cum, m.x[:-1])
    assert np.array_equal(out.view(np.int64), m.cum[:-1].view(np.int64))
    q = np.array([a, b, a - 1e-9, b + 1e-9, np.nan, 0.5 * (m.x[10] + m.x[11])])
    out = mr.mesh_eval(m.x, m.f, m.cum, q)
    assert out[0] == 0.0 and np.isnan(out[2:5]).all() and m.cum[10] < out[5] < m.cum[11]
    assert abs(out[1] - m.cum[-1]) <= 4 * np.spacing(m.cum[-1])
