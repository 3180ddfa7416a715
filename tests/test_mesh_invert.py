"""Mesh inversion without a GPU: aq_mesh_invert declared, exported, bound and refusing a NULL context on the host; and
its numpy restatement (tests/mesh_invert_reference.py), which the GPU tests compare with bit for bit, checked for the
properties include/aquad.h states. (On the GPU: tests/test_gpu_mesh_invert.py.)"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import mesh_invert_reference as mir
import mesh_reference as mr

AQ_EINVAL = -1


def test_declared_bound_exported_and_null_context_refused():
    from test_abi import header_functions
    from ppls_amd import _lib
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aq_[a-z0-9_]+)$", out, flags=re.M))
    name = "aq_mesh_invert"
    assert name in header_functions() and name in _lib.EXPORTS and name in exported
    assert lib.aq_mesh_invert.restype is ctypes.c_int
    assert lib.aq_mesh_invert(None, 3, 8, 8, 8, 1, 8, 8) == AQ_EINVAL   # (never dereferenced: the context comes first)
    assert lib.aq_mesh_invert(None, 3, None, None, None, 0, None, None) == AQ_EINVAL


def test_the_meshes_are_the_ones_described():
    assert [c[0] for c in mir.MONOTONE] == ["cosh4_0_5_1e-6", "cosh4_-3_2_1e-5", "gauss_-4_4_1e-7", "cosh4_root_leaf",
                                            "gauss_-30_30_1e-7"]
    for case in mir.MONOTONE:
        assert np.all(np.diff(mir.mesh(case).cum) >= 0)
    m = mir.mesh(mir.MONOTONE[-1])
    assert m.accepted == 584 and int((np.diff(m.cum) == 0).sum()) == 5 and int((m.f == 0).sum()) == 2
    assert np.any(np.diff(mir.mesh(mir.NON_MONOTONE).cum) < 0)


@pytest.mark.parametrize("case", mir.MONOTONE, ids=[c[0] for c in mir.MONOTONE])
def test_restatement_on_a_monotone_mesh(case):
    """The residual bound: max(f_k, f_k+1) * spacing(|out|) is what moving out by one place of the x grid changes the
    integral by, 4 * spacing(cum_m) the handful of roundings of the two formulas -- derived, not tuned."""
    m = mir.mesh(case)
    x, f, cum = m.x, m.f, m.cum
    y = mir.queries(cum, 31)
    out = mir.mesh_invert(x, f, cum, y)
    k = mir.panel(cum, y)
    assert not np.isnan(out).any()
    assert np.all(x[k] <= out) and np.all(out <= x[k + 1])
    order = np.argsort(y, kind="stable")
    assert np.all(np.diff(out[order]) >= 0)
    # at a node where cum increases strictly: that node, bit for bit
    strict = np.flatnonzero(np.diff(cum) > 0)
    at = mir.mesh_invert(x, f, cum, cum[strict])
    assert np.array_equal(at.view(np.int64), x[strict].view(np.int64))
    # across a run of equal cum values: the right end of the run
    flat = np.flatnonzero(np.diff(cum[:-1]) == 0)
    if flat.size:
        ends = mir.panel(cum, cum[flat])
        assert np.all(ends > flat) and np.array_equal(mir.mesh_invert(x, f, cum, cum[flat]), x[ends])
    resid = np.abs(mr.mesh_eval(x, f, cum, out) - y)
    bound = np.maximum(f[k], f[k + 1]) * np.spacing(np.abs(out)) + 4 * np.spacing(cum[-1])
    print(case[0], "worst residual / bound", float((resid / bound).max()))
    assert np.all(resid <= bound)


def test_restatement_outside_and_nan():
    m = mir.mesh(mir.MONOTONE[1])
    y = np.array([-1e-300, np.nextafter(m.cum[-1], np.inf), np.nan, -np.inf, np.inf, 0.0, m.cum[-1]])
    out = mir.mesh_invert(m.x, m.f, m.cum, y)
    assert np.isnan(out[:5]).all() and out[5] == m.x[0]
    assert m.x[-2] < out[6] <= m.x[-1]
