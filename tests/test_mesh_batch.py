"""Batched meshes without a GPU: the three functions declared, bound, exported and refusing a NULL context on the
host; and the CPU reference (tests/mesh_batch_reference.py), which the GPU tests compare with bit for bit, checked
against the references it extends and for the shapes the GPU cases rely on. (On the GPU: tests/test_gpu_mesh_batch.py.)"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import mesh_batch_reference as mbr
import mesh_reference as mr
import param_reference as pr

AQ_EINVAL = -1
NAMES = ("aq_integrate_mesh_batch", "aq_mesh_eval_batch", "aq_mesh_invert_batch")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_declared_bound_exported_and_null_context_refused():
    from test_abi import header_functions
    from ppls_amd import _lib
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aq_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert name in header_functions() and name in _lib.EXPORTS and name in exported
        assert getattr(lib, name).restype is ctypes.c_int
    io, info = _lib.aq_mesh_batch_io(), _lib.aq_mesh_batch_info()
    assert lib.aq_integrate_mesh_batch(None, 1, ctypes.byref(io), 1e-3, 0, 16, 4, 16, ctypes.byref(info)) == AQ_EINVAL
    for name in NAMES[1:]:   # (never dereferenced: the context comes first)
        assert getattr(lib, name)(None, 1, 8, 8, 8, 8, 1, 8, 8) == AQ_EINVAL
        assert getattr(lib, name)(None, 0, None, None, None, None, 0, None, None) == AQ_EINVAL
    # the structures are the header's: 12 pointers and two int32; four uint64 and two uint32
    assert ctypes.sizeof(_lib.aq_mesh_batch_io) == 12 * 8 + 8 and ctypes.sizeof(_lib.aq_mesh_batch_info) == 40


def test_one_leaf_rows_and_the_table_of_the_edges_case():
    integrand, a, b, theta, eps, ref = mbr.case("edges")
    assert a.size == 307 and eps == 1e-5 and theta is None
    assert np.all(ref.accepted[:300] == 1) and np.all(ref.tasks[:300] == 1)
    got = {(float(a[i]), float(b[i])): (int(ref.accepted[i]), ref.rows[i].levels if ref.rows[i] else None)
           for i in range(300, 307)}
    assert got == {(-3.0, 2.0): (1382, 14), (1.0, 1.0): (1, 1), (2.0, 1.0): (0, None), (0.0, 171.0): (0, None),
                   (0.0, 5.0): (15573, 18), (-1.0, 0.5): (83, 8), (0.0, 0.25): (8, 4)}
    assert list(ref.status[300:]) == [0, 0, mbr.ROW_INVALID, mbr.ROW_INVALID, 0, 0, 0] and ref.invalid_rows == 2
    assert np.isnan(ref.area[302]) and np.isnan(ref.area[303]) and ref.offsets[302] == ref.offsets[303] == ref.offsets[304]
    # a head at leaf 300 (lane 44 of scan block 1), segments of many blocks, levels of several 1024-record chunks
    assert int(ref.accepted[:300].sum()) == 300 and ref.accepted[300] > 4 * 256 and ref.widest_level > 2 * 1024
    assert list(ref.depth_status(8)[300:]) == [mbr.ROW_DEPTH, 0, mbr.ROW_INVALID, mbr.ROW_INVALID, mbr.ROW_DEPTH, 0, 0]
    assert ref.n_nodes == 2 * ref.leaves + 305 and ref.tasks_total == 2 * ref.leaves - 305


def test_scale_and_sin_rows():
    _, a, b, _, eps, ref = mbr.case("scale")
    assert eps == 1e163 and list(ref.accepted) == [1552, 1, 1]
    for i in (1, 2):   # one leaf: no summation in its three cum values
        r = ref.rows[i]
        larea = (r.f[0] + r.f[1]) * (r.x[1] - r.x[0]) / 2
        rarea = (r.f[1] + r.f[2]) * (r.x[2] - r.x[1]) / 2
        assert np.array_equal(_bits(r.cum), _bits(np.array([0.0, larea, larea + rarea])))
    assert ref.area[0] > 1e170 and ref.area[1] < 10    # a global prefix would lose every bit of rows 1 and 2
    _, a, b, _, eps, ref = mbr.case("sin")
    assert all(np.any(np.diff(r.cum) < 0) for r in ref.rows[:2])   # non-monotone cum


def test_param_rows_at_unit_theta_are_the_user_meshes():
    _, a, b, theta, eps, ref = mbr.case("param_unit")
    for i in range(mbr.PARAM_N):
        m = mr.reference_mesh(mr.USER, float(a[i]), float(b[i]), eps)
        r = ref.rows[i]
        for u, v in ((r.x, m.x), (r.f, m.f), (r.cum, m.cum)):
            assert np.array_equal(_bits(u), _bits(v))
        assert np.array_equal(r.level, m.level) and (r.tasks, r.accepted, r.levels) == (m.tasks, m.accepted, m.levels)


def test_param_shapes():
    _, a, b, theta, eps, ref = mbr.case("param")
    assert eps == 1e-6 and ref.leaves == 11596 and ref.widest_level == 6306
    assert (int(ref.accepted.min()), int(ref.accepted.max())) == (27, 436)
    w = pr.draw_reference(mbr.PARAM_N)[3]
    assert np.array_equal(ref.accepted, w["leaves"]) and np.array_equal(ref.tasks, w["tasks"])
    _, _, _, _, _, one = mbr.case("param_one")
    t = pr.tree_reference(pr.TREE_SHIFTED)
    assert (one.leaves, one.tasks_total, one.levels) == (21319, t["tasks"], t["levels"]) and t["leaves"] == 21319
    assert list(one.tasks_per_level) == t["tasks_per_level"]


def test_the_query_restatements_are_per_row_calls():
    _, a, b, _, _, ref = mbr.case("edges")
    rows = [0, 299, 300, 301, 302, 305]
    q = np.stack([mbr.queries(ref.rows[i].x) if ref.rows[i] else np.zeros(257) for i in rows])
    off = np.concatenate([[0], np.cumsum([ref.offsets[i + 1] - ref.offsets[i] for i in rows])])
    x, f, cum = (np.concatenate([v[ref.offsets[i]:ref.offsets[i + 1]] for i in rows]) for v in (ref.x, ref.f, ref.cum))
    ev = mbr.mesh_eval_batch(off, x, f, cum, q)
    assert ev.shape == (6, 257) and np.isnan(ev[4]).all()            # the empty row
    assert np.isnan(ev[2, 254:]).all() and not np.isnan(ev[2, :254]).any()   # two points outside and a NaN, last
    r = ref.rows[300]
    assert np.array_equal(_bits(ev[2, :254]), _bits(mr.mesh_eval(r.x, r.f, r.cum, q[2, :254])))
    inv = mbr.mesh_invert_batch(off, x, f, cum, ev)
    assert np.isnan(inv[4]).all() and np.all((inv[2, :254] >= r.x[0]) & (inv[2, :254] <= r.x[-1]))
