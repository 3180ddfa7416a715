"""Mesh coarsening without a GPU: the three functions declared, bound, exported and refusing a NULL context on the
host; and the CPU reference (tests/mesh_coarsen_reference.py), which the GPU tests compare with bit for bit, checked
for the identity the feature rests on -- a fine mesh coarsened to eps' IS the mesh built from the roots at eps' --
for the budget's leaf counts, and for the shapes the GPU cases rely on. (On the GPU: tests/test_gpu_mesh_coarsen.py.)"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import mesh_batch_reference as mbr
import mesh_coarsen_reference as mcr
import mesh_refine_reference as mrr

AQ_EINVAL = -1
NAMES = ("aq_mesh_thresholds_batch", "aq_mesh_budget_batch", "aq_mesh_coarsen_batch")
CASES = ["edges", "param", "sin", "scale"]
BUDGETS = [1, 2, 64, 257]
# (leaves fine, leaves coarse, rows changed, rows) at mesh_refine_reference.COARSE
COUNTS = {"edges": (17347, 3896, 4, 307), "param": (11596, 2904, 64, 64), "sin": (653, 82, 3, 3), "scale": (1554, 153, 1, 3)}


def test_declared_bound_exported_and_null_context_refused():
    from test_abi import header_functions
    from ppls_amd import _lib
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aq_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert name in header_functions() and name in _lib.EXPORTS and name in exported
        assert getattr(lib, name).restype is ctypes.c_int
    io, info = _lib.aq_mesh_batch_io(), _lib.aq_mesh_coarsen_info()
    # (never dereferenced: the context comes first)
    assert lib.aq_mesh_thresholds_batch(None, 1, 8, 8, 8, 8, 8) == AQ_EINVAL
    assert lib.aq_mesh_thresholds_batch(None, 0, None, None, None, None, None) == AQ_EINVAL
    assert lib.aq_mesh_budget_batch(None, 1, 8, 8, 4, 8) == AQ_EINVAL
    assert lib.aq_mesh_budget_batch(None, 0, None, None, 4, None) == AQ_EINVAL
    assert lib.aq_mesh_coarsen_batch(None, 1, 8, 8, 8, 8, None, None, 1e-3, ctypes.byref(io), 16, ctypes.byref(info)) == AQ_EINVAL
    assert lib.aq_mesh_coarsen_batch(None, 0, None, None, None, None, None, None, 1e-3, ctypes.byref(io), 16,
                                     ctypes.byref(info)) == AQ_EINVAL
    # the structure is the header's: four uint64 and two uint32
    assert ctypes.sizeof(_lib.aq_mesh_coarsen_info) == 40


def test_python_surface_is_exported():
    import ppls_amd
    assert hasattr(ppls_amd.Context, "mesh_coarsen") and hasattr(ppls_amd.Context, "mesh_thresholds")


@pytest.mark.parametrize("name", CASES)
def test_a_coarsened_mesh_is_the_mesh_built_at_the_coarser_eps(name):
    integrand, a, b, theta, feps, fine = mbr.case(name)
    ceps = mrr.COARSE[name]
    want = mrr.built(name, ceps)
    got = mcr.coarsen(fine, ceps)
    assert ceps > feps and mrr.same_mesh(got, want)                    # cum included: the same leaves, the same Fractions
    changed = sum(got.rows[i] is not fine.rows[i] for i in range(a.size))
    assert (fine.leaves, got.leaves, changed, a.size) == COUNTS[name]
    assert got.n_nodes == 2 * got.leaves + (a.size - got.invalid_rows)
    # every threshold lies above the eps the mesh was built with; the ends and the odd nodes are as the header says
    thr = mcr.thresholds(fine)
    for i in range(a.size):
        o0, o1 = int(fine.offsets[i]), int(fine.offsets[i + 1])
        if o1 > o0:
            assert thr[o0] == np.inf and thr[o1 - 1] == np.inf and np.all(thr[o0 + 1:o1:2] == 0.0)
            assert np.all(thr[o0 + 2:o1 - 1:2] > feps) and np.all(np.isfinite(thr[o0 + 2:o1 - 1:2]))
    # the threshold form of the same mesh: x[k] bounds a leaf at eps' iff thr[k] > eps'
    for i in range(a.size):
        o0, o1, g0, g1 = (int(v) for v in (fine.offsets[i], fine.offsets[i + 1], got.offsets[i], got.offsets[i + 1]))
        bounds = fine.x[o0:o1][thr[o0:o1] > ceps]
        assert np.array_equal(bounds, got.x[g0:g1:2])
    # nothing merges at the mesh's own eps, below it, or under the mask
    for eps in (feps, 0.0, -1.0, np.nan):
        same = mcr.coarsen(fine, eps)
        assert all(u is v for u, v in zip(same.rows, fine.rows)) and mrr.same_mesh(same, fine)


def test_edges_further_up():
    _, a, _, _, feps, fine = mbr.case("edges")
    first = mcr.coarsen(fine, mrr.EDGES_FIRST)
    assert mrr.same_mesh(first, mrr.built("edges", mrr.EDGES_FIRST)) and (first.leaves, first.n_nodes) == (1098, 2501)
    top = mcr.coarsen(fine, 1e300)
    assert mrr.same_mesh(top, mrr.built("edges", 1e300)) and (top.leaves, top.n_nodes) == (305, 915)
    assert np.all(top.accepted[top.status == 0] == 1)
    # two hops equal one
    assert mrr.same_mesh(mcr.coarsen(mcr.coarsen(fine, 1e-3), mrr.EDGES_FIRST), first)
    thr = mcr.thresholds(fine)
    interior = thr[(thr > 0) & np.isfinite(thr)]
    assert feps < interior.min() < 1.001 * feps                        # 1.00016e-5
    # per-row eps: row 304 alone
    eps = np.full(a.size, -1.0)
    eps[304] = 1e-3
    one = mcr.coarsen(fine, eps)
    coarse = mrr.built("edges", 1e-3)
    assert all(one.rows[i] is fine.rows[i] for i in range(a.size) if i != 304)
    assert np.array_equal(one.rows[304].x, coarse.rows[304].x) and np.array_equal(one.rows[304].cum, coarse.rows[304].cum)


@pytest.mark.parametrize("K", BUDGETS)
def test_budget_on_edges(K):
    integrand, a, b, theta, feps, fine = mbr.case("edges")
    assert (a[304], b[304]) == (0.0, 5.0) and fine.accepted[304] == 15573
    thr = mcr.thresholds(fine)
    eps = mcr.budget_eps(fine, K)
    got = mcr.coarsen(fine, eps)
    for i in range(a.size):
        L = int(fine.accepted[i])
        assert got.accepted[i] <= max(K, 0) or L <= K
        if L <= K:
            assert eps[i] == -1.0 and got.rows[i] is fine.rows[i]
            continue
        o0, o1 = int(fine.offsets[i]), int(fine.offsets[i + 1])
        t = np.sort(thr[o0 + 2:o1 - 1:2])[::-1]                        # descending
        assert eps[i] == t[K - 1] and got.accepted[i] == 1 + int((t > eps[i]).sum()) <= K
        if K == 1 or t[K - 1] != t[K - 2]:
            assert got.accepted[i] == K
    assert got.accepted[304] == K
    want = {1: 3.79e7, 2: 1.87e7, 64: 156.07, 257: 2.2749}[K]
    assert abs(eps[304] - want) <= 5e-3 * want
    row = mbr.fixed_batch(integrand, a[304:305], b[304:305], float(eps[304])).rows[0]
    for k in ("x", "f", "cum", "level"):
        assert np.array_equal(getattr(got.rows[304], k), getattr(row, k)), k


def test_comb_is_a_deep_row_at_an_odd_offset():
    batch = mcr.comb()
    row = batch.rows[1]
    assert batch.offsets[1] % 2 == 1 and row.accepted == mcr.COMB_DEPTH + 1 and row.levels == mcr.COMB_DEPTH + 1
    assert row.levels > 96 and np.array_equal(row.x[::2][:3], [0.0, 2.0 ** -100, 2.0 ** -99])
    t = mcr.tree(batch, 1)
    assert t.d.size == mcr.COMB_DEPTH and np.all(t.start == 0)        # a chain of nodes [0, 2^-k]
    o0, o1 = int(batch.offsets[1]), int(batch.offsets[2])
    thr = mcr.thresholds(batch)[o0 + 2:o1 - 1:2]
    assert np.all(np.diff(thr) > 0)                                    # distinct: every leaf count 1 .. 101 is some eps's
    for cut in (3, 37, 64, 99):                                        # positions below and above bit 64
        e = 0.5 * (thr[cut - 1] + thr[cut])
        assert thr[cut - 1] < e < thr[cut]
        assert mcr.coarsen(batch, e).accepted[1] == 1 + (mcr.COMB_DEPTH - cut)
    assert mcr.coarsen(batch, thr[50]).accepted[1] == mcr.COMB_DEPTH - 50     # the strict >: the node AT eps merges
