"""Mesh refinement without a GPU: the two functions declared, bound, exported and refusing a NULL context on the
host; and the CPU reference (tests/mesh_refine_reference.py), which the GPU tests compare with bit for bit, checked
for the identity the feature rests on -- a mesh continued from a coarser eps IS the mesh built from the roots at the
finer one -- and for the shapes the GPU cases rely on. (On the GPU: tests/test_gpu_mesh_refine.py.)"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import mesh_batch_reference as mbr
import mesh_refine_reference as mrr
import param_reference as pr
import tol_reference as tr

AQ_EINVAL = -1
NAMES = ("aq_mesh_refine_batch", "aq_mesh_err_batch")


def test_declared_bound_exported_and_null_context_refused():
    from test_abi import header_functions
    from ppls_amd import _lib
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aq_[a-z0-9_]+)$", out, flags=re.M))
    for name in NAMES:
        assert name in header_functions() and name in _lib.EXPORTS and name in exported
        assert getattr(lib, name).restype is ctypes.c_int
    io, info = _lib.aq_mesh_batch_io(), _lib.aq_mesh_refine_info()
    # (never dereferenced: the context comes first)
    assert lib.aq_mesh_refine_batch(None, 1, 8, 8, 8, 8, None, None, 1e-3, 0, ctypes.byref(io), 16, 4, 16,
                                    ctypes.byref(info)) == AQ_EINVAL
    assert lib.aq_mesh_refine_batch(None, 0, None, None, None, None, None, None, 1e-3, 0, ctypes.byref(io), 16, 4, 16,
                                    ctypes.byref(info)) == AQ_EINVAL
    assert lib.aq_mesh_err_batch(None, 1, 8, 8, 8, 8, 8) == AQ_EINVAL
    assert lib.aq_mesh_err_batch(None, 0, None, None, None, None, None) == AQ_EINVAL
    # the structure is the header's: five uint64 and two uint32
    assert ctypes.sizeof(_lib.aq_mesh_refine_info) == 48


@pytest.mark.parametrize("name", ["edges", "param", "sin", "scale"])
def test_a_continued_mesh_is_the_mesh_built_at_the_finer_eps(name):
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case(name)
    assert feps < ceps and mrr.same_mesh(rf.batch, fine)          # cum included: the same leaves, the same Fractions
    assert rf.batch.leaves == fine.leaves and rf.batch.levels == fine.levels
    assert rf.evaluated == fine.tasks_total - coarse.tasks_total
    # the survivors, and the leaves of the 2 * reseeded subtrees the run walked (a binary tree of t tasks has
    # (t + 1) / 2 leaves)
    assert fine.leaves == (coarse.leaves - rf.reseeded) + (rf.evaluated + 2 * rf.reseeded) // 2
    # nothing fails at the input's own eps, or above it
    for eps in (ceps, 2 * ceps):
        same = mrr.refine(coarse, integrand, theta, eps)
        assert (same.reseeded, same.evaluated, same.seed_depths, same.changed) == (0, 0, [], [])
        assert mrr.same_mesh(same.batch, coarse)


def test_the_shapes_of_the_cases():
    _, a, _, _, ceps, feps, coarse, fine, rf = mrr.case("edges")
    assert (ceps, feps) == (1e-3, 1e-5)
    assert (rf.reseeded, len(rf.seed_depths), rf.changed, rf.widest_level, rf.evaluated) == (
        3595, 12, [300, 304, 305, 306], 7790, 26902)
    assert np.all(coarse.accepted[:300] == 1) and np.all(fine.accepted[:300] == 1) and a.size == 307
    # seeds arrive at levels the run has already begun, and a level takes several 1024-record chunks
    assert rf.seed_depths[0] == 2 and rf.seed_depths[-1] == 15 and rf.widest_level > 7 * 1024
    assert max(rf.level_records) + 1 == fine.levels == 18
    _, _, _, _, ceps, feps, coarse, fine, rf = mrr.case("param")
    assert (ceps, feps) == (6.4e-5, 1e-6) and ceps == pr.DRAW_EPS * 64
    assert (rf.reseeded, coarse.leaves, len(rf.changed), rf.widest_level, rf.evaluated) == (2902, 2904, 64, 6242, 17384)
    _, _, _, _, ceps, feps, coarse, fine, rf = mrr.case("sin")
    assert (ceps, feps) == (1e-3, 1e-5) and len(rf.seed_depths) == 10
    assert len(set(fine.rows[0].level.tolist())) >= 10            # a skewed tree: leaves on many depths
    _, _, _, _, ceps, feps, coarse, fine, rf = mrr.case("scale")
    assert (ceps, feps) == (1e166, 1e163) and rf.changed == [0] and fine.area[0] > 1e170


def test_a_mask_keeps_the_other_rows():
    integrand, a, b, theta, ceps, feps, coarse, fine, rf = mrr.case("edges")
    active = np.zeros(a.size, bool)
    active[304] = True
    one = mrr.refine(coarse, integrand, theta, feps, active=active)
    assert one.changed == [304] and one.batch.rows[304].accepted == fine.rows[304].accepted
    assert np.array_equal(one.batch.rows[304].x, fine.rows[304].x) and np.array_equal(one.batch.rows[304].cum, fine.rows[304].cum)
    assert all(one.batch.rows[i] is coarse.rows[i] for i in range(a.size) if i != 304)
    assert one.evaluated == one.batch.tasks_total - coarse.tasks_total
    # two hops equal one
    first = mrr.built("edges", mrr.EDGES_FIRST)
    hop1 = mrr.refine(first, integrand, theta, ceps)
    hop2 = mrr.refine(hop1.batch, integrand, theta, feps)
    assert mrr.same_mesh(hop1.batch, coarse) and mrr.same_mesh(hop2.batch, fine)
    assert hop1.evaluated + hop2.evaluated == fine.tasks_total - first.tasks_total


def test_error_sums_from_the_mesh_are_the_walkers():
    from oracle import pyoracle
    import err_reference as er
    integrand, a, b, theta, eps, ref = mbr.case("sin")
    w = er.walk(a, b, eps, integrand, pyoracle)
    ea, es = mrr.err_sums(ref)
    assert np.array_equal(ea, w["err_abs"]) and np.array_equal(es, w["err_signed"])
    assert np.array_equal(mrr.area_sums(ref), w["area"])
    _, _, _, _, _, edges = mbr.case("edges")
    exact = mrr.err_exact(edges)
    assert [e[0] is None for e in exact[300:]] == [False, False, True, True, False, False, False]
    assert np.isnan(mrr.err_sums(edges)[0][302])


def _sets():
    a, b, ref = tr.set_c(n=64)
    k = tr.SET_C
    yield 0, a, b, None, k, ref
    k = tr.SET_P
    a, b, theta = pr.draw(64)
    yield mbr.PARAM, a, b, theta, k, tr.run(a, b, mbr.PARAM, k["epsabs"], k["epsrel"], k["eps0"], k["shrink"],
                                            k["max_rounds"], theta)


def test_the_tolerance_loop_over_continued_meshes_is_the_round_by_round_walk():
    for integrand, a, b, theta, k, ref in _sets():
        assert ref["ratio_min"] >= tr.SAFE                        # before any decision is relied on
        if integrand == mbr.PARAM:
            first = mbr.Batch(mbr.param_rows(a, b, theta, k["eps0"]))
        else:
            first = mbr.fixed_batch(integrand, a, b, k["eps0"])
        rounds, eps_used, final, evaluated = mrr.tol_loop(first, integrand, theta, k["epsabs"], k["epsrel"], k["eps0"],
                                                          k["shrink"], k["max_rounds"])
        assert np.array_equal(rounds, ref["rounds"]) and np.array_equal(eps_used, ref["eps_used"])
        assert np.array_equal(final.tasks, ref["tasks"]) and np.array_equal(final.accepted, ref["leaves"])
        assert evaluated == int(ref["tasks"].sum())               # every task of the final trees exactly once
        assert len(set(np.abs(rounds).tolist())) > 2              # rows retire in different rounds
