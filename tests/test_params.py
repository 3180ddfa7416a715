"""Per-integral parameters (AQ_F_PARAM) without a GPU: the reference walker the GPU tests check against
(tests/param_reference.py) is itself checked against reference-pinned data, and the new entry points'
host-side surface (argument validation, the compiled-in family)."""
import ctypes
import math

import numpy as np
import pytest

import param_reference as pr


@pytest.fixture(scope="module")
def lib():
    from ppls_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", ["gauss_eps1e-10", "gauss_eps1e-13"])
def test_walker_at_unit_theta_is_the_oracle_user_tree(oracle, trees, name):
    """theta = {0, 1}: (x - 0) * 1 is exact, so the walk is the AQ_F_USER Gaussian's tree -- the oracle's
    (tasks, leaves, levels, both histograms, the area to the last bit) and the golden file's, whose
    totals the reference binary built with that F printed."""
    g = trees[name]
    o = oracle.integrate(oracle.USER, g["a"], g["b"], g["eps"])
    w = pr.walk_one(g["a"], g["b"], 0.0, 1.0, g["eps"], oracle)
    assert (w["tasks"], w["leaves"], w["levels"]) == (o.tasks, o.leaves, o.levels) == (g["tasks"], g["leaves"], g["levels"])
    assert w["tasks_per_level"] == o.tasks_per_level == g["tasks_per_level"]
    assert w["leaves_per_level"] == o.leaves_per_level == g["leaves_per_level"]
    assert w["area"] == o.area == float(g["area_quad"])
    assert w["tasks"] == g["reference"]["tasks_total"]
    assert "%f" % w["area"] == g["reference"]["area_printed"]


def test_walker_trees_of_the_gpu_tests(oracle):
    """The lone trees the GPU tests run: their sizes as first measured with this walker, so a change of
    the walker or the oracle that moves them shows here, without a GPU."""
    w = pr.tree_reference(pr.TREE_SHIFTED)
    assert (w["tasks"], w["levels"]) == (42637, 17)
    w = pr.tree_reference(pr.TREE_WIDE_256)
    assert (w["tasks"], w["levels"]) == (196795, 19)
    w = pr.tree_reference(pr.TREE_WIDE)
    assert (w["tasks"], w["levels"]) == (197487, 31)
    for t in (pr.TREE_SHIFTED, pr.TREE_WIDE, pr.TREE_UNIT):
        w = pr.tree_reference(t)
        assert w["tasks"] == 2 * w["leaves"] - 1 and sum(w["tasks_per_level"]) == w["tasks"]


def test_walker_batch_equals_walks_of_one(oracle):
    """The batch walk keeps the integrals apart: a few of the draw, each walked alone, give the same rows;
    and the draw's neighbours really differ in size (what makes a stale theta visible)."""
    a, b, theta, w = pr.draw_reference()
    for i in (0, 1, 2, 17, 4999):
        o = pr.walk_one(a[i], b[i], theta[i, 0], theta[i, 1], pr.DRAW_EPS, oracle)
        assert (o["tasks"], o["leaves"], o["levels"]) == (w["tasks"][i], w["leaves"][i], w["levels"][i])
        assert o["area"] == w["area"][i]
    assert (w["tasks"] == 2 * w["leaves"] - 1).all()
    assert w["tasks"].min() >= 3 and w["tasks"].max() > 500 and np.unique(w["tasks"]).size > 200
    assert (w["tasks"][1:] != w["tasks"][:-1]).mean() > 0.9


def test_param_family_compiled_in(lib):
    from ppls_amd import PARAM, param_count, param_integrand_name
    from ppls_amd.aquad import INTEGRANDS
    assert lib.aq_param_count() == 2 == param_count()
    assert lib.aq_param_integrand_name().startswith(b"gauss") and param_integrand_name().startswith("gauss")
    assert PARAM == 3 == INTEGRANDS["param"]


def test_null_arguments_are_rejected_without_a_gpu(lib):
    """NULL context / arguments return AQ_EINVAL before any device call."""
    from ppls_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    x = np.zeros(2)
    xp = x.ctypes.data_as(dp)
    p = _lib.aq_problem(3, 0, 0.0, 1.0, 1e-3, 0, 0)
    r = _lib.aq_result()
    assert lib.aq_eval_integrand_params(None, 1, xp, xp, xp) == -1
    assert lib.aq_integrate_params(None, ctypes.byref(p), xp, ctypes.byref(r)) == -1
    assert lib.aq_integrate_params(None, None, None, None) == -1
    assert lib.aq_integrate_many_params_async(None, 1, xp, xp, xp, 1e-3, 0, 0, 1, 0) == -1
    assert lib.aq_integrate_batch_params(None, 1, xp, xp, xp, 1e-3, None, None, None) == -1
    assert lib.aq_integrate_batch_params(None, 1, xp, xp, None, 1e-3, None, None, None) == -1


def test_python_theta_shape_is_checked():
    """A theta array of the wrong width raises before any library call (no context needed)."""
    from ppls_amd.aquad import _theta
    assert _theta([[0.0, 1.0]], 1).shape == (1, 2) and _theta([0.0, 1.0], 1).shape == (1, 2)
    for bad, n in (([[0.0, 1.0, 2.0]], 1), ([[0.0]], 1), ([[0.0, 1.0]], 2), ([0.0, 1.0, 2.0, 3.0], 2)):
        with pytest.raises(ValueError):
            _theta(bad, n)
    assert math.isfinite(_theta(np.ones((3, 2), np.float32), 3).sum())
