"""The ring at its capacity line (aq_ring_window.h): whole trees on one or two workgroups.

A wave's ring reaches its spill line only when the wave owns a deep subtree, so these runs set a small grid
(AQ_GRID): twelve or twenty-four waves carry a whole tree, every wave's ring runs at its line for most of its
life and its cellar goes as deep as it ever does. An over-full ring wraps modulo WCAP and overwrites live
pairs: that shows as wrong counts, so every case checks the exact tree. The diagnostics (DIAG instances)
add that the cellar really ran (cellar_out: pairs spilled to the waves' cellars) and how far S = ring + held
went (max_ring: S at a round's start, at most the line <= WCAP; the issue's bound is WCAP + 63).

(chunks_out counts chunks published to the HBM queue for OTHER workgroups waiting on it: one workgroup
alone never publishes one, so the cellar's own counter is the one asserted; chunks_out is printed.)
"""
import json
import math
import os
from decimal import Decimal

import numpy as np
import pytest

import err_reference as er

pytestmark = pytest.mark.gpu

COSH4, SIN_RECIP = 0, 1
WCAP = 256
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def trees():
    with open(os.path.join(HERE, "golden", "trees.json")) as f:
        return json.load(f)


def _small_grid_ctx(monkeypatch, grid, diag=True):
    from ppls_amd import Context
    monkeypatch.setenv("AQ_GRID", str(grid))
    c = Context(0)
    c.set_level_histograms(False)   # the plain / DIAG instances (per-burst depth cap), not the histogram one
    if diag:
        c.set_diagnostics(True)
    return c


def _check_tree(r, g, what):
    assert (r.tasks, r.accepted, r.levels) == (g["tasks"], g["leaves"], g["levels"]), (what, r)
    want = Decimal(g["area_quad"])
    rel = abs((Decimal(r.area) - want) / want) if want else abs(Decimal(r.area))
    print(what, "area", r.area, "rel dev", float(rel))
    assert rel <= Decimal("1e-12"), (what, r.area, g["area_quad"])


def _check_diag(c, what, grid):
    d, names = c.diagnostics()
    col = dict(zip(names, d.T))
    fig = {k: int(col[k].sum()) for k in ("cellar_out", "cellar_in", "prefetch", "chunks_out", "pool_push", "rounds")}
    fig["max_ring"] = int(col["max_ring"].max())
    fig["max_cellar"] = int(col["max_cellar"].max())
    print(what, fig)
    assert d.shape[0] == grid
    assert fig["max_ring"] <= WCAP + 63, (what, fig)
    assert fig["cellar_out"] > 0, (what, fig)
    # every pair that went down came back up: as a refill or as a landed prefetch
    assert fig["cellar_out"] == fig["cellar_in"] + fig["prefetch"], (what, fig)
    return fig


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("eps,tag,counts", [(1e-10, "cosh4_eps1e-10", (1464273, 732137)),
                                            (1e-12, "cosh4_eps1e-12", (6606491, 3303246))])
def test_cosh4_whole_tree_on_few_workgroups(trees, monkeypatch, grid, eps, tag, counts):
    """One cosh^4 [0, 5] integral on 1 and on 2 workgroups: exact counts, the golden area, no error (an error
    word raises), the cellar used. eps = 1e-12 takes the cellar deepest."""
    from ppls_amd import Problem
    g = trees[tag]
    assert (g["tasks"], g["leaves"]) == counts
    c = _small_grid_ctx(monkeypatch, grid)
    try:
        r = c.integrate(Problem(eps=eps))
        _check_tree(r, g, (tag, grid))
        _check_diag(c, (tag, grid), grid)
        if eps == 1e-10:
            # ... and as one of a few integrals of one launch (the multi-integral instance, dynamic jobs)
            c.integrate_many_async(np.zeros(16), np.full(16, 5.0), eps, first_slot=0)
            for i in range(16):
                _check_tree(c.fetch(i), g, (tag, grid, "x16", i))
            _check_diag(c, (tag, grid, "x16"), grid)
    finally:
        c.close()


def test_sin_recip_skewed_tree_one_workgroup(trees, monkeypatch):
    """sin(1/x) on [1e-4, 1] at 1e-9: nearly all of the tree in one region, bursts cut every SKEWED_GIVE
    rounds (the burst's end, its push-back and its chunk move run most often here)."""
    from ppls_amd import Problem
    g = trees["sin_recip_eps1e-9"]
    c = _small_grid_ctx(monkeypatch, 1)
    try:
        r = c.integrate(Problem(SIN_RECIP, 1e-4, 1.0, 1e-9))
        _check_tree(r, g, "sin_recip")
        d, names = c.diagnostics()
        col = dict(zip(names, d.T))
        print("sin_recip max_ring", int(col["max_ring"].max()), "cellar_out", int(col["cellar_out"].sum()))
        assert int(col["max_ring"].max()) <= WCAP + 63
    finally:
        c.close()


def test_err_instance_one_workgroup(monkeypatch):
    """The ERR instance (8 waves, its own register budget) of the eps = 1e-10 tree on one workgroup, against the
    walker's error sums with test_gpu_err.py's bounds."""
    from ppls_amd import Problem
    w = er.lone(COSH4, 0.0, 5.0, 1e-10)
    c = _small_grid_ctx(monkeypatch, 1, diag=False)
    try:
        r = c.integrate_err(Problem(COSH4, 0.0, 5.0, 1e-10))
        assert (r.tasks, r.accepted, r.levels) == (w["tasks"], w["leaves"], w["levels"])
        assert abs(r.area - w["area"]) <= math.ulp(w["area"]), (r.area.hex(), w["area"].hex())
        t = er.tol(w)
        print("err_abs", r.err_abs, w["err_abs"], "err_signed", r.err_signed, w["err_signed"], "tol", t)
        assert abs(r.err_abs - w["err_abs"]) <= t
        assert abs(r.err_signed - w["err_signed"]) <= t
    finally:
        c.close()


def test_depth_cap_drops_a_full_ring(trees, monkeypatch):
    """max_depth three levels short of the tree's on one workgroup: the waves hit the cap with their rings at
    the line and their cellars in use, drop both, and report AQ_EDEPTH; the next launches on the same context
    are exact -- nothing of the dropped rings, cellars or prefetches is left behind."""
    from ppls_amd import AquadError, Problem
    g = trees["cosh4_eps1e-10"]
    c = _small_grid_ctx(monkeypatch, 1)
    try:
        with pytest.raises(AquadError, match="depth") as e:
            c.integrate(Problem(eps=1e-10, max_depth=g["levels"] - 3))
        assert e.value.code == -5
        _check_tree(c.integrate(Problem(eps=1e-10)), g, "after the capped lone launch")
        c.integrate_many_async(np.zeros(4), np.full(4, 5.0), 1e-10, first_slot=0, max_depth=g["levels"] - 3)
        with pytest.raises(AquadError, match="depth"):
            c.fetch(0)
        c.integrate_many_async(np.zeros(4), np.full(4, 5.0), 1e-10, first_slot=0)
        for i in range(4):
            _check_tree(c.fetch(i), g, ("after the capped launch", i))
    finally:
        c.close()
