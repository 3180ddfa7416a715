"""The error estimate without a GPU: the reference walker's figures (tests/err_reference.py), the host
function aq_err_extrapolate, the _err entry points' argument checks, and the launch plan's ERR flag."""
import ctypes
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

import err_reference as er
from conftest import ROOT

COSH4, SIN_RECIP, USER, PARAM = 0, 1, 2, 3
EXACT = er.cosh4_exact(5.0)


@pytest.fixture(scope="module")
def lib():
    from ppls_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("eps,tasks", [(1e-3, 6567), (1e-6, 68135), (1e-10, 1464273)])
def test_walker_cosh4_rows(oracle, trees, eps, tasks):
    """cosh^4 on [0, 5]: the golden task count; EPSILON does not bound the area's error, err_abs does, and the
    extrapolated area is closer to the integral than the area."""
    w = er.lone(COSH4, 0.0, 5.0, eps)
    assert w["tasks"] == tasks
    err = abs(w["area"] - EXACT)
    assert err > eps                                     # what the caller is not told today
    assert err <= w["err_abs"]
    assert w["err_signed"] == -w["err_abs"]              # cosh^4 is convex: every d has one sign
    assert abs(w["area"] + w["err_signed"] / 3.0 - EXACT) < err
    # the sums the feature's proposal tabulates, to their printed digits
    printed, half_unit = {1e-3: (1.3199562, 5e-8), 1e-6: (1.2583e-2, 5e-7), 1e-10: (2.6497e-5, 5e-10)}[eps]
    assert abs(w["err_abs"] - printed) <= half_unit
    g = trees[{1e-3: "cosh4_eps1e-3", 1e-6: "cosh4_eps1e-6", 1e-10: "cosh4_eps1e-10"}[eps]]
    assert (w["tasks"], w["leaves"], w["levels"]) == (g["tasks"], g["leaves"], g["levels"])


def test_walker_sin_recip_row(oracle):
    """sin(1/x) on [1e-4, 1] at 1e-9: mixed signs, err_abs about 50 x |err_signed|."""
    w = er.lone(SIN_RECIP, 1e-4, 1.0, 1e-9)
    assert w["tasks"] == 56357
    assert w["err_signed"] > 0.0 and 30.0 < w["err_abs"] / w["err_signed"] < 70.0
    assert abs(w["err_signed"] - 2.04e-7) <= 0.005e-7 and abs(w["err_abs"] - 1.036e-5) <= 0.0005e-5


def test_walker_equals_the_param_walker(oracle):
    """The same counts and areas as tests/param_reference.py on its draw (the walk this one extends)."""
    import param_reference as pr
    a, b, theta, w = er.draw_reference()
    _, _, _, w0 = pr.draw_reference()
    for k in ("tasks", "leaves", "levels"):
        assert np.array_equal(w[k], w0[k]), k
    assert np.array_equal(w["area"], w0["area"])
    assert np.all(w["err_abs"] >= np.abs(w["err_signed"])) and np.all(w["err_abs"] > 0.0)


def test_extrapolate_is_host_code(lib):
    from ppls_amd import _lib
    rng = np.random.default_rng(3)
    for area, sg in zip(rng.normal(size=200) * 10.0 ** rng.uniform(-8, 8, 200), rng.normal(size=200) * 1e-3):
        e = _lib.aq_err(abs(sg), sg)
        assert lib.aq_err_extrapolate(float(area), ctypes.byref(e)) == float(area) + float(sg) / 3.0
    e = _lib.aq_err(2.6497e-5, -2.6497e-5)
    assert lib.aq_err_extrapolate(1.0, ctypes.byref(e)) == 1.0 + (-2.6497e-5) / 3.0


def test_null_and_mismatched_arguments_are_rejected_without_a_gpu(lib):
    """NULL context, problem or outputs, and a theta that does not go with the integrand, are AQ_EINVAL
    before any device call (as test_null_arguments_are_rejected_without_a_gpu for the _params calls)."""
    from ppls_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    one = (ctypes.c_double * 2)(0.0, 1.0)
    th = ctypes.cast(one, dp)
    r, e = _lib.aq_result(), _lib.aq_err()
    p = _lib.aq_problem(COSH4, 0, 0.0, 5.0, 1e-3, 0, 0)
    q = _lib.aq_problem(PARAM, 0, 0.0, 5.0, 1e-3, 0, 0)
    fake = ctypes.c_void_p(1)   # never dereferenced: every call below fails its argument checks first
    assert lib.aq_integrate_err(None, ctypes.byref(p), None, ctypes.byref(r), ctypes.byref(e)) == -1
    assert lib.aq_integrate_err(fake, None, None, ctypes.byref(r), ctypes.byref(e)) == -1
    assert lib.aq_integrate_err(fake, ctypes.byref(p), None, None, ctypes.byref(e)) == -1
    assert lib.aq_integrate_err(fake, ctypes.byref(p), None, ctypes.byref(r), None) == -1
    assert lib.aq_integrate_err(fake, ctypes.byref(p), th, ctypes.byref(r), ctypes.byref(e)) == -1   # theta, not PARAM
    assert lib.aq_integrate_err(fake, ctypes.byref(q), None, ctypes.byref(r), ctypes.byref(e)) == -1  # PARAM, no theta
    assert lib.aq_integrate_many_err_async(None, COSH4, 1, th, th, None, 1e-3, 0, 0, 1, 0) == -1
    assert lib.aq_integrate_many_err_async(fake, COSH4, 1, None, th, None, 1e-3, 0, 0, 1, 0) == -1
    assert lib.aq_integrate_many_err_async(fake, COSH4, 1, th, th, th, 1e-3, 0, 0, 1, 0) == -1
    assert lib.aq_integrate_many_err_async(fake, PARAM, 1, th, th, None, 1e-3, 0, 0, 1, 0) == -1
    assert lib.aq_integrate_many_err_async(fake, 7, 1, th, th, None, 1e-3, 0, 0, 1, 0) == -1
    assert lib.aq_fetch_err(None, 0, ctypes.byref(e)) == -1
    assert lib.aq_fetch_err(fake, 0, None) == -1
    assert lib.aq_fetch_err(fake, -1, ctypes.byref(e)) == -1
    assert lib.aq_integrate_batch_err(None, 1, th, th, None, 1e-3, COSH4, None, None, None, None, None) == -1
    assert lib.aq_integrate_batch_err(fake, 1, th, th, th, 1e-3, COSH4, None, None, None, None, None) == -1
    assert lib.aq_integrate_batch_err(fake, 1, th, th, None, 1e-3, PARAM, None, None, None, None, None) == -1
    assert lib.aq_integrate_batch_err(fake, 1, None, th, None, 1e-3, COSH4, None, None, None, None, None) == -1


def test_python_theta_checks_need_no_library_call():
    """A theta of the wrong shape, a theta without PARAM and PARAM without theta raise ValueError before
    the library is called (the methods are called on a context object that was never created)."""
    from ppls_amd import Context, Problem
    c = Context.__new__(Context)
    c.L, c._h = None, ctypes.c_void_p()
    one = np.array([0.0]), np.array([1.0])
    for call in (lambda: c.integrate_err(Problem(PARAM, 0.0, 1.0, 1e-3), [0.0, 1.0, 2.0]),
                 lambda: c.integrate_err(Problem(PARAM, 0.0, 1.0, 1e-3)),
                 lambda: c.integrate_err(Problem(COSH4, 0.0, 1.0, 1e-3), [0.0, 1.0]),
                 lambda: c.integrate_many_err_async(*one, 1e-3, integrand=PARAM, theta=[[0.0]]),
                 lambda: c.integrate_many_err_async(*one, 1e-3, theta=[[0.0, 1.0]]),
                 lambda: c.integrate_batch_err(*one, 1e-3, integrand=PARAM, theta=[[0.0, 1.0], [0.0, 1.0]]),
                 lambda: c.integrate_batch_err(*one, 1e-3, integrand=PARAM)):
        with pytest.raises(ValueError):
            call()


def test_result_fields_default_to_none():
    from ppls_amd.aquad import Result
    r = Result(1.0, 1, 1, 1, 0)
    assert (r.err_abs, r.err_signed, r.area_extrapolated) == (None, None, None)


PLAN_SRC = textwrap.dedent("""
    #include <cstdio>
    #include <cstring>
    #include "aq_launch_plan.h"
    using namespace aq;
    static bool same_hint(const HintState& x, const HintState& y) {
        return x.valid == y.valid && x.preset == y.preset && x.per_ok == y.per_ok && x.fid == y.fid &&
               x.nshards == y.nshards && x.eps == y.eps;
    }
    static bool same_plan(const LaunchPlan& x, const LaunchPlan& y) {
        return x.rc == y.rc && x.variant == y.variant && x.nwt == y.nwt && x.shares == y.shares && x.D == y.D &&
               x.tail_from == y.tail_from && x.tail_mult == y.tail_mult && x.per_cu == y.per_cu &&
               x.static_jobs == y.static_jobs && x.adaptive == y.adaptive && same_hint(x.hint, y.hint);
    }
    int main() {
        const int ks[] = {1, 2, 11, 12, 15, 16, 17, 63, 64, 300, 3071, 3072, 5000, 32768, 262144};
        long n = 0, bad = 0;
        for (int fid = 0; fid < 4; ++fid)
        for (int k : ks)
        for (int nshards : {1, 2, 3, 8})
        for (int diag = 0; diag < 2; ++diag)
        for (int heap = 0; heap < 2; ++heap)
        for (int first : {0, 20, NPARTS, SYNC_SLOT})
        for (int hv = 0; hv < 2; ++hv) {
            LaunchRequest omitted;   // a request that never names the ERR flag
            omitted.fid = fid; omitted.grid = 256; omitted.k = k; omitted.nshards = nshards; omitted.first_slot = first;
            omitted.diag = diag != 0; omitted.batch_heap = heap != 0; omitted.eps = 1e-10;
            LaunchRequest off = omitted;
            off.err = false;
            LaunchRequest on = omitted;
            on.err = true;
            HintState h;
            h.valid = hv != 0; h.fid = fid; h.nshards = nshards; h.eps = 1e-10; h.per_ok = hv != 0;
            const LaunchPlan p0 = plan_launch(omitted, h), p1 = plan_launch(off, h), p2 = plan_launch(on, h);
            ++n;
            if (!same_plan(p0, p1) || p0.err || p1.err) ++bad;
            // an ERR plan: ERR_NW waves whatever the shape, no DIAG variant, the flag carried
            if (p2.rc == 0 && (!p2.err || p2.nwt != ERR_NW || p2.variant == Variant::DIAG || p2.variant == Variant::DIAG_PCU))
                ++bad;
            if (p2.rc == 0 && p2.per_cu != p0.per_cu) ++bad;
        }
        std::printf("%ld %ld %d\\n", n, bad, ERR_NW);
        return bad != 0;
    }
""")


def test_launch_plan_flag_false_is_the_plan_of_today(tmp_path):
    """plan_launch built alone with g++: a request with the ERR flag false plans exactly what a request that
    omits the flag does (which tests/golden/launch_plans.json pins row by row), over every launch shape; with
    the flag set every plan runs ERR_NW waves per workgroup and no diagnostics instance."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "plan_err.cpp"
    src.write_text(PLAN_SRC)
    exe = str(tmp_path / "plan_err")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ppls_amd", "csrc"), "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    n, bad, nw = (int(v) for v in r.stdout.split())
    assert r.returncode == 0 and bad == 0 and n == 4 * 15 * 4 * 2 * 2 * 4 * 2 and nw == 8
