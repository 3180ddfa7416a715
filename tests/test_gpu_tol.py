"""The tolerance-driven batch on the GPU (aq_integrate_batch_tol) against tests/tol_reference.py, the walker of
tests/err_reference.py driven round by round with the call's schedule and criterion -- never against the
library's own _err call.

rounds and eps_used must be equal, tasks and accepted exact, an area within 1 ulp of the walker's math.fsum, both
sums within err_reference.tol of the walker's. The device's err_abs and area differ from the walker's by at most
slack = tol + epsrel * ulp(|area|), so a round's decision is the walker's whenever the walker's err_abs is further
than that from the target: every test first asserts, from the walker, that EVERY decision of its run has
margin >= 16 * slack, and leaves out no integral."""
import ctypes
import subprocess

import numpy as np
import pytest

import err_reference as er
import tol_reference as tr

pytestmark = pytest.mark.gpu

COSH4, SIN_RECIP, USER, PARAM = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


def _check(res, ref, what):
    """A call's seven arrays against a reference run, every integral."""
    assert ref["ratio_min"] >= tr.SAFE, (what, ref["ratio_min"])   # the condition: no decision within 16 x slack
    area, tasks, acc, err_abs, err_signed, eps_used, rounds = res
    n = ref["rounds"].size
    assert all(x.shape == (n,) for x in res), what
    assert np.array_equal(rounds, ref["rounds"]), (what, np.nonzero(rounds != ref["rounds"])[0][:8])
    assert np.array_equal(eps_used, ref["eps_used"]), what
    bad = np.nonzero((tasks.astype(np.int64) != ref["tasks"]) | (acc.astype(np.int64) != ref["leaves"]))[0]
    assert bad.size == 0, (what, [(int(i), int(tasks[i]), int(ref["tasks"][i])) for i in bad[:8]], bad.size)
    off = np.nonzero(np.abs(area - ref["area"]) > np.spacing(np.abs(ref["area"])))[0]
    assert off.size == 0, (what, [(int(i), float(area[i]).hex(), float(ref["area"][i]).hex()) for i in off[:8]])
    t = tr.row_tol(ref)
    for name, got in (("err_abs", err_abs), ("err_signed", err_signed)):
        dev = np.abs(got - ref[name])
        if n:
            print(what, name, "worst deviation / tol", float(np.max(dev / t)))
        off = np.nonzero(dev > t)[0]
        assert off.size == 0, (what, name, [(int(i), float(got[i]), float(ref[name][i]), float(t[i])) for i in off[:8]])


def _run(ctx, a, b, k, integrand=COSH4, theta=None, max_rounds=None):
    return ctx.integrate_batch_tol(a, b, epsabs=k["epsabs"], epsrel=k["epsrel"], eps0=k["eps0"], shrink=k["shrink"],
                                   max_rounds=max_rounds or k["max_rounds"], integrand=integrand, theta=theta)


def test_set_p(ctx):
    """600 parametrised integrals, all live for five rounds, retiring in rounds 5, 6 and 7; all converge."""
    a, b, theta, ref = tr.set_p()
    assert ref["live"] == [600, 600, 600, 600, 600, 405, 85]
    res = _run(ctx, a, b, tr.SET_P, PARAM, theta)
    assert res.converged
    _check(res, ref, "set P")


def test_set_c_reports_the_unconverged(ctx):
    """300 cosh^4 integrals retiring from round 1 on; 23 miss the tolerance in 7 rounds: no exception, the flag,
    rounds == -7 and the round-7 values for those."""
    a, b, ref = tr.set_c()
    assert int(np.sum(ref["rounds"] == -7)) == 23 and ref["live"][-1] == 66
    res = _run(ctx, a, b, tr.SET_C)
    assert not res.converged
    _check(res, ref, "set C")
    assert int(np.sum(res[6] == -7)) == 23
    # the raw return code
    from ppls_amd import _lib
    t = _lib.aq_tol(1e-6, 1e-6, 1e-2, 8.0, 7, 0)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = ctx.L.aq_integrate_batch_tol(ctx._h, a.size, a.ctypes.data_as(dp), b.ctypes.data_as(dp), None, COSH4,
                                      ctypes.byref(t), None, None, None, None, None, None, None)
    assert rc == _lib.AQ_ENOCONV == -10


def test_small_launches(ctx):
    """Set C's first 40 integrals with up to 9 rounds: the live counts pass through launches of 12 to 63 integrals
    and of fewer than 12, whose bounds the host rebuilds from the survivors' indices (kernel arguments)."""
    a, b, ref = tr.set_c(40, 9)
    assert any(12 <= k <= 63 for k in ref["live"][1:]) and any(1 <= k <= 11 for k in ref["live"][1:]), ref["live"]
    res = _run(ctx, a, b, tr.SET_C, max_rounds=9)
    assert res.converged and np.all(ref["rounds"] > 0)
    _check(res, ref, "first 40 of set C")
    # only some outputs asked for
    from ppls_amd import _lib
    t = _lib.aq_tol(1e-6, 1e-6, 1e-2, 8.0, 9, 0)
    dp = ctypes.POINTER(ctypes.c_double)
    rounds = np.zeros(40, np.int32)
    acc = np.zeros(40, np.uint64)
    rc = ctx.L.aq_integrate_batch_tol(ctx._h, 40, a.ctypes.data_as(dp), b.ctypes.data_as(dp), None, COSH4,
                                      ctypes.byref(t), None, acc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None,
                                      None, None, None, rounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == 0 and np.array_equal(rounds, ref["rounds"]) and np.array_equal(acc.astype(np.int64), ref["leaves"])


def test_one_and_none(ctx):
    """n = 1 (a per-CU launch from the first round on) and n = 0."""
    a, b, ref = tr.set_c(1, 9)
    res = _run(ctx, a, b, tr.SET_C, max_rounds=9)
    assert res.converged
    _check(res, ref, "n = 1")
    res = ctx.integrate_batch_tol(np.zeros(0), np.zeros(0), epsrel=1e-6)
    assert res.converged and len(res) == 7 and all(x.size == 0 for x in res)


def test_blocks(ctx, monkeypatch):
    """Set P in blocks of 256, 256 and 88 (AQ_TOL_BLOCK): the reference's results, and the one-block run's."""
    a, b, theta, ref = tr.set_p()
    whole = _run(ctx, a, b, tr.SET_P, PARAM, theta)
    monkeypatch.setenv("AQ_TOL_BLOCK", "256")
    res = _run(ctx, a, b, tr.SET_P, PARAM, theta)
    monkeypatch.delenv("AQ_TOL_BLOCK")
    assert res.converged
    _check(res, ref, "set P in blocks of 256")
    for i in (1, 2, 5, 6):   # tasks, accepted, eps_used, rounds
        assert np.array_equal(res[i], whole[i]), i


def test_lone_sin_recip(ctx):
    """sin(1/x) on [1e-4, 1] to epsabs = 1e-6: ten rounds of one integral; the signs are mixed, so err_abs is far
    above |err_signed| and a criterion on the signed sum would stop rounds earlier."""
    ref = tr.lone(SIN_RECIP, 1e-4, 1.0, 1e-6, 0.0, 1e-3)
    assert ref["rounds"][0] == 10 and ref["err_abs"][0] > 30.0 * abs(ref["err_signed"][0])
    res = ctx.integrate_batch_tol([1e-4], [1.0], epsabs=1e-6, eps0=1e-3, integrand=SIN_RECIP)
    assert res.converged
    _check(res, ref, "sin_recip")


def test_state_after_the_call(ctx, trees):
    """The call leaves its slots clean: a plain launch into slots 0..15 gives the golden counts and is no _err
    launch. A context's device memory moves with its first _tol call only, by the block's buffers."""
    from ppls_amd import AquadError, Context, Problem
    a, b, ref = tr.set_c(40, 9)
    _run(ctx, a, b, tr.SET_C, max_rounds=9)
    g = trees["cosh4_eps1e-3"]
    ctx.integrate_many_async(np.zeros(16), np.full(16, 5.0), 1e-3, first_slot=0)
    for i in range(16):
        r = ctx.fetch(i)
        assert (r.tasks, r.accepted) == (g["tasks"], g["leaves"]), i
    with pytest.raises(AquadError) as e:
        ctx.fetch_err(0)
    assert e.value.code == -1
    with Context(0) as c, Context(0) as d:
        fresh = d.device_bytes
        c.integrate(Problem(eps=1e-3))
        c.integrate_many_async(np.zeros(4), np.full(4, 5.0), 1e-3, first_slot=0)
        c.synchronize()
        assert c.device_bytes == fresh
        res = _run(c, a, b, tr.SET_C, max_rounds=9)
        assert np.array_equal(res[6], ref["rounds"])
        # the slots' error sums (the first ERR launch's), and per row of the 40: two halves of bounds and indices,
        # the gathered rows {4} and {2}, a flag, the 8-double record; a count and a task sum per 256 rows
        held = c.device_bytes
        assert held == fresh + 16 * (c.async_slots + 1) + 40 * (2 * 16 + 2 * 4 + 32 + 16 + 1 + 64) + 4 + 8
        _run(c, a, b, tr.SET_C, max_rounds=9)
        assert c.device_bytes == held


def test_cli_tol(trees):
    """`aquad --epsrel R`: the reference's printout of the retiring round, the two --err lines, and the round."""
    from ppls_amd import build
    for epsrel, want_round in ((1e-6, 1), (1e-9, 5)):
        ref = tr.lone(COSH4, 0.0, 5.0, 0.0, epsrel, 1e-3)
        assert ref["ratio_min"] >= tr.SAFE and ref["rounds"][0] == want_round
        out = subprocess.run([build.CLI, "--epsrel", repr(epsrel)], capture_output=True, text=True, timeout=120,
                             check=True).stdout
        lines = out.splitlines()
        assert len(lines) == 8, out
        assert lines[0] == "Area=%f" % ref["area"][0]
        assert lines[2] == "Tasks Per Process" and lines[3] == "0\t1\t"
        assert [int(v) for v in lines[4].split()] == [0, int(ref["tasks"][0])]
        assert lines[5] == "Error estimate=%.6e" % ref["err_abs"][0]
        ext = float(lines[6].split("=")[1])
        want = ref["area"][0] + ref["err_signed"][0] / 3.0
        assert lines[6].startswith("Extrapolated area=")
        assert abs(ext - want) <= 2.0 * np.spacing(want) + tr.row_tol(ref)[0] / 3.0
        assert lines[7] == "Rounds=%d eps=%.17g" % (want_round, ref["eps_used"][0])
    assert lines[0] != "Area=" + trees["cosh4_eps1e-3"]["reference"]["area_printed"]   # (round 5 is not round 1's area)
    p = subprocess.run([build.CLI, "--epsrel", "1e-6", "--levels"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and p.stdout == ""
    p = subprocess.run([build.CLI, "--epsabs", "1e-6", "--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and p.stdout == ""
