"""The tolerance-driven batch (aq_integrate_batch_tol) without a GPU: the aq_tol rules and the EPSILON schedule
of ppls_amd/csrc/aq_host_args.h built alone with g++ (plain and under AddressSanitizer + UBSan), the entry
point's exports and argument checks, and the consistency of the reference the GPU tests compare against
(tests/tol_reference.py) on their two sets."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tol_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tol_args_check.cpp")
INC = [os.path.join(ROOT, "ppls_amd", "csrc"), os.path.join(ROOT, "include")]
SAN = [None, "address,undefined"]
COSH4, SIN_RECIP, USER, PARAM = 0, 1, 2, 3
MAXK = 262144


def _exe(san, tmp_path):
    exe = str(tmp_path / "tol_args_check")
    if os.path.exists(exe):
        return exe
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", INC[0], "-I", INC[1], SRC, "-o", exe]
    if san:
        cmd.insert(1, "-fsanitize=" + san)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and san:
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-400:])
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(san, tmp_path, mode, rows):
    path = tmp_path / (mode + ".txt")
    path.write_text("".join(" ".join(str(x) for x in row) + "\n" for row in rows))
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([_exe(san, tmp_path), mode, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _hex(x):
    return float(x).hex() if np.isfinite(x) else repr(float(x))


@pytest.mark.parametrize("san", SAN)
def test_tol_args(tmp_path, san):
    """tol_args_ok: a good set, each bad field, both tolerances 0, and a last round whose EPSILON is subnormal."""
    ok = dict(epsabs=0.0, epsrel=1e-6, eps0=1e-3, shrink=8.0, max_rounds=12, max_depth=0)
    nan, inf = float("nan"), float("inf")
    table = [  # (what differs from `ok`, accepted)
        ({}, 1),
        (dict(shrink=0.0, max_rounds=0), 1),                               # the defaults
        (dict(epsabs=1e-9, epsrel=0.0), 1), (dict(epsabs=1e-9), 1),
        (dict(epsabs=0.0, epsrel=0.0), 0),                                 # both tolerances 0
        (dict(epsabs=-1e-9), 0), (dict(epsabs=nan), 0), (dict(epsabs=inf), 0),
        (dict(epsrel=-1e-9), 0), (dict(epsrel=nan), 0), (dict(epsrel=inf), 0),
        (dict(eps0=0.0), 0), (dict(eps0=-1e-3), 0), (dict(eps0=nan), 0), (dict(eps0=inf), 0),
        (dict(shrink=2.0), 1), (dict(shrink=1024.0), 1), (dict(shrink=1.9999), 0), (dict(shrink=1024.5), 0),
        (dict(shrink=-8.0), 0), (dict(shrink=nan), 0), (dict(shrink=inf), 0), (dict(shrink=1.0), 0),
        (dict(max_rounds=1), 1), (dict(max_rounds=64), 1), (dict(max_rounds=65), 0), (dict(max_rounds=-1), 0),
        (dict(max_depth=127), 1), (dict(max_depth=128), 0), (dict(max_depth=-1), 0),
        # the last round's EPSILON: 1e-300 / 1024^2 is normal, 1e-300 / 1024^3 = 9.3e-310 is subnormal
        (dict(eps0=1e-300, shrink=1024.0, max_rounds=3), 1), (dict(eps0=1e-300, shrink=1024.0, max_rounds=4), 0),
        (dict(eps0=2.0 ** -1022, max_rounds=1), 1), (dict(eps0=2.0 ** -1022, shrink=2.0, max_rounds=2), 0),
        (dict(eps0=1e-3, shrink=8.0, max_rounds=64), 1),                  # 1e-3 / 8^63 = 1.3e-60
        (dict(eps0=1e-3, shrink=1024.0, max_rounds=64), 1),               # 1e-3 / 2^630
        (dict(eps0=1e-200, shrink=1024.0, max_rounds=64), 0),             # 1e-200 / 2^630 underflows to zero
        (dict(eps0=1e-300, shrink=0.0, max_rounds=0), 0),                 # ... judged with the defaults: 1e-300 / 8^11
        (dict(eps0=1e-290, shrink=0.0, max_rounds=0), 1),
    ]
    cols = ["epsabs", "epsrel", "eps0", "shrink", "max_rounds", "max_depth"]
    rows = []
    for diff, _ in table:
        row = dict(ok, **diff)
        rows.append([_hex(row[c]) if c not in ("max_rounds", "max_depth") else row[c] for c in cols])
    got = [int(x) for x in _run(san, tmp_path, "ok", rows).split()]
    assert got == [want for _, want in table], [(d, g) for (d, w), g in zip(table, got) if g != w]


@pytest.mark.parametrize("san", SAN)
def test_schedule_is_repeated_division(tmp_path, san):
    """Round r's EPSILON is eps0 divided r - 1 times: shrink = 8 is exact (a power of two), shrink = 10 and others
    equal Python's repeated division bit for bit (and differ from eps0 / shrink ** (r - 1) somewhere); zeros
    take the defaults 8 and 12."""
    cases = [(1e-3, 8.0, 12), (1e-2, 8.0, 7), (1e-3, 10.0, 12), (0.7, 3.0, 40), (1e-3, 0.0, 0), (1e-3, 10.0, 0),
             (5.0, 1000.0, 64)]
    lines = _run(san, tmp_path, "schedule", [(_hex(e), _hex(s), r) for e, s, r in cases]).splitlines()
    assert len(lines) == len(cases)
    power_differs = False
    for (eps0, shrink, rounds), ln in zip(cases, lines):
        f = ln.split()
        s, n = float.fromhex(f[0]), int(f[1])
        assert (s, n) == (shrink or 8.0, rounds or 12)
        got = [float.fromhex(x) for x in f[2:]]
        want = tr.schedule(eps0, s, n)
        assert len(got) == n and [g.hex() for g in got] == [w.hex() for w in want], (eps0, shrink, rounds)
        if s == 8.0:
            assert got == [eps0 * 2.0 ** (-3 * r) for r in range(n)]
        power_differs |= any(g != eps0 / s ** r for r, g in enumerate(got))
    assert power_differs
    assert (tr.DEFAULT_SHRINK, tr.DEFAULT_ROUNDS) == (8.0, 12)


@pytest.mark.parametrize("san", SAN)
def test_block_rows(tmp_path, san):
    """AQ_TOL_BLOCK: a value in [1, a whole launch] is the block, anything else a whole launch."""
    vals = [0, 1, 256, MAXK - 1, MAXK, MAXK + 1, -5, 2 ** 40]
    got = [int(x) for x in _run(san, tmp_path, "block", [[v] for v in vals]).split()]
    assert got == [MAXK, 1, 256, MAXK - 1, MAXK, MAXK, MAXK, MAXK]


@pytest.fixture(scope="module")
def lib():
    from ppls_amd import _lib
    return _lib.load()


def test_exports_and_strerror(lib):
    """The library exports the entry point, refuses a NULL context, and names the new code."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    assert " T aq_integrate_batch_tol\n" in out
    from ppls_amd import _lib
    t = _lib.aq_tol(0.0, 1e-6, 1e-3, 8.0, 12, 0)
    assert lib.aq_integrate_batch_tol(None, 0, None, None, None, COSH4, ctypes.byref(t), None, None, None, None, None,
                                      None, None) == -1
    text = lib.aq_strerror(-10)
    assert text and text != lib.aq_strerror(-1000) and b"tolerance" in text
    assert _lib.AQ_ENOCONV == -10 and ctypes.sizeof(_lib.aq_tol) == 40


def test_arguments_are_rejected_without_a_gpu(lib):
    """NULL tol or bounds, a theta that does not go with the integrand and a bad aq_tol are AQ_EINVAL before any
    device call (the context is never dereferenced)."""
    from ppls_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    one = (ctypes.c_double * 2)(0.0, 1.0)
    th = ctypes.cast(one, dp)
    fake = ctypes.c_void_p(1)
    good = _lib.aq_tol(0.0, 1e-6, 1e-3, 8.0, 12, 0)

    def call(ctx, n, a, b, theta, f, tol):
        return lib.aq_integrate_batch_tol(ctx, n, a, b, theta, f, None if tol is None else ctypes.byref(tol), None, None,
                                          None, None, None, None, None)
    assert call(fake, 1, th, th, None, COSH4, None) == -1
    assert call(fake, 1, None, th, None, COSH4, good) == -1
    assert call(fake, 1, th, None, None, COSH4, good) == -1
    assert call(fake, 1, th, th, th, COSH4, good) == -1       # theta, not PARAM
    assert call(fake, 1, th, th, None, PARAM, good) == -1     # PARAM, no theta
    assert call(fake, 1, th, th, None, 7, good) == -1
    for bad in (_lib.aq_tol(0.0, 0.0, 1e-3, 8.0, 12, 0), _lib.aq_tol(0.0, 1e-6, 0.0, 8.0, 12, 0),
                _lib.aq_tol(0.0, 1e-6, 1e-3, 1.5, 12, 0), _lib.aq_tol(0.0, 1e-6, 1e-3, 8.0, 65, 0),
                _lib.aq_tol(0.0, 1e-6, 1e-3, 8.0, 12, 128), _lib.aq_tol(0.0, 1e-6, 1e-300, 1024.0, 4, 0),
                _lib.aq_tol(float("nan"), 1e-6, 1e-3, 8.0, 12, 0)):
        assert call(fake, 1, th, th, None, COSH4, bad) == -1


def test_python_theta_checks_need_no_library_call():
    from ppls_amd import Context
    c = Context.__new__(Context)
    c.L, c._h = None, ctypes.c_void_p()
    one = np.array([0.0]), np.array([1.0])
    for call in (lambda: c.integrate_batch_tol(*one, epsrel=1e-6, integrand=PARAM),
                 lambda: c.integrate_batch_tol(*one, epsrel=1e-6, theta=[[0.0, 1.0]]),
                 lambda: c.integrate_batch_tol(*one, epsrel=1e-6, integrand=PARAM, theta=[[0.0, 1.0], [0.0, 1.0]])):
        with pytest.raises(ValueError):
            call()


def test_tol_result_is_the_seven_arrays_with_a_flag():
    from ppls_amd import TolResult
    r = TolResult(tuple(np.zeros(1) for _ in range(7)), False)
    assert len(r) == 7 and r.converged is False
    area, tasks, acc, ea, es, eps_used, rounds = r
    assert TolResult(tuple(r), True).converged is True


def _check_consistency(ref, n, k):
    """A run's own invariants: every integral retired exactly once, in a round whose EPSILON is the schedule's;
    converged rows meet the criterion with the values reported, unconverged ones miss it and sit in the last
    round; the live counts are what the retirements leave."""
    sched = tr.schedule(k["eps0"], k["shrink"], k["max_rounds"])
    r = np.abs(ref["rounds"])
    assert np.all((r >= 1) & (r <= k["max_rounds"]))
    assert np.array_equal(ref["eps_used"], np.array(sched)[r - 1])
    target = np.fmax(k["epsabs"], k["epsrel"] * np.abs(ref["area"]))
    conv = ref["rounds"] > 0
    assert np.all(ref["err_abs"][conv] <= target[conv]) and np.all(ref["err_abs"][~conv] > target[~conv])
    assert np.all(r[~conv] == k["max_rounds"])
    assert ref["live"] == [int(np.sum(r >= q)) for q in range(1, len(ref["live"]) + 1)] and ref["live"][0] == n
    assert np.all(ref["err_abs"] >= np.abs(ref["err_signed"])) and np.all(ref["leaves"] * 2 - 1 == ref["tasks"])
    assert len(ref["ratio"]) == len(ref["live"]) and [x.size for x in ref["ratio"]] == ref["live"]


def test_reference_set_p(oracle):
    """Set P: the live rows per round, the retirements and the distance of every decision from its slack."""
    a, b, theta, ref = tr.set_p()
    _check_consistency(ref, 600, tr.SET_P)
    print("set P live", ref["live"], "tasks", int(ref["tasks"].sum()), "ratio_min", ref["ratio_min"])
    assert ref["live"] == [600, 600, 600, 600, 600, 405, 85]
    assert [int(np.sum(ref["rounds"] == q)) for q in (5, 6, 7)] == [195, 320, 85] and np.all(ref["rounds"] > 0)
    assert ref["ratio_min"] >= 5e8
    # the retiring rounds' walks are those of a plain walk at that EPSILON (round 7: eps0 / 8^6)
    import err_reference as er
    sel = np.nonzero(ref["rounds"] == 7)[0]
    w = er.walk(a[sel], b[sel], 1e-3 / 8.0 ** 6, PARAM, oracle, theta[sel])
    assert np.array_equal(w["tasks"], ref["tasks"][sel]) and np.array_equal(w["err_abs"], ref["err_abs"][sel])


def test_reference_set_c(oracle):
    """Set C: 23 integrals miss epsabs = epsrel = 1e-6 within 7 rounds."""
    a, b, ref = tr.set_c()
    _check_consistency(ref, 300, tr.SET_C)
    print("set C live", ref["live"], "tasks", int(ref["tasks"].sum()), "ratio_min", ref["ratio_min"])
    assert ref["live"] == [300, 286, 233, 179, 145, 109, 66]
    assert int(np.sum(ref["rounds"] == -7)) == 23 and int(np.sum(ref["rounds"] < 0)) == 23
    assert ref["ratio_min"] >= 5e8
