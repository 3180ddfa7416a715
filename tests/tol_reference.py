"""Reference for the tolerance-driven batch (aq_integrate_batch_tol): tests/err_reference.py's walker driven
round by round with the call's own schedule and criterion.

Round r walks the live integrals at eps_r (eps_1 = eps0, eps_{r+1} = eps_r / shrink: one division per round,
as the library's loop does it, so the values agree bit for bit). An integral converges in a round when
    err_abs <= fmax(epsabs, epsrel * |area|)
with the walker's math.fsum sums, and retires when it converges or in round max_rounds (the walker has no
error bits). Every decision also records margin / slack: margin = |err_abs - target| is how far the decision
is from flipping, slack = err_reference.tol(w) + epsrel * ulp(|area|) is how far the device's figures may
lie from the walker's (its err_abs within tol, its area within 1 ulp). A test may rely on a decision only
when margin >= 16 * slack.

A helper module, not a conftest: the CPU and GPU tests import it and share its cached results.
"""
import functools
import math

import numpy as np

import err_reference as er
import param_reference as pr

PARAM = 3
DEFAULT_SHRINK = 8.0
DEFAULT_ROUNDS = 12
SAFE = 16.0   # margin / slack every relied-on decision must reach


def schedule(eps0, shrink, max_rounds):
    """[eps_1, ..., eps_max_rounds] by repeated division."""
    out, e = [], float(eps0)
    for _ in range(max_rounds):
        out.append(e)
        e = e / float(shrink)
    return out


def run(a, b, integrand, epsabs, epsrel, eps0, shrink=DEFAULT_SHRINK, max_rounds=DEFAULT_ROUNDS, theta=None):
    """The call's outputs from the walker: per-integral rounds (+r converged in round r, -r retired there
    unconverged), eps_used, tasks, leaves, area, err_abs, err_signed of the retiring round; `live` (rows per
    round, in order), and `ratio`: margin / slack of every decision, one array per round over that round's
    live rows (`ratio_min`: the least of them all)."""
    from oracle import pyoracle
    a = np.ascontiguousarray(a, np.float64).ravel()
    b = np.ascontiguousarray(b, np.float64).ravel()
    n = a.size
    if integrand == PARAM:
        theta = np.ascontiguousarray(theta, np.float64).reshape(n, 2)
    out = {"rounds": np.zeros(n, np.int32), "eps_used": np.zeros(n), "tasks": np.zeros(n, np.int64),
           "leaves": np.zeros(n, np.int64), "area": np.zeros(n), "err_abs": np.zeros(n), "err_signed": np.zeros(n)}
    live_idx = np.arange(n)
    live, ratio = [], []
    for r, eps in enumerate(schedule(eps0, shrink, max_rounds), start=1):
        if live_idx.size == 0:
            break
        live.append(int(live_idx.size))
        w = er.walk(a[live_idx], b[live_idx], eps, integrand, pyoracle, None if theta is None else theta[live_idx])
        target = np.fmax(epsabs, epsrel * np.abs(w["area"]))
        conv = w["err_abs"] <= target
        slack = er.tol(w) + epsrel * np.spacing(np.abs(w["area"]))
        ratio.append(np.abs(w["err_abs"] - target) / slack)
        retire = conv | (r == max_rounds)
        at = live_idx[retire]
        out["rounds"][at] = np.where(conv[retire], r, -r)
        out["eps_used"][at] = eps
        for k in ("tasks", "leaves", "area", "err_abs", "err_signed"):
            out[k][at] = w[k][retire]
        live_idx = live_idx[~retire]
    for v in out.values():
        v.flags.writeable = False
    out["live"] = live
    out["ratio"] = ratio
    out["ratio_min"] = min((float(x.min()) for x in ratio), default=math.inf)
    return out


def row_tol(ref):
    """err_reference.tol per integral of a run (the bound on either sum's deviation from the walker's)."""
    return ref["leaves"] * 2.0 ** -52 * ref["err_abs"]


# The two sets of the GPU tests.
SET_P = dict(n=600, epsabs=0.0, epsrel=1e-5, eps0=1e-3, shrink=8.0, max_rounds=7)
SET_C = dict(n=300, epsabs=1e-6, epsrel=1e-6, eps0=1e-2, shrink=8.0, max_rounds=7)


@functools.lru_cache(maxsize=None)
def set_p():
    """param_reference.draw(600), AQ_F_PARAM, epsrel = 1e-5 from eps0 = 1e-3 in at most 7 rounds."""
    k = SET_P
    a, b, theta = pr.draw(k["n"])
    ref = run(a, b, PARAM, k["epsabs"], k["epsrel"], k["eps0"], k["shrink"], k["max_rounds"], theta)
    for v in (a, b, theta):
        v.flags.writeable = False
    return a, b, theta, ref


@functools.lru_cache(maxsize=None)
def set_c(n=SET_C["n"], max_rounds=SET_C["max_rounds"]):
    """The first n of pyoracle.batch_bounds(300), cosh^4, epsabs = epsrel = 1e-6 from eps0 = 1e-2."""
    from oracle import pyoracle
    k = SET_C
    a, b = pyoracle.batch_bounds(k["n"])
    a, b = a[:n].copy(), b[:n].copy()
    ref = run(a, b, 0, k["epsabs"], k["epsrel"], k["eps0"], k["shrink"], max_rounds)
    for v in (a, b):
        v.flags.writeable = False
    return a, b, ref


@functools.lru_cache(maxsize=None)
def lone(integrand, a, b, epsabs, epsrel, eps0, shrink=DEFAULT_SHRINK, max_rounds=DEFAULT_ROUNDS):
    """One integral's run, computed once per process."""
    return run([a], [b], integrand, epsabs, epsrel, eps0, shrink, max_rounds)
