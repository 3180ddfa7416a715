"""aq_integrate_batch_tol against the loop a caller writes without it: rounds of aq_integrate_batch_err at the same
EPSILON schedule, with the convergence test, the selection of the integrals that missed and the rebuilding of
a / b / theta on the host between two calls.

  python tools/bench_tol.py [--set P|C3] [--n N] [--runs 9] [--warmup 2]

Set P: tests/param_reference.draw(N) (default 200000), AQ_F_PARAM, epsrel = 1e-5 from eps0 = 1e-3, shrink 8, at
most 7 rounds. Set C3: N (default 1000000) splitmix64 bounds of cosh^4 (tools/bench_batch.py), epsrel = 1e-6
from eps0 = 1e-3, shrink 8, at most 12 rounds. The two loops run alternately after `warmup` runs of each; every
time is a host clock around a blocking call. Prints one JSON line: both medians, each one's min and max, the
rows live per round, and whether the two loops agree on rounds, eps_used, tasks and accepted.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ppls_amd import COSH4, PARAM, Context  # noqa: E402


def host_loop(ctx, a, b, theta, integrand, epsabs, epsrel, eps0, shrink, max_rounds):
    """What a caller writes on aq_integrate_batch_err: (tasks, accepted, eps_used, rounds, live per round)."""
    n = a.size
    tasks = np.zeros(n, np.uint64)
    acc = np.zeros(n, np.uint64)
    eps_used = np.zeros(n)
    rounds = np.zeros(n, np.int32)
    live = np.arange(n)
    counts = []
    eps = eps0
    for r in range(1, max_rounds + 1):
        counts.append(int(live.size))
        area, t, k, ea, _ = ctx.integrate_batch_err(a[live], b[live], eps, integrand=integrand,
                                                    theta=None if theta is None else theta[live])
        conv = ea <= np.fmax(epsabs, epsrel * np.abs(area))
        retire = conv | (r == max_rounds)
        at = live[retire]
        tasks[at], acc[at], eps_used[at] = t[retire], k[retire], eps
        rounds[at] = np.where(conv[retire], r, -r)
        live = live[~retire]
        if live.size == 0:
            break
        eps = eps / shrink
    return tasks, acc, eps_used, rounds, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="P", choices=["P", "C3"])
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.set == "P":
        import param_reference as pr
        a, b, theta = pr.draw(args.n or 200000)
        integrand, k = PARAM, dict(epsabs=0.0, epsrel=1e-5, eps0=1e-3, shrink=8.0, max_rounds=7)
    else:
        from tools.bench_batch import splitmix64_bounds
        a, b = splitmix64_bounds(args.n or 1000000)
        theta, integrand, k = None, COSH4, dict(epsabs=0.0, epsrel=1e-6, eps0=1e-3, shrink=8.0, max_rounds=12)
    with Context(0) as ctx:
        ctx.set_level_histograms(False)

        def device():
            return ctx.integrate_batch_tol(a, b, integrand=integrand, theta=theta, **k)

        def host():
            return host_loop(ctx, a, b, theta, integrand, **k)

        for _ in range(args.warmup):
            dev, hst = device(), host()
        t_dev, t_host = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            dev = device()
            t1 = time.perf_counter()
            hst = host()
            t2 = time.perf_counter()
            t_dev.append(t1 - t0)
            t_host.append(t2 - t1)
    same = bool(np.array_equal(dev[1], hst[0]) and np.array_equal(dev[2], hst[1]) and np.array_equal(dev[5], hst[2]) and
                np.array_equal(dev[6], hst[3]))
    out = {"set": args.set, "n": int(a.size), "runs": args.runs, "live_per_round": hst[4],
           "tasks_retiring_rounds": int(dev[1].sum()), "unconverged": int(np.sum(dev[6] < 0)),
           "device_loop_s": {"median": statistics.median(t_dev), "min": min(t_dev), "max": max(t_dev)},
           "host_loop_s": {"median": statistics.median(t_host), "min": min(t_host), "max": max(t_host)},
           "loops_agree": same}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
