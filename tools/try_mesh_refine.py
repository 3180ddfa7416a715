"""Mesh refinement against the rebuild from the roots it replaces (diagnostic tool), in one process:
  1. Context.mesh_refine coarse -> fine against Context.integrate_mesh_batch at the fine eps, for the `edges` and
     `param` rows of tests/mesh_batch_reference.py (restated here) and for the README's batch of 4096 Gaussians
     {mu_i, s_i} at 1e-4 -> 1e-6;
  2. Context.integrate_mesh_batch_tol on that Gaussian batch with --epsrel (default 1e-8) against integrate_mesh_batch
     of every row at the smallest eps_used, which is what a caller had without refinement (--skip-refine: this alone).
Both sides get the node capacity they need, so neither retries. 5 untimed calls of each, then --passes (default 10)
timed passes alternating the two; HIP events around the calls, which block, so a time is the call's whole duration,
host looks included. One JSON line each, printed and appended to --out: medians, spreads (max - min) / median, every
pass, and the task counts.
  python tools/try_mesh_refine.py [--passes 10] [--epsrel 1e-8] [--frontier-cap 4194304] [--skip-refine]
                                  [--out profiles/mesh_refine/ab.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # before the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ppls_amd import COSH4, PARAM, Context  # noqa: E402

DRAW_SEED = 20240607   # tests/param_reference.py


def draw(n, seed=DRAW_SEED):
    """tests/param_reference.draw, restated."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-2.0, 2.0, n)
    s = np.exp(rng.uniform(-2.0, 2.0, n))
    a = mu - rng.uniform(0.0, 4.0, n) / s
    b = mu + rng.uniform(0.1, 4.0, n) / s
    return a, b, np.ascontiguousarray(np.stack([mu, s], axis=1))


def edges():
    """tests/mesh_batch_reference.edges_bounds, restated: 300 one-leaf rows and seven more, two of them invalid."""
    k = np.arange(300, dtype=np.float64)
    tail = [(-3.0, 2.0), (1.0, 1.0), (2.0, 1.0), (0.0, 171.0), (0.0, 5.0), (-1.0, 0.5), (0.0, 0.25)]
    return (np.concatenate([k * 1e-3, [r[0] for r in tail]]), np.concatenate([(k + 1) * 1e-3, [r[1] for r in tail]]))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def summary(ms):
    med = statistics.median(ms)
    return {"ms": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def alternate(first, second, passes, warm=5):
    for _ in range(warm):
        first()
        second()
    t1, t2 = [], []
    for _ in range(passes):
        t1.append(timed(first)[0])
        t2.append(timed(second)[0])
    return summary(t1), summary(t2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--epsrel", type=float, default=1e-8)
    ap.add_argument("--frontier-cap", type=int, default=1 << 22)
    ap.add_argument("--skip-refine", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_refine", "ab.jsonl"))
    args = ap.parse_args()
    FRONTIER_CAP = args.frontier_cap
    g = dict(dtype=torch.float64, device="cuda")
    dev = lambda v: None if v is None else torch.as_tensor(np.ascontiguousarray(v)).to("cuda")   # noqa: E731
    mu, s = torch.linspace(-2, 2, 4096, **g), torch.linspace(0.5, 2, 4096, **g)
    gauss = (mu - 6 / s, mu + 6 / s, torch.stack([mu, s], 1).contiguous())
    ea, eb = edges()
    pa, pb, pth = draw(64)
    cases = [("edges", COSH4, dev(ea), dev(eb), None, 1e-3, 1e-5), ("param", PARAM, dev(pa), dev(pb), dev(pth), 6.4e-5, 1e-6),
             ("gauss4096", PARAM, *gauss, 1e-4, 1e-6)]
    lines = []
    with Context(0) as ctx:
        for name, integrand, a, b, theta, ceps, feps in ([] if args.skip_refine else cases):
            kw = dict(integrand=integrand, theta=theta, frontier_cap=FRONTIER_CAP)
            coarse = ctx.integrate_mesh_batch(a, b, ceps, **kw)
            fine = ctx.integrate_mesh_batch(a, b, feps, **kw)
            m = fine.n_nodes
            out = ctx.mesh_refine(coarse, feps, cap_nodes=m, frontier_cap=FRONTIER_CAP)
            assert torch.equal(out.x, fine.x) and torch.equal(out.cum, fine.cum) and out.evaluated == fine.total_tasks - coarse.total_tasks
            refine, build = alternate(lambda: ctx.mesh_refine(coarse, feps, cap_nodes=m, frontier_cap=FRONTIER_CAP),
                                      lambda: ctx.integrate_mesh_batch(a, b, feps, cap_nodes=m, **kw), args.passes)
            lines.append({"what": "mesh_refine coarse -> fine against integrate_mesh_batch at the fine eps", "case": name,
                          "n": int(a.shape[0]), "eps": [ceps, feps], "tasks_coarse": coarse.total_tasks,
                          "tasks_fine": fine.total_tasks, "evaluated": out.evaluated, "reseeded": out.reseeded,
                          "leaves_coarse": coarse.leaves, "leaves_fine": fine.leaves, "widest_level_refine": out.widest_level,
                          "widest_level_build": fine.widest_level, "refine": refine, "build": build,
                          "build_over_refine": round(build["median_ms"] / refine["median_ms"], 3)})
            print(json.dumps(lines[-1]), flush=True)
        a, b, theta = gauss
        kw = dict(integrand=PARAM, theta=theta, frontier_cap=FRONTIER_CAP)
        res = ctx.integrate_mesh_batch_tol(a, b, epsrel=args.epsrel, **kw)
        least = float(res.eps_used.min())
        flat = ctx.integrate_mesh_batch(a, b, least, **kw)
        m = flat.n_nodes
        tol, build = alternate(lambda: ctx.integrate_mesh_batch_tol(a, b, epsrel=args.epsrel, cap_nodes=m, **kw),
                               lambda: ctx.integrate_mesh_batch(a, b, least, cap_nodes=m, **kw), args.passes)
        rounds = res.rounds.cpu().numpy()
        lines.append({"what": "integrate_mesh_batch_tol against integrate_mesh_batch of every row at the smallest eps_used",
                      "case": "gauss4096", "epsrel": args.epsrel, "n": 4096, "converged": res.converged,
                      "rows_retired_in_round": np.bincount(np.abs(rounds)).tolist(), "eps_used_min": least,
                      "evaluated_tol": res.evaluated, "nodes_tol": res.mesh.n_nodes, "tasks_flat": flat.total_tasks,
                      "nodes_flat": flat.n_nodes, "tol": tol, "flat": build,
                      "flat_over_tol": round(build["median_ms"] / tol["median_ms"], 3)})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
