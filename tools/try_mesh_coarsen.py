"""Mesh coarsening against the rebuild from the roots it can replace (diagnostic tool), in one process:
  1. Context.mesh_coarsen fine -> coarse (thresholds computed inside the call) against Context.integrate_mesh_batch at
     the coarse eps, for the `edges` and `param` rows of tests/mesh_batch_reference.py (restated here) and for the
     README's batch of 4096 Gaussians {mu_i, s_i} at 1e-6 -> 1e-4;
  2. the same with the thresholds passed in (many eps from one threshold array), and Context.mesh_thresholds alone;
  3. Context.mesh_coarsen(max_leaves=257) on the Gaussians (thresholds -> budget -> coarsen), which no single build
     replaces: every row has its own eps.
Both sides get the node capacity they need. 5 untimed calls of each, then --passes (default 10) timed passes
alternating the two; HIP events around the calls, which block, so a time is the call's whole duration, host looks
included. One JSON line each, printed and appended to --out: medians, spreads (max - min) / median, every pass, and the
leaf counts.
  python tools/try_mesh_coarsen.py [--passes 10] [--frontier-cap 4194304] [--out profiles/mesh_coarsen/ab.jsonl]"""
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
    ap.add_argument("--frontier-cap", type=int, default=1 << 22)
    ap.add_argument("--max-leaves", type=int, default=257)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_coarsen", "ab.jsonl"))
    args = ap.parse_args()
    FRONTIER_CAP = args.frontier_cap
    g = dict(dtype=torch.float64, device="cuda")
    dev = lambda v: None if v is None else torch.as_tensor(np.ascontiguousarray(v)).to("cuda")   # noqa: E731
    mu, s = torch.linspace(-2, 2, 4096, **g), torch.linspace(0.5, 2, 4096, **g)
    gauss = (mu - 6 / s, mu + 6 / s, torch.stack([mu, s], 1).contiguous())
    ea, eb = edges()
    pa, pb, pth = draw(64)
    cases = [("edges", COSH4, dev(ea), dev(eb), None, 1e-5, 1e-3), ("param", PARAM, dev(pa), dev(pb), dev(pth), 1e-6, 6.4e-5),
             ("gauss4096", PARAM, *gauss, 1e-6, 1e-4)]
    lines = []
    with Context(0) as ctx:
        for name, integrand, a, b, theta, feps, ceps in cases:
            kw = dict(integrand=integrand, theta=theta, frontier_cap=FRONTIER_CAP)
            fine = ctx.integrate_mesh_batch(a, b, feps, **kw)
            coarse = ctx.integrate_mesh_batch(a, b, ceps, **kw)
            m = coarse.n_nodes
            thr = ctx.mesh_thresholds(fine)
            out = ctx.mesh_coarsen(fine, ceps, cap_nodes=m)
            assert torch.equal(out.x, coarse.x) and torch.equal(out.f, coarse.f) and torch.equal(out.cum, coarse.cum)
            assert torch.equal(out.offsets, coarse.offsets) and out.merged == fine.leaves - coarse.leaves
            coarsen, build = alternate(lambda: ctx.mesh_coarsen(fine, ceps, cap_nodes=m),
                                       lambda: ctx.integrate_mesh_batch(a, b, ceps, cap_nodes=m, **kw), args.passes)
            reuse, thresholds = alternate(lambda: ctx.mesh_coarsen(fine, ceps, thr=thr, cap_nodes=m),
                                          lambda: ctx.mesh_thresholds(fine), args.passes)
            lines.append({"what": "mesh_coarsen fine -> coarse against integrate_mesh_batch at the coarse eps", "case": name,
                          "n": int(a.shape[0]), "eps": [feps, ceps], "leaves_fine": fine.leaves, "leaves_coarse": coarse.leaves,
                          "nodes_fine": fine.n_nodes, "tasks_coarse": coarse.total_tasks, "merged": out.merged,
                          "coarsen": coarsen, "build": build, "coarsen_given_thresholds": reuse, "thresholds": thresholds,
                          "build_over_coarsen": round(build["median_ms"] / coarsen["median_ms"], 3),
                          "build_over_coarsen_given_thresholds": round(build["median_ms"] / reuse["median_ms"], 3)})
            print(json.dumps(lines[-1]), flush=True)
        a, b, theta = gauss
        K = args.max_leaves
        out = ctx.mesh_coarsen(fine, max_leaves=K)     # (fine: the Gaussians at 1e-6, the last case)
        assert int(out.accepted.max()) <= K
        u = torch.linspace(0.0, 1.0, 101, **g)
        budget, quant = alternate(lambda: ctx.mesh_coarsen(fine, max_leaves=K), lambda: ctx.mesh_quantiles(out, u), args.passes)
        lines.append({"what": "mesh_coarsen(max_leaves) on the fine mesh: thresholds -> budget -> coarsen; and mesh_quantiles "
                              "(101 per row) of the result", "case": "gauss4096", "n": 4096, "max_leaves": K,
                      "leaves_fine": fine.leaves, "leaves_out": out.leaves, "rows_over_budget": int((out.eps >= 0).sum()),
                      "accepted_max_fine": int(fine.accepted.max()), "accepted_max_out": int(out.accepted.max()),
                      "budget": budget, "quantiles": quant})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
