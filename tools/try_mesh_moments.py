"""Mesh moments against the error sums over the same bytes (diagnostic tool), in one process: on the README's batch of
4096 Gaussians {mu_i, s_i} at --eps (default 1e-6), aq_mesh_moments_batch at order 1 and at order 4 (centre the row's
mu, whole rows) against aq_mesh_err_batch, the existing one-pass call that reads the same x and f once.
The three calls only enqueue, so a timed pass is --reps (default 2000) calls of one of them on the context's stream and
one synchronise, a host clock around the lot: a pass lasts tens of milliseconds, and a call's time is the pass over
--reps, launch gaps included (two kernels per call each). 5 untimed passes of each, then --passes (default 10) timed
passes alternating the three. One JSON line, printed and appended to --out: medians, spreads (max - min) / median, every
pass, the mesh's size and the bytes per second each median amounts to (16 bytes per node).
  python tools/try_mesh_moments.py [--passes 10] [--reps 2000] [--eps 1e-6] [--note TEXT]
                                   [--out profiles/mesh_moments/ab.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # before the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ppls_amd import PARAM, Context  # noqa: E402


def summary(us):
    med = statistics.median(us)
    return {"us": [round(v, 3) for v in us], "median_us": round(med, 3), "spread": round((max(us) - min(us)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--frontier-cap", type=int, default=1 << 22)
    ap.add_argument("--note", default="", help="a word on the code measured, kept in the line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_moments", "ab.jsonl"))
    args = ap.parse_args()
    g = dict(dtype=torch.float64, device="cuda")
    mu, s = torch.linspace(-2, 2, 4096, **g), torch.linspace(0.5, 2, 4096, **g)
    with Context(0) as ctx:
        mesh = ctx.integrate_mesh_batch(mu - 6 / s, mu + 6 / s, args.eps, integrand=PARAM,
                                        theta=torch.stack([mu, s], 1).contiguous(), frontier_cap=args.frontier_cap)
        n = len(mesh)
        # the results the timed calls give: the statistics of the Gaussians, as a check that the work is real
        st = ctx.mesh_stats(mesh)
        assert torch.allclose(st.mean, mu, atol=1e-3) and torch.allclose(st.var, 0.5 / (s * s), rtol=1e-2)
        ea, es = (torch.empty(n, **g) for _ in range(2))
        out = torch.empty(n * 5, **g)
        c = mu.contiguous()
        torch.cuda.synchronize()
        p = [t.data_ptr() for t in (mesh.offsets, mesh.x, mesh.f)]

        def err():
            return ctx.L.aq_mesh_err_batch(ctx._h, n, *p, ea.data_ptr(), es.data_ptr())

        def moments(order):
            return lambda: ctx.L.aq_mesh_moments_batch(ctx._h, n, *p, order, c.data_ptr(), None, None, out.data_ptr())

        calls = {"err": err, "moments1": moments(1), "moments4": moments(4)}

        def one_pass(fn):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                rc = fn()
            ctx.synchronize()
            assert rc == 0
            return (time.perf_counter() - t0) * 1e6 / args.reps

        for _ in range(5):
            for fn in calls.values():
                one_pass(fn)
        us = {k: [] for k in calls}
        for _ in range(args.passes):
            for k, fn in calls.items():
                us[k].append(one_pass(fn))
        line = {"what": "aq_mesh_moments_batch at order 1 and 4 against aq_mesh_err_batch on one mesh, per call",
                "case": "gauss4096", "eps": args.eps, "n": n, "nodes": mesh.n_nodes, "leaves": mesh.leaves,
                "bytes_read": 16 * mesh.n_nodes, "reps": args.reps, "note": args.note}
        for k in calls:
            line[k] = summary(us[k])
            line[k]["GB_per_s"] = round(16 * mesh.n_nodes / line[k]["median_us"] / 1e3, 1)
        line["moments1_over_err"] = round(line["moments1"]["median_us"] / line["err"]["median_us"], 3)
        line["moments4_over_err"] = round(line["moments4"]["median_us"] / line["err"]["median_us"], 3)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
