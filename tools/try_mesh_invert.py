"""aq_mesh_invert's two kernel instances against each other on the GPU (diagnostic tool): the plain binary search
(AQ_MESH_INVERT=0) and the search staged through an LDS table (AQ_MESH_INVERT=1), plus the library's own choice, on
the mesh of Problem(eps) -- cosh^4 on [0, 5], 1e-10 by default. For nq = 4096, 2^16 and 2^20 .. 2^24 uniform random y,
and the same y sorted, it first checks that the instances agree bit for bit, then times them in alternating passes
with the context's HIP events around each launch (aq_kernel_timing). One JSON line per (nq, order): the node count,
every pass's mean time per call in microseconds for each instance, the median, and the pass-to-pass spread
(max - min) / median. Lines are printed and appended to --out.
  python tools/try_mesh_invert.py [--eps 1e-10] [--passes 7] [--out profiles/mesh_invert/ab.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch  # before the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ppls_amd import Context, Problem  # noqa: E402

CONFIGS = [("plain", {"AQ_MESH_INVERT": "0"}), ("staged", {"AQ_MESH_INVERT": "1"}), ("auto", {})]
# (nq, calls per timed pass)
SIZES = [(1 << 12, 400), (1 << 16, 200), (1 << 20, 50), (1 << 21, 50), (1 << 22, 20), (1 << 24, 10)]
KNOBS = ("AQ_MESH_INVERT",)


def call(ctx, mesh, y, out, env, reps=1):
    """reps launches under env (the library reads it per call); the context's stream is left running."""
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    x, f, cum = mesh
    for _ in range(reps):
        rc = ctx.L.aq_mesh_invert(ctx._h, x.numel(), x.data_ptr(), f.data_ptr(), cum.data_ptr(), y.numel(),
                                  y.data_ptr(), out.data_ptr())
        assert rc == 0, rc
    for k in KNOBS:
        os.environ.pop(k, None)


def agree(ctx, mesh, y, configs):
    """Every instance's output for y, bit for bit the first one's."""
    outs = []
    for _, env in configs:
        out = torch.empty_like(y)
        call(ctx, mesh, y, out, env)
        ctx.synchronize()
        outs.append(out.view(torch.int64))
    return all(torch.equal(outs[0], o) for o in outs[1:]) and not bool(torch.isnan(outs[0].view(torch.float64)).any())


def time_passes(ctx, mesh, y, configs, reps, passes):
    """{label: [mean us per call of each pass]}, the instances alternating inside every pass."""
    out = torch.empty_like(y)
    for _, env in configs:   # warm every instance at this shape
        call(ctx, mesh, y, out, env, 3)
    ctx.synchronize()
    us = {label: [] for label, _ in configs}
    for _ in range(passes):
        for label, env in configs:
            ctx.kernel_timing(True)
            call(ctx, mesh, y, out, env, reps)
            ms, n = ctx.kernel_time()
            assert n == reps, (n, reps)
            us[label].append(ms * 1e3 / reps)
    ctx.kernel_timing(False)
    return us


def measure(ctx, mesh, cum_m, configs, passes, sizes=SIZES, seed=20261):
    gen = torch.Generator(device=mesh[0].device).manual_seed(seed)
    y_all = torch.rand(max(nq for nq, _ in sizes), dtype=torch.float64, device=mesh[0].device, generator=gen) * cum_m
    lines = []
    for nq, reps in sizes:
        for order in ("random", "sorted"):
            y = y_all[:nq].contiguous() if order == "random" else torch.sort(y_all[:nq]).values.contiguous()
            torch.cuda.synchronize()
            line = {"n_nodes": mesh[0].numel(), "nq": nq, "order": order, "calls_per_pass": reps, "passes": passes,
                    "bit_identical": agree(ctx, mesh, y, configs)}
            assert line["bit_identical"], line
            for label, t in time_passes(ctx, mesh, y, configs, reps, passes).items():
                med = statistics.median(t)
                line[label] = {"us": [round(v, 3) for v in t], "median_us": round(med, 3),
                               "spread": round((max(t) - min(t)) / med, 4)}
            lines.append(line)
            print(json.dumps(line), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eps", type=float, default=1e-10)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_invert", "ab.jsonl"))
    args = ap.parse_args()
    with Context(0) as ctx:
        res, x, f, cum, level = ctx.integrate_mesh(Problem(eps=args.eps))
        del level
        lines = measure(ctx, (x, f, cum), cum[-1], CONFIGS, args.passes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(dict(line, eps=args.eps)) + "\n")


if __name__ == "__main__":
    main()
