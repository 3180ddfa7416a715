"""aq_integrate_mesh_batch against the loop of aq_integrate_mesh calls it replaces (diagnostic tool), in one process:
  1. ONE aq_integrate_mesh_batch over n (default 4096) AQ_F_USER Gaussian rows -- the bounds drawn as
     tests/param_reference.draw draws them (the same seed and order) -- at eps (default 1e-6), device arrays
     preallocated;
  2. the loop of n aq_integrate_mesh calls on the same rows, one blocking call each, into preallocated arrays.
5 untimed calls of each, then --passes (default 10) timed passes alternating the two, a host clock around the blocking
calls (each ends in a stream synchronise). Then the AQ_F_PARAM batch of draw(n) -- every row its own {mu, s} -- which
has no per-row baseline, timed the same way alone. One JSON line each, printed and appended to --out: medians, spreads
(max - min) / median, every pass, and the leaf totals.
  python tools/try_mesh_batch.py [--n 4096] [--eps 1e-6] [--passes 10] [--out profiles/mesh_batch/ab.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ppls_amd import PARAM, USER, Context, Problem, _lib  # noqa: E402

DRAW_SEED = 20240607   # tests/param_reference.py
FRONTIER_CAP = 1 << 21
AQ_EOVERFLOW = -4


def draw(n, seed=DRAW_SEED):
    """tests/param_reference.draw, restated: mu in [-2, 2], s = e^U(-2, 2), bounds mu - U(0, 4)/s .. mu + U(0.1, 4)/s."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-2.0, 2.0, n)
    s = np.exp(rng.uniform(-2.0, 2.0, n))
    a = mu - rng.uniform(0.0, 4.0, n) / s
    b = mu + rng.uniform(0.1, 4.0, n) / s
    return a, b, np.ascontiguousarray(np.stack([mu, s], axis=1))


class BatchCall:
    """aq_integrate_mesh_batch on preallocated device arrays (sized by a first call that is told the node count)."""

    def __init__(self, ctx, integrand, a, b, theta, eps):
        dev = "cuda:%d" % ctx.device
        self.ctx, self.integrand, self.eps, self.n = ctx, integrand, eps, a.size
        self.a, self.b = (torch.as_tensor(v).to(dev) for v in (a, b))
        self.theta = None if theta is None else torch.as_tensor(theta).to(dev)
        self.offsets = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.area = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.info = _lib.aq_mesh_batch_info()
        self.cap = 3
        self._alloc(dev)
        rc = self()
        assert rc == AQ_EOVERFLOW and self.info.n_nodes, (rc, self.info.n_nodes)
        self.cap = int(self.info.n_nodes)
        self._alloc(dev)
        assert self() == 0

    def _alloc(self, dev):
        self.x, self.f, self.cum = (torch.empty(self.cap, dtype=torch.float64, device=dev) for _ in range(3))
        self.level = torch.empty(self.cap, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        self.io = _lib.aq_mesh_batch_io(ptr(self.a), ptr(self.b), ptr(self.theta), ptr(self.offsets), ptr(self.x),
                                        ptr(self.f), ptr(self.cum), ptr(self.level), ptr(self.area), None, None, None, 0, 0)

    def __call__(self):
        return self.ctx.L.aq_integrate_mesh_batch(self.ctx._h, self.n, ctypes.byref(self.io), self.eps, self.integrand,
                                                  FRONTIER_CAP, 4, self.cap, ctypes.byref(self.info))


class LoopCall:
    """n aq_integrate_mesh calls, one row each, into arrays that hold the largest row."""

    def __init__(self, ctx, integrand, a, b, eps, max_nodes):
        dev = "cuda:%d" % ctx.device
        self.ctx = ctx
        self.x, self.f, self.cum = (torch.empty(max_nodes, dtype=torch.float64, device=dev) for _ in range(3))
        self.level = torch.empty(max_nodes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.io = _lib.aq_mesh_io(self.x.data_ptr(), self.f.data_ptr(), self.cum.data_ptr(), self.level.data_ptr())
        self.cap = max_nodes
        self.problems = [Problem(integrand, float(u), float(v), eps).c() for u, v in zip(a, b)]
        self.res, self.nn = _lib.aq_result(), ctypes.c_uint64(0)

    def __call__(self):
        L, h, io, res, nn, cap = self.ctx.L, self.ctx._h, ctypes.byref(self.io), ctypes.byref(self.res), ctypes.byref(self.nn), self.cap
        leaves = 0
        for p in self.problems:
            rc = L.aq_integrate_mesh(h, ctypes.byref(p), FRONTIER_CAP, 4, cap, io, res, nn)
            assert rc == 0, rc
            leaves += self.res.accepted
        return leaves


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    med = statistics.median(ms)
    return {"ms": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_batch", "ab.jsonl"))
    args = ap.parse_args()
    a, b, theta = draw(args.n)
    lines = []
    with Context(0) as ctx:
        batch = BatchCall(ctx, USER, a, b, None, args.eps)
        off = batch.offsets.cpu().numpy()
        loop = LoopCall(ctx, USER, a, b, args.eps, int(np.diff(off).max()))
        for _ in range(5):
            assert batch() == 0
            loop()
        tb, tl, loop_leaves = [], [], 0
        for _ in range(max(args.passes, 10)):
            ms, rc = timed(batch)
            assert rc == 0
            tb.append(ms)
            ms, loop_leaves = timed(loop)
            tl.append(ms)
        assert loop_leaves == batch.info.leaves, (loop_leaves, batch.info.leaves)
        line = {"what": "USER rows: one batch call against the loop of single-mesh calls", "n": args.n, "eps": args.eps,
                "leaves": int(batch.info.leaves), "n_nodes": int(batch.info.n_nodes), "levels": int(batch.info.levels),
                "widest_level": int(batch.info.widest_level), "batch": summary(tb), "loop": summary(tl)}
        line["loop_over_batch"] = round(line["loop"]["median_ms"] / line["batch"]["median_ms"], 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
        par = BatchCall(ctx, PARAM, a, b, theta, args.eps)
        for _ in range(5):
            assert par() == 0
        tp = []
        for _ in range(max(args.passes, 10)):
            ms, rc = timed(par)
            assert rc == 0
            tp.append(ms)
        line = {"what": "PARAM rows (draw(n)): one batch call, no per-row baseline", "n": args.n, "eps": args.eps,
                "leaves": int(par.info.leaves), "n_nodes": int(par.info.n_nodes), "levels": int(par.info.levels),
                "widest_level": int(par.info.widest_level), "batch": summary(tp)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
