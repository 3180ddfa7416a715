"""aq_integrate_batch_device against the host batch (aq_integrate_batch) on the same rows, for a caller whose
bounds and results live on the GPU.

  python tools/bench_device_batch.py [--set C3|bench] [--n N] [--eps E] [--runs 7] [--host-only]

Set C3: N (default 1000000) splitmix64 bounds of cosh^4 (tools/bench_batch.py). Set bench: N (default 32768) times
cosh^4 on [0, 5] (bench.py's shape). The two paths run alternately after a warm-up of each:
  device   HIP events on the caller's stream around the call, inputs already on the device, outputs left there;
  host     a host clock around aq_integrate_batch on host arrays, and, separately, what a caller with device
           arrays pays on top: the copy of a, b to the host and of area, tasks, accepted back to the device.
Prints one JSON line: medians with min and max (ms), the device call's host time, whether the two paths agree on
tasks and accepted, and how many areas have the same bits. --host-only (e.g. with AQ_LIB naming another build of the
library): the
host path alone.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch   # before the library is loaded: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ppls_amd import Context  # noqa: E402


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="C3", choices=["C3", "bench"])
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    if args.set == "C3":
        from tools.bench_batch import splitmix64_bounds
        a, b = splitmix64_bounds(args.n or 1000000)
    else:
        n = args.n or 32768
        a, b = np.zeros(n), np.full(n, 5.0)
    n = a.size
    dev = torch.device("cuda", 0)
    da, db = torch.as_tensor(a).to(dev), torch.as_tensor(b).to(dev)
    out_h = (np.empty(n), np.empty(n, np.uint64), np.empty(n, np.uint64))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with Context(0) as ctx:
        ctx.set_level_histograms(False)
        out_d = None

        def device():
            nonlocal out_d
            e0.record()
            t0 = time.perf_counter()
            out_d = ctx.integrate_batch_device(da, db, args.eps, out=out_d)
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), (t1 - t0) * 1e3

        def host():
            t0 = time.perf_counter()
            ctx.integrate_batch(a, b, args.eps, out=out_h)
            return (time.perf_counter() - t0) * 1e3

        def copies():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ha, hb = da.cpu().numpy(), db.cpu().numpy()
            t1 = time.perf_counter()
            back = [torch.as_tensor(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev) for x in out_h]
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, ha.size + hb.size + len(back)

        t_dev, t_call, t_host, t_down, t_up = [], [], [], [], []
        for i in range(args.runs + 1):   # (run 0: the warm-up of each)
            if not args.host_only:
                d, c = device()
            h = host()
            dn, up, _ = copies()
            if i:
                t_host.append(h), t_down.append(dn), t_up.append(up)
                if not args.host_only:
                    t_dev.append(d), t_call.append(c)
        res = {"set": args.set, "n": int(n), "eps": args.eps, "runs": args.runs, "lib": os.environ.get("AQ_LIB", "in-tree"),
               "host_call_ms": stats(t_host), "caller_d2h_inputs_ms": stats(t_down), "caller_h2d_outputs_ms": stats(t_up),
               "tasks": int(out_h[1].sum())}
        if not args.host_only:
            ctx.device_batch_check()
            o = [t.cpu().numpy() for t in (out_d.area, out_d.tasks, out_d.accepted)]
            res["device_path_ms"] = stats(t_dev)
            res["device_call_host_ms"] = stats(t_call)
            res["counts_agree"] = bool(np.array_equal(o[1], out_h[1].view(np.int64)) and np.array_equal(o[2], out_h[2].view(np.int64)))
            # (an area's last bits depend on the launch's schedule: reported, not required)
            res["areas_same_bits"] = int(np.sum(o[0].view(np.int64) == out_h[0].view(np.int64)))
            res["areas_max_rel_diff"] = float(np.max(np.abs(o[0] - out_h[0]) / np.maximum(np.abs(out_h[0]), 1e-300)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
