"""Regenerate the committed golden fixtures under tests/golden/.

Run HERE (the build container), never on the GPU box:  python tests/golden/make_golden.py

Sources of truth, in order:
  1. the reference itself: oracle/_ref/aquadPartA_* compiled from /root/reference/aquadPartA.c by
     oracle/Makefile (`make -C oracle ref`), run under the image's MPICH `mpirun`. Its stdout
     (the `Area=%lf` line and the tasks-per-process row, aquadPartA.c:107-117) is recorded verbatim;
  2. the host glibc 2.35 libm (cosh / exp bit patterns at tree points and random points);
  3. the oracle's restatement (oracle/aq_oracle.c) for what the reference does not print:
     per-level task/leaf histograms, leaf counts, the quad-precision Σ of leaf areas.
Every oracle number that the reference also prints is cross-checked here before it is written.

Outputs (data only, no code of the reference):
  trees.json      per config: counts, per-level histograms, areas, reference stdout
  libm_bits.npz   x, cosh(x), exp(x) as uint64 bit patterns from the host libm
  batch.json      splitmix64 batch bounds KATs and per-integral counts (config C3 prefix)
  plugin_bits.npz x, F(x) of the AQ_F_USER plug-in (exp(-x*x), host libm) as uint64 bit patterns
  deep.json       eps 1e-14 .. 1e-16 cosh4 trees pinned by the reference binary's task totals
  sin_bits.npz    x, F(x) = sin(1.0/x) (config 4's F macro, host libm) as uint64 bit patterns
  edges.json      trees at the edges of the documented domain (|x| = 170, subnormal areas, eps = 0, 2^-900, 2^900),
                  on which the restated and the host-libm oracle modes must agree
  recip_hard_bits.npz  x, cosh(x) (host libm) where 0.5 / exp(x) lies within 100 * 2^-106 (relative) of a rounding
                  midpoint (needs sympy)
"""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MPIRUN = "/opt/conda/bin/mpirun"

# name, integrand, a, b, eps, reference binary (oracle/_ref), mpirun -n
CONFIGS = [
    ("cosh4_eps1e-3", O.COSH4, 0.0, 5.0, 1e-3, "aquadPartA_eps1e-3", 5),
    ("cosh4_eps1e-6", O.COSH4, 0.0, 5.0, 1e-6, None, 0),
    ("cosh4_eps1e-8", O.COSH4, 0.0, 5.0, 1e-8, None, 0),
    ("cosh4_eps1e-10", O.COSH4, 0.0, 5.0, 1e-10, "aquadPartA_eps1e-10", 5),
    ("cosh4_eps1e-12", O.COSH4, 0.0, 5.0, 1e-12, "aquadPartA_eps1e-12", 5),
    ("sin_recip_eps1e-9", O.SIN_RECIP, 1e-4, 1.0, 1e-9, "aquadPartA_sin_eps1e-9", 5),
    # edge cases: one-task tree (accepted at the root), empty interval, tiny domain
    ("cosh4_eps1e3_root_leaf", O.COSH4, 0.0, 5.0, 1e9, None, 0),
    ("cosh4_empty_interval", O.COSH4, 2.0, 2.0, 1e-3, None, 0),
    ("cosh4_neg_domain", O.COSH4, -1.5, 0.75, 1e-9, None, 0),
]


def run_reference(binary, nprocs):
    path = os.path.join(O.REF_DIR, binary)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(O.REF_DIR), "ref"])
    out = subprocess.run([MPIRUN, "-n", str(nprocs), path], check=True, capture_output=True, text=True,
                         timeout=600).stdout
    m = re.search(r"Area=(\S+)", out)
    rows = [ln for ln in out.strip().splitlines() if ln.strip()]
    counts = [int(v) for v in rows[-1].split()]
    return {"stdout": out, "area_printed": m.group(1), "tasks_per_process": counts, "tasks_total": sum(counts),
            "nprocs": nprocs}


def trees():
    out = {}
    for name, integrand, a, b, eps, ref, nprocs in CONFIGS:
        r = O.integrate(integrand, a, b, eps)
        rec = {
            "integrand": "cosh4" if integrand == O.COSH4 else "sin_recip",
            "a": a, "b": b, "eps": eps,
            "tasks": r.tasks, "leaves": r.leaves, "levels": r.levels,
            "tasks_per_level": r.tasks_per_level, "leaves_per_level": r.leaves_per_level,
            "area_quad": r.area_quad_str,
            "area_lifo_hex": float(r.area_lifo).hex(),
            "area_lifo_printed": "%f" % r.area_lifo,
        }
        assert r.tasks == 2 * r.leaves - 1 or r.tasks == 0
        if ref and os.path.exists("/root/reference"):
            refrun = run_reference(ref, nprocs)
            # the reference's own totals pin the restatement
            assert refrun["tasks_total"] == r.tasks, (name, refrun["tasks_total"], r.tasks)
            assert refrun["area_printed"] == "%f" % (r.area_quad_hi + r.area_quad_lo), (name, refrun["area_printed"])
            # P=2 (one worker) is deterministic LIFO order: the printed area must be area_lifo exactly
            ref2 = run_reference(ref, 2)
            assert ref2["tasks_total"] == r.tasks
            assert ref2["area_printed"] == "%f" % r.area_lifo
            rec["reference"] = refrun
            rec["reference_p2"] = ref2
        out[name] = rec
        print(name, r.tasks, r.leaves, r.levels, r.area_quad_str)
    with open(os.path.join(OUT, "trees.json"), "w") as f:
        json.dump(out, f, indent=1)


def tree_points(eps=1e-10, a=0.0, b=5.0):
    """All distinct F arguments of the cosh4 tree (endpoints + midpoints), via a BFS in numpy."""
    pts = [np.array([a, b])]
    l = np.array([a]); r = np.array([b])
    fl = O.cosh(l, O.HOST_LIBM) ** 4; fr = O.cosh(r, O.HOST_LIBM) ** 4
    # F = ((c*c)*c)*c, same as c**4? not guaranteed: compute explicitly
    def F(x):
        c = O.cosh(x, O.HOST_LIBM)
        return c * c * c * c
    fl = F(l); fr = F(r)
    while l.size:
        lr = (fl + fr) * (r - l) / 2
        m = (l + r) / 2
        fm = F(m)
        pts.append(m)
        la = (fl + fm) * (m - l) / 2
        ra = (fm + fr) * (r - m) / 2
        ref = np.abs((la + ra) - lr) > eps
        l, r, fl, fr = (np.concatenate([l[ref], m[ref]]), np.concatenate([m[ref], r[ref]]),
                        np.concatenate([fl[ref], fm[ref]]), np.concatenate([fm[ref], fr[ref]]))
    return np.concatenate(pts)


def libm_bits():
    rng = np.random.default_rng(20261015)
    tp = tree_points(1e-10)
    sample_tp = rng.choice(tp, 6000, replace=False)
    edges = np.array([0.0, 2.0 ** -60, 2.0 ** -55, 2.0 ** -54, 1e-10, 0.25, 0.3465735902799726,
                      0.34657359027997264, 0.3465735902799727, 0.5, 1.0, 2.5, 4.999999999999999, 5.0,
                      5.000000000000001, 10.0, 21.999999999999996, 22.0, 30.0, 100.0, 177.0, 700.0, 709.0,
                      710.4758600739439, 711.0, -0.3, -5.0, 1e-300, 5e-324])
    uni = rng.uniform(0.0, 5.0, 2000)
    x = np.concatenate([edges, sample_tp, uni])
    cosh = O.cosh(x, O.HOST_LIBM)
    expx = np.abs(x)
    expx = np.where((expx > 2.0 ** -54) & (expx < 709.0), expx, 1.0)
    exp = O.exp(expx, O.HOST_LIBM)
    np.savez_compressed(os.path.join(OUT, "libm_bits.npz"), x=x.view(np.uint64), cosh=cosh.view(np.uint64),
                        exp_x=expx.view(np.uint64), exp=exp.view(np.uint64))
    # the restatement must already agree
    assert (O.cosh(x).view(np.uint64) == cosh.view(np.uint64)).all()
    assert (O.exp(expx).view(np.uint64) == exp.view(np.uint64)).all()
    print("libm_bits:", x.size, "points;", tp.size, "distinct-ish tree points at 1e-10")


def recip_hard(max_delta=100):
    """cosh's hard reciprocals. For 0.5 ln 2 <= |x| < 22 glibc's cosh is 0.5 t + 0.5 / t with t = exp(|x|). Take a
    53-bit T with T N = 2^106 - delta for an odd N and a small delta > 0: 2^105 / T = N / 2 + delta / (2 T), so 0.5 / t
    for t = T 2^a lies delta 2^-106 (relative) above the midpoint of two doubles -- a division that is not correct to
    about 100 bits before its last rounding gets it wrong. The T come from the divisors of 2^106 - delta (sympy), the x
    from the neighbours of log(t) whose host-libm exp is t exactly, t in [1.4143, 8) (further up 0.5 / t no longer
    moves cosh's last bit). Output: recip_hard_bits.npz (x, host-libm cosh(x), delta)."""
    import math

    from sympy import factorint
    xs, ds = [], []
    for delta in range(1, max_delta + 1):
        n = (1 << 106) - delta
        div = [1]
        for p, k in factorint(n).items():
            div = [d * p ** i for d in div for i in range(k + 1)]
        for T in sorted(div):
            if not ((1 << 52) <= T < (1 << 53) and (n // T) & 1):
                continue
            for a in (-52, -51, -50):
                t = math.ldexp(float(T), a)
                if not 1.4143 <= t < 8.0:
                    continue
                cand = [math.log(t)]
                for _ in range(8):
                    cand = [math.nextafter(cand[0], -math.inf)] + cand + [math.nextafter(cand[-1], math.inf)]
                cand = np.array(cand)
                for x in cand[O.exp(cand, O.HOST_LIBM) == t][:2]:
                    xs.append(float(x))
                    ds.append(delta)
    x = np.array(xs)
    cosh = O.cosh(x, O.HOST_LIBM)
    assert (O.cosh(x).view(np.uint64) == cosh.view(np.uint64)).all()   # the restatement must already agree
    np.savez_compressed(os.path.join(OUT, "recip_hard_bits.npz"), x=x.view(np.uint64), cosh=cosh.view(np.uint64),
                        delta=np.array(ds, np.int64))
    print("recip_hard:", x.size, "points from", len(set(ds)), "values of delta")


def _batch10_part(rng):
    s, e = rng
    a, b = O.batch_bounds(e)
    _, t, lv = O.integrate_batch(a[s:e], b[s:e], 1e-10)
    return int(lv.sum()), int(t.sum())


def batch():
    a, b = O.batch_bounds(10000)
    ar3, t3, l3 = O.integrate_batch(a, b, 1e-3)
    n10 = 200
    ar10, t10, l10 = O.integrate_batch(a[:n10], b[:n10], 1e-10)
    out = {
        "generator": "splitmix64 state0=0x9E3779B97F4A7C15; a=5*u1, b=5*u2 (u=(z>>11)*2^-53), swap if a>b",
        "first_bounds_hex": [[float(x).hex(), float(y).hex()] for x, y in zip(a[:16], b[:16])],
        "n_eps1e-3": 10000,
        "mean_leaves_eps1e-3": float(l3.mean()),
        "sum_leaves_eps1e-3": int(l3.sum()),
        "sum_tasks_eps1e-3": int(t3.sum()),
        "leaves_eps1e-3_first256": [int(v) for v in l3[:256]],
        "area_eps1e-3_first256_hex": [float(v).hex() for v in ar3[:256]],
        "n_eps1e-10": n10,
        "leaves_eps1e-10": [int(v) for v in l10],
        "area_eps1e-10_hex": [float(v).hex() for v in ar10],
    }
    # SURVEY §8d KAT: the first 10 000 draws give mean leaves 711.5 at eps=1e-3
    assert abs(out["mean_leaves_eps1e-3"] - 711.5) < 0.05, out["mean_leaves_eps1e-3"]
    # ... and 153 330.8 at eps=1e-10: the exact sums (3e9 tasks; 8 processes, ~1 min), which the
    # bench's C3 pass checks its first 10 000 integrals against
    from multiprocessing import Pool
    with Pool(8) as pool:
        parts = pool.map(_batch10_part, [(i, min(i + 250, 10000)) for i in range(0, 10000, 250)], chunksize=1)
    out["kat_n_eps1e-10"] = 10000
    out["kat_sum_leaves_eps1e-10"] = sum(p[0] for p in parts)
    out["kat_sum_tasks_eps1e-10"] = sum(p[1] for p in parts)
    assert round(out["kat_sum_leaves_eps1e-10"] / 10000, 1) == 153330.8, out["kat_sum_leaves_eps1e-10"]
    assert out["kat_sum_tasks_eps1e-10"] == 2 * out["kat_sum_leaves_eps1e-10"] - 10000
    with open(os.path.join(OUT, "batch.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("batch: mean leaves 1e-3 =", out["mean_leaves_eps1e-3"], "; first", n10, "at 1e-10 mean",
          float(l10.mean()))


PLUGIN_CONFIGS = [
    # the AQ_F_USER plug-in (ppls_amd/csrc/plugins/aq_user_gauss.h): the reference binary with line 46
    # replaced by `#define F(arg) exp(-(arg)*(arg))` (oracle/Makefile), A = 0, B = 5 unchanged
    ("gauss_eps1e-10", 1e-10, "aquadPartA_gauss_eps1e-10"),
    ("gauss_eps1e-13", 1e-13, "aquadPartA_gauss_eps1e-13"),
]


def plugin():
    """Add the plug-in integrand's trees to trees.json (pinned by the reference binary built with
    that F) and its F bit patterns (host libm exp) to plugin_bits.npz."""
    path = os.path.join(OUT, "trees.json")
    with open(path) as f:
        out = json.load(f)
    for name, eps, ref in PLUGIN_CONFIGS:
        r = O.integrate(O.USER, 0.0, 5.0, eps)
        rec = {"integrand": "gauss", "a": 0.0, "b": 5.0, "eps": eps, "tasks": r.tasks, "leaves": r.leaves,
               "levels": r.levels, "tasks_per_level": r.tasks_per_level, "leaves_per_level": r.leaves_per_level,
               "area_quad": r.area_quad_str, "area_lifo_hex": float(r.area_lifo).hex(),
               "area_lifo_printed": "%f" % r.area_lifo}
        refrun = run_reference(ref, 5)
        assert refrun["tasks_total"] == r.tasks, (name, refrun["tasks_total"], r.tasks)
        assert refrun["area_printed"] == "%f" % (r.area_quad_hi + r.area_quad_lo), (name, refrun["area_printed"])
        ref2 = run_reference(ref, 2)
        assert ref2["tasks_total"] == r.tasks
        assert ref2["area_printed"] == "%f" % r.area_lifo
        rec["reference"] = refrun
        rec["reference_p2"] = ref2
        out[name] = rec
        print(name, r.tasks, r.leaves, r.levels, r.area_quad_str)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    rng = np.random.default_rng(20261016)
    x = np.concatenate([[0.0, -0.0, 2.0 ** -28, 2.0 ** -27.5, 1.0, 5.0, 22.0, 22.7, 26.0, 27.2, 27.3, 28.0, 40.0],
                        rng.uniform(-5.0, 5.0, 4000), rng.uniform(22.0, 27.5, 1000), rng.uniform(-1e-8, 1e-8, 200)])
    F = O.F(x, O.USER, O.HOST_LIBM)
    assert (O.F(x, O.USER).view(np.uint64) == F.view(np.uint64)).all()
    np.savez_compressed(os.path.join(OUT, "plugin_bits.npz"), x=x.view(np.uint64), F=F.view(np.uint64))


def sin_bits():
    """Config 4's F(arg) = sin(1.0/(arg)) from the host glibc 2.35 libm at points of its domain
    [1e-4, 1], log-uniform points across every s_sin.c range of 1/x (|1/x| < 105414350), negative
    points, and both sides of each range boundary of 1/x (0.855469, 2.426265, 105414350)."""
    rng = np.random.default_rng(20261017)
    edges = []
    for e in (0.85546875, 2.4262657165527344, 105414350.0, 0.126, 1.0, 2.0 ** -26):
        for v in (e, np.nextafter(e, 0.0), np.nextafter(e, 2 * e), e * (1 + 1e-9), e * (1 - 1e-9)):
            edges += [1.0 / v, -1.0 / v]
    x = np.concatenate([np.array(edges), rng.uniform(1e-4, 1.0, 8000),
                        np.exp(rng.uniform(np.log(9.5e-9), np.log(10.0), 3000)),
                        -rng.uniform(1e-4, 1.0, 500), [1e-4, 1.0, 0.5, 2.0, 1e-8]])
    F = O.F(x, O.SIN_RECIP, O.HOST_LIBM)
    assert (O.F(x, O.SIN_RECIP).view(np.uint64) == F.view(np.uint64)).all()
    np.savez_compressed(os.path.join(OUT, "sin_bits.npz"), x=x.view(np.uint64), F=F.view(np.uint64))
    print("sin_bits:", x.size, "points")


DEEP_EPS = (("1e-14", 1e-14), ("1e-15", 1e-15), ("1e-16", 1e-16))


def deep():
    """Deep cosh4 trees (eps 1e-14 .. 1e-16, 31 M .. 150 M tasks) pinned by the reference binary
    itself (mpirun -n 5, ~15-80 s each here): its printed task total and Area= line are recorded and
    the oracle's restatement must reproduce both. The oracle adds the accepted count, depth and the
    quad-precision area. Output: deep.json."""
    out = {}
    for tag, eps in DEEP_EPS:
        refrun = run_reference("aquadPartA_eps" + tag, 5)
        r = O.integrate(O.COSH4, 0.0, 5.0, eps, maxlev=128)
        assert refrun["tasks_total"] == r.tasks, (tag, refrun["tasks_total"], r.tasks)
        # the reference's own arrival-order sum (:149) drifts from the exact sum by up to ~1e-13
        # relative at these sizes, which can move its 6th printed decimal: compare within
        # the print rounding plus the north star's 1e-12 relative tolerance
        exact = r.area_quad_hi + r.area_quad_lo
        assert abs(float(refrun["area_printed"]) - exact) <= 5e-7 + 1e-12 * exact, (tag, refrun["area_printed"])
        out["cosh4_eps" + tag] = {
            "integrand": "cosh4", "a": 0.0, "b": 5.0, "eps": eps,
            "tasks": r.tasks, "leaves": r.leaves, "levels": r.levels,
            "tasks_per_level": r.tasks_per_level, "leaves_per_level": r.leaves_per_level,
            "area_quad": r.area_quad_str, "reference": refrun,
        }
        print("deep", tag, r.tasks, r.leaves, r.levels, refrun["area_printed"])
    with open(os.path.join(OUT, "deep.json"), "w") as f:
        json.dump(out, f, indent=1)


# Trees at the edges of the documented domain (include/aquad.h AQ_EINVAL): name, integrand, a, b, eps, and the
# tasks, levels and area the oracle must give (written down from a run of both oracle modes; the step below
# refuses to write anything else).
_ULP1 = float(np.nextafter(1.0, 2.0))
EDGES = [
    ("user_tail_eps0", O.USER, 27.0, 27.5, 0.0, 597, 17, 4.638140063463870e-319),   # every area subnormal
    ("user_zero_eps0", O.USER, 28.0, 40.0, 0.0, 1, 1, 0.0),                         # F underflows to 0 throughout
    ("user_cross", O.USER, -6.0, 6.0, 1e-9, 5371, 14, 1.772453960562458545),
    ("cosh_170", O.COSH4, 169.0, 170.0, 1e280, 82045, 17, 3.2065616394753214e293),
    ("cosh_m170", O.COSH4, -170.0, -169.0, 1e280, 82045, 17, 3.2065616394753214e293),
    ("cosh_pm170", O.COSH4, -170.0, 170.0, 1e285, 4843, 20, 6.532778077271939e293),
    ("cosh_3ulp", O.COSH4, 1.0, 1.0 + 3 * 2.0 ** -52, 0.0, 5, 3, 3.776730228584413e-15),
    ("cosh_ulp", O.COSH4, 1.0, _ULP1, 0.0, 1, 1, 1.2589100761948034e-15),
    ("cosh_0tiny", O.COSH4, 0.0, 2.0 ** -900, 0.0, 1, 1, 1.1830521861667747e-271),
    ("cosh_tiny", O.COSH4, 2.0 ** -900, 2.0 ** -899, 0.0, 1, 1, 1.1830521861667747e-271),
    ("sin_neg", O.SIN_RECIP, -1.0, -1e-3, 1e-8, 11891, 22, -0.50406631068191603),
    ("sin_big", O.SIN_RECIP, 2.0 ** 899, 2.0 ** 900, 1e-3, 9, 4, 0.69377140317542796),
    ("sin_1e-8", O.SIN_RECIP, 1e-8, 1e-6, 1e-9, 715, 11, 2.4829501285150798e-9),
]


def edges():
    """Trees at the edges of the documented domain: cosh^4 at |x| = 170, the Gaussian where F and its areas are
    subnormal or zero, eps = 0, a negative sin(1/x) interval, bounds at 2^-900 and 2^900, intervals of one and three
    ulps. The restated and the host-libm oracle modes must agree on every number and give the counts of EDGES.
    Output: edges.json (bounds and areas also as hex floats)."""
    names = {O.COSH4: "cosh4", O.SIN_RECIP: "sin_recip", O.USER: "gauss"}
    out = {}
    for name, integrand, a, b, eps, tasks, levels, area in EDGES:
        r = O.integrate(integrand, a, b, eps, maxlev=128)
        h = O.integrate(integrand, a, b, eps, mode=O.HOST_LIBM, maxlev=128)
        assert (r.tasks, r.leaves, r.levels, r.tasks_per_level, r.leaves_per_level, r.area_quad_hi, r.area_quad_lo) == \
            (h.tasks, h.leaves, h.levels, h.tasks_per_level, h.leaves_per_level, h.area_quad_hi, h.area_quad_lo), name
        assert (r.tasks, r.levels) == (tasks, levels) and r.tasks == 2 * r.leaves - 1, (name, r.tasks, r.levels)
        got = r.area_quad_hi + r.area_quad_lo
        assert got == area or abs(got - area) <= 4e-16 * abs(area), (name, got, area)   # (the table's 16-17 digits)
        out[name] = {"integrand": names[integrand], "a": a, "b": b, "eps": eps, "a_hex": float(a).hex(),
                     "b_hex": float(b).hex(), "tasks": r.tasks, "leaves": r.leaves, "levels": r.levels,
                     "tasks_per_level": r.tasks_per_level, "leaves_per_level": r.leaves_per_level,
                     "area_quad": r.area_quad_str, "area_hex": float(got).hex()}
        print("edges", name, r.tasks, r.leaves, r.levels, repr(got))
    with open(os.path.join(OUT, "edges.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if not shutil.which(MPIRUN) and not os.path.exists(MPIRUN):
        print("warning: no mpirun; reference stdout will not be recorded")
    O.build()
    which = sys.argv[1:] or ["trees", "plugin", "libm_bits", "sin_bits", "batch", "deep", "edges", "recip_hard"]
    for name in which:
        {"trees": trees, "plugin": plugin, "libm_bits": libm_bits, "sin_bits": sin_bits, "batch": batch,
         "deep": deep, "edges": edges, "recip_hard": recip_hard}[name]()
