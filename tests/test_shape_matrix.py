"""The launch-shape matrix (tests/shape_matrix.py) reaches every instance of the persistent kernel: each case's
launches go through plan_launch itself (tests/native/launch_plan_check.cpp --plan, g++ alone, grid 256) in the
order the GPU test issues them, the hint carried from launch to launch, and the set of (integrand, variant, ERR)
reached must equal shape_matrix.REQUIRED. The oracle's side of the matrix -- the degenerate rows' counts, the time
of a whole batch -- is checked here as well, not on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import shape_matrix as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "launch_plan_check.cpp")
INC = [os.path.join(ROOT, "ppls_amd", "csrc"), os.path.join(ROOT, "include")]
W = sm.GRID * sm.NW


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("plan") / "launch_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", INC[0], "-I", INC[1], SRC, "-o", exe]
    # under ASan + UBSan where the runtime is there (a stand-alone host program), else plain
    r = subprocess.run(cmd[:1] + ["-fsanitize=address,undefined"] + cmd[1:], capture_output=True, text=True)
    if r.returncode:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def plan(reqs):
        path = exe + ".rows"
        with open(path, "w") as f:
            f.write(sm.plan_rows(reqs))
        r = subprocess.run([exe, "--plan", path], capture_output=True, text=True, timeout=60, env=env)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        plans = sm.parse_plans(r.stdout)
        assert len(plans) == len(reqs)
        return plans
    plan.exe = exe
    return plan


def _reached(planner, cases):
    """(case, request, plan) of every launch of the accepted cases, the breakers left out."""
    out = []
    for c in cases:
        if c.refused:
            continue
        reqs = sm.requests(c, W)
        plans = planner(reqs)
        # the breaker: a fresh hint made valid (a context that collects diagnostics has no heap instance)
        assert plans[0]["variant"] == ("DIAG" if c.diag else "HEAP") and plans[0]["adaptive"] == 2
        out += [(c, r, p) for r, p in zip(reqs[1:], plans[1:])]
    return out


@pytest.fixture(scope="module")
def reached(planner):
    return _reached(planner, sm.CASES)


def _triples(reached):
    return {(c.fid, p["variant"], bool(p["err"])) for c, _, p in reached}


def test_constants_are_the_planners(planner):
    """shape_matrix restates a few constants of the launch shape: they are the headers'."""
    import json
    k = json.loads(subprocess.run([planner.exe, "--constants"], capture_output=True, text=True, check=True).stdout)
    assert (k["NW"], k["PCU_MAXK"], k["SYNC_SLOT"], k["MAXK"]) == (sm.NW, sm.PCU_MAXK, sm.SYNC_SLOT, 1 << 18)
    src = open(os.path.join(INC[0], "aq_shape.h")).read() + open(os.path.join(INC[0], "aq_launch_plan.h")).read() + \
        open(os.path.join(INC[0], "aq_batch_plan.h")).read() + open(os.path.join(INC[0], "aq_abi.inc")).read()
    for text in ("constexpr int ERR_NW = %d;" % sm.ERR_NW, "constexpr int BATCH_SORT_MIN = %d;" % sm.BATCH_SORT_MIN,
                 "#define AQ_BATCH_FIRST %d " % sm.BATCH_FIRST,
                 "enum class Variant : int { %s };" % ", ".join(sm.VARIANTS)):
        assert text in src, text


def test_every_launch_is_planned(reached):
    assert all(p["rc"] == 0 for _, _, p in reached)
    # a case's launches run twice exactly where the planner sizes jobs adaptively
    for c in sm.CASES:
        mine = [p for cc, _, p in reached if cc is c]
        if not c.refused and c.entry not in sm.BATCH_ENTRIES and len(set(c.ks)) == 1:
            assert (len(c.ks) == 2 and c.nshards == 1) == (mine[0]["adaptive"] != 0), c.id


def test_matrix_reaches_the_required_instances(reached):
    got = _triples(reached)
    assert got == sm.REQUIRED, (sorted(sm.REQUIRED - got), sorted(got - sm.REQUIRED))
    # the planner never picks the lone instance for sin(1/x): its synchronous call runs the per-CU one
    sync = [p for c, r, p in reached if c.fid == sm.SIN_RECIP and r["first_slot"] == sm.SYNC_SLOT and not c.diag]
    assert sync and all(p["variant"] == "PCU" and p["nwt"] == sm.NW for p in sync)
    assert not any(p["variant"] == "LONE" for c, _, p in reached if c.fid == sm.SIN_RECIP)
    lone = [p for c, _, p in reached if p["variant"] == "LONE"]
    assert lone and all(p["nwt"] == 8 and p["shares"] == sm.GRID * 8 for p in lone)


def test_removing_a_case_is_noticed(planner, reached):
    """The coverage assertion has teeth: without the cases that reach a required triple, the set differs."""
    for triple in sorted(sm.REQUIRED):
        keep = [c for c in sm.CASES if not any(cc is c and (cc.fid, p["variant"], bool(p["err"])) == triple
                                                for cc, _, p in reached)]
        assert len(keep) < len(sm.CASES), triple
    # ... and through the planner again for one of them
    triple = (sm.USER, "HEAP", True)
    keep = [c for c in sm.CASES if not (c.fid == sm.USER and c.err)]
    assert triple not in _triples(_reached(planner, keep))


def test_other_plan_fields(reached):
    for v in ("HEAP", "PLAIN"):
        for err in (False, True):
            want = {2, 3, 7} if not err else {2, 7} if v == "HEAP" else {2, 3}
            assert want <= {p["adaptive"] for _, _, p in reached if p["variant"] == v and bool(p["err"]) == err}, (v, err)
    for fid in sm.FIDS:
        assert {2, 3, 7} <= {p["adaptive"] for c, _, p in reached if c.fid == fid and p["variant"] == "HEAP"}, fid
        assert {2, 3, 7} <= {p["adaptive"] for c, _, p in reached if c.fid == fid and p["variant"] == "PLAIN"}, fid
    assert {p["static_jobs"] for _, _, p in reached} == {0, 1}
    assert {p["tail_mult"] > 1 for _, _, p in reached} == {False, True}
    sin = [(c, r, p) for c, r, p in reached if c.fid == sm.SIN_RECIP and not c.err and not c.diag]
    # its unsharded per-CU launches seed one level deeper, its sharded ones keep the oracle's partition. (At grid
    # 256 the deeper level always fits the seeding's 128 nodes: V <= 3072 shares give D <= 13 and at most 8
    # positions per share, (D + 2) * 8 + 2 <= 122 -- so "not deeper" is reached through the shards.)
    pcu = [(r, p) for _, r, p in sin if p["per_cu"]]
    assert {p["deeper"] for r, p in pcu if r["nshards"] == 1 and not r["shard_array"]} == {1}
    assert {p["deeper"] for r, p in pcu if r["nshards"] > 1} == {0}
    assert {r["shard_array"] for r, p in pcu if r["nshards"] > 1} == {0, 1}
    assert not any(p["deeper"] for c, _, p in reached if c.fid != sm.SIN_RECIP)
    # its deal of few whole integrals: W shares each up to 4 integrals, about W / k from 5 on (PCU either way)
    few = {r["k"]: p for _, r, p in sin if p["per_cu"] and r["nshards"] == 1 and r["first_slot"] == 0}
    assert set(few) == {1, 2, 4, 5, 11}
    assert [few[k]["shares"] for k in (1, 2, 4)] == [W, W, W] and few[5]["shares"] == few[11]["shares"] == W // 2
    cosh = {r["k"]: p for c, r, p in reached if c.fid == sm.COSH4 and p["variant"] == "PCU" and r["nshards"] == 1 and
            r["first_slot"] == 0 and not p["err"]}
    assert [cosh[k]["shares"] for k in (2, 4, 5, 11)] == [W // 2, W // 4, W // 2, W // 2]
    # few integrals in slots past the per-workgroup words: the heap instance with the static deal, no per-CU counts
    high = [p for c, r, p in reached if r["first_slot"] == 20000]
    assert len(high) == 4 and all(p["variant"] == "HEAP" and p["static_jobs"] == 1 and p["per_cu"] == 0 and
                                  p["adaptive"] == 0 for p in high)
    # the batch front end's launches: the heap instance, whatever their size; a fresh call's sorted chunks preset
    for c, r, p in reached:
        if c.entry in sm.BATCH_ENTRIES:
            assert p["variant"] == "HEAP" and (p["adaptive"] == 7) == bool(r["preset"] or r is not _first(reached, c)), c.id


def _first(reached, case):
    return next(r for c, r, _ in reached if c is case)


def test_refusals_are_the_headers():
    """include/aquad.h: AQ_F_PARAM goes through the _params and _err entry points only; every other entry point
    refuses it with AQ_EINVAL. Nothing else in the matrix is refused, and every plain entry point is tried."""
    refused = [c for c in sm.CASES if c.refused]
    assert {c.entry for c in refused} == set(sm.PLAIN_ENTRY.values()) | {"integrate_mixed_async"}
    assert all(c.fid == sm.PARAM and c.refused == sm.AQ_EINVAL for c in refused)
    for c in sm.CASES:
        if c.fid == sm.PARAM and not c.refused:
            assert c.entry in tuple(sm.PARAM_ENTRY.values()) + tuple(sm.ERR_ENTRY.values()), c.id
    hdr = open(os.path.join(INC[1], "aquad.h")).read()
    assert "aq_*_params entry points only -- every other entry point refuses it" in hdr


def test_every_k_and_entry_point_occurs():
    for fid in sm.FIDS:
        many = {k for c in sm.CASES if c.fid == fid and not c.refused and not c.err and not c.diag and c.nshards == 1 and
                c.first_slot == 0 and "many" in c.entry for k in c.ks}
        assert many == set(sm.KSYMS), fid
        assert {k for c in sm.CASES if c.fid == fid and c.err and "many" in c.entry for k in c.ks} == {"5", "16", "W+64"}
    assert {c.entry for c in sm.CASES} == set(sm.PLAIN_ENTRY.values()) | set(sm.PARAM_ENTRY.values()) | \
        {"integrate_many_err_async", "integrate_batch_err", "integrate_mixed_async"}
    # the batch cases' chunks: every one holds the degenerate rows; an unsorted first chunk, sorted later ones
    # and a short unsorted last chunk occur
    shapes = set()
    for c in sm.CASES:
        if c.entry in sm.BATCH_ENTRIES and not c.refused:
            n = sm.k_of(c.ks[0], W)
            idx, chunks = sm.case_rows(c, n), sm.case_chunks(c, n)
            assert sum(m for m, _, _ in chunks) == n == idx.size
            for m, srt, off in chunks:
                assert set(sm.DEG_AT[:len(sm.degenerate_kinds(c.fid))]) <= set(idx[off:off + m].tolist()), (c.id, off)
            shapes.add(tuple((m, srt) for m, srt, _ in chunks))
    assert ((32, False), (64, True), (128, True), (256, True), (512, True), (1024, True), (1080, True), (40, False)) in shapes
    assert ((64, True), (128, True), (256, True), (512, True), (1024, True), (1152, True)) in shapes
    assert ((W + 64, True),) in shapes and ((W + 64, False),) in shapes


@pytest.mark.parametrize("fid", sm.FIDS)
def test_degenerate_rows_and_oracle_budget(fid, oracle):
    """The oracle on the integrand's W + 64 rows: an empty interval is one task of area 0, a one-ulp interval one
    task; every row is a whole tree (T = 2 L - 1); the rows of every launch size hold the degenerate rows; and the
    fixed integrands' batch run (oracle.integrate_batch, which the per-row reference restates with histograms)
    stays within the budget."""
    n = W + 64
    a, b, theta = sm.master(fid, n)
    ref = sm.reference(fid, n)
    assert (ref["tasks"] == 2 * ref["leaves"] - 1).all() and (ref["levels"] >= 1).all()
    assert (ref["tasks_per_level"].sum(1) == ref["tasks"]).all() and (ref["leaves_per_level"].sum(1) == ref["leaves"]).all()
    at = dict(zip(sm.degenerate_kinds(fid), sm.DEG_AT))
    i = at["empty"]
    assert a[i] == b[i] and (ref["tasks"][i], ref["levels"][i], ref["area"][i]) == (1, 1, 0.0)
    i = at["ulp"]
    assert b[i] == np.nextafter(a[i], np.inf) and (ref["tasks"][i], ref["levels"][i]) == (1, 1) and ref["area"][i] != 0.0
    i = at["narrow"]
    assert a[i] < b[i] < a[i] + 1e-8 and ref["tasks"][i] >= 1
    if fid != sm.SIN_RECIP:
        i = at["zero_tiny"]
        assert (a[i], b[i]) == (0.0, 2.0 ** -900) and ref["tasks"][i] == 1 and ref["area"][i] > 0.0
        i = at["straddle"]
        assert a[i] < 0.0 < b[i] and ref["tasks"][i] > 1
    else:
        assert a.min() >= 1e-3 > 1e-8
    # trees of many sizes share the launches: the rows are no degenerate workload themselves
    assert ref["tasks"].max() > 50 * np.median(ref["tasks"]) or ref["tasks"].max() > 1000
    for sym in sm.KSYMS:
        k = sm.k_of(sym, W)
        idx = sm.rows(fid, k)
        assert idx.size == k and len(set(idx.tolist())) == k
        if k >= 11:
            assert set(at.values()) <= set(idx.tolist())
        elif k > 1:
            assert idx[:min(k, len(at))].tolist() == list(at.values())[:k]
    if fid != sm.PARAM:
        import time
        best = None
        for _ in range(2):   # (the faster of two runs: the budget is the oracle's, not the machine's other load)
            t0 = time.perf_counter()
            area, tasks, leaves = oracle.integrate_batch(a, b, sm.EPS[fid], integrand=fid)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print(sm.FID_NAME[fid], "oracle batch of", n, "rows:", int(tasks.sum()), "tasks,", round(best, 3), "s")
        assert (tasks == ref["tasks"]).all() and (leaves == ref["leaves"]).all()
        assert np.array_equal(area, ref["area"])
        assert best < sm.ORACLE_BUDGET_S, best
    else:
        print("param walk of", n, "rows:", int(ref["tasks"].sum()), "tasks,", round(ref["seconds"], 3), "s")
        assert ref["seconds"] < sm.ORACLE_BUDGET_S, ref["seconds"]
    # the ERR cases' walker agrees with the oracle on the same rows
    w = sm.err_walk(fid, n)
    assert np.array_equal(w["tasks"], ref["tasks"]) and np.array_equal(w["leaves"], ref["leaves"])
    assert np.array_equal(w["levels"], ref["levels"])
    assert (np.abs(w["area"] - ref["area"]) <= np.spacing(np.abs(ref["area"]))).all()
    i = at["empty"]
    assert w["err_abs"][i] == 0.0 and w["err_signed"][i] == 0.0
