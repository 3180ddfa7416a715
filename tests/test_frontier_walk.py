"""The frontier engine's host loop (`frontier_walk` of `ppls_amd/csrc/aq_frontier_walk.h`, what aq_abi.inc
walk_run runs for aq_frontier_integrate / aq_integrate_mesh, aq_integrate_mesh_batch and aq_mesh_refine_batch)
built alone with g++, plain and under AddressSanitizer + UBSan, and run over fake operations driven by a table of
true level sizes: its calls, code and final depth equal a restatement of each entry point's own loop as it stood
before the three shared one -- three separate functions below, each written from its entry point."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "frontier_walk_check.cpp")
INC = [os.path.join(ROOT, "ppls_amd", "csrc"), os.path.join(ROOT, "include")]
SAN = [None, "address,undefined"]
ML = 128            # AQ_MAX_LEVELS
EOVERFLOW = -4      # AQ_EOVERFLOW
CAP = 64            # small, so that clamping is reachable
SYNC = (1, 3, 4)
_built = {}


class Ops:
    """The fake operations: they record the call, a look reads the true size of its depth, and the `at`-th call
    of `kind` returns `code`."""

    def __init__(self, sizes, fail):
        self.sizes, self.fail, self.calls, self.seen = sizes, fail, [], {"seed": 0, "step": 0, "look": 0}

    def _call(self, op, depth, n):
        self.calls.append((op, depth, n))
        kind, at, code = self.fail
        self.seen[op] += 1
        return code if op == kind and self.seen[op] - 1 == at else 0

    def seed(self, depth, ns):
        return self._call("seed", depth, ns)

    def step(self, depth, n_in):
        return self._call("step", depth, n_in)

    def look(self, depth):
        now = self.sizes.get(depth, 0)
        return self._call("look", depth, now), now


def integrate_loop(ops, cap, max_depth, sync_every):
    """frontier_run: the narrow top ends at min(13, max_depth - 1); chained steps from there."""
    depth = min(13, max_depth - 1)
    depth = max(depth, 0)
    bound = min(1 << depth, cap)
    since, rc = 0, 0
    while depth <= max_depth and depth < ML:
        rc = ops.step(depth, bound)
        if rc:
            break
        depth += 1
        bound = min(2 * bound, cap)
        since += 1
        if since == sync_every:
            since = 0
            rc, n = ops.look(depth)
            if rc:
                break
            if n == 0:
                break
            if n > cap:
                rc = EOVERFLOW
                break
            bound = n
    return rc, depth


def batch_loop(ops, n, cap, max_depth, sync_every):
    """aq_integrate_mesh_batch: from depth 0, which holds at most n records."""
    depth, since, rc = 0, 0, 0
    bound = n
    while depth <= max_depth and depth < ML:
        rc = ops.step(depth, bound)
        if rc:
            break
        depth += 1
        bound = min(2 * bound, cap)
        since += 1
        if since == sync_every:
            since = 0
            rc, now = ops.look(depth)
            if rc:
                break
            if now == 0:
                break
            if now > cap:
                rc = EOVERFLOW
                break
            bound = now
    return rc, depth


def refine_table(failing):
    """aq_mesh_refine_batch's segment arithmetic over the depth table (failing leaves per depth): the seed records
    of depth e are [seg[e - 1], seg[e]); the first and the last depth that has seeds."""
    seg, first_depth, last_depth, pre = [0] * (ML + 1), -1, -1, 0
    for d in range(ML):
        seg[d] = 2 * pre
        if failing.get(d, 0):
            if first_depth < 0:
                first_depth = d + 1
            last_depth = d + 1
        pre += failing.get(d, 0)
    seg[ML] = 2 * pre
    return seg, first_depth, last_depth


def refine_loop(ops, failing, cap, max_depth, sync_every):
    """aq_mesh_refine_batch: from the first depth that has seeds; a depth's seeds join before its step; an empty
    level ends the loop only when no deeper segment is left."""
    seg, first_depth, last_depth = refine_table(failing)

    def seeds_of(depth):
        return seg[depth] - seg[depth - 1] if 1 <= depth <= ML else 0

    depth, since = (0 if first_depth < 0 else first_depth), 0
    bound, rc = 0, 0
    while first_depth >= 0 and depth <= max_depth and depth < ML:
        ns = seeds_of(depth)
        if ns:
            rc = ops.seed(depth, ns)
            if rc:
                break
        n_in = min(bound + ns, cap)
        rc = ops.step(depth, n_in)
        if rc:
            break
        depth += 1
        bound = min(2 * n_in, cap)
        if bound == 0 and depth > last_depth:
            break
        since += 1
        if since == sync_every:
            since = 0
            rc, now = ops.look(depth)
            if rc:
                break
            if now == 0 and depth > last_depth:
                break
            if now > cap:
                rc = EOVERFLOW
                break
            bound = now
    return rc, depth


NOFAIL = ("", 0, 0)


def _want(case):
    """(calls, rc, final depth) of the case's own loop, and the walk's description of it."""
    ops = Ops(case["sizes"], case.get("fail", NOFAIL))
    cap, max_depth, sync = case.get("cap", CAP), case["max_depth"], case["sync"]
    if case["shape"] == "integrate":
        rc, depth = integrate_loop(ops, cap, max_depth, sync)
        start = max(min(13, max_depth - 1), 0)
        walk = (start, min(1 << start, cap), -1, None)
    elif case["shape"] == "batch":
        rc, depth = batch_loop(ops, case["n"], cap, max_depth, sync)
        walk = (0, case["n"], -1, None)
    else:
        rc, depth = refine_loop(ops, case["failing"], cap, max_depth, sync)
        _, first_depth, last_depth = refine_table(case["failing"])
        walk = (max(first_depth, 0), 0, last_depth, {d + 1: 2 * v for d, v in case["failing"].items()})
    return ops.calls, rc, depth, walk


def _line(case):
    start, bound, last_seed, seeds = _want(case)[3]
    kind, at, code = case.get("fail", NOFAIL)
    words = [start, bound, case.get("cap", CAP), case["max_depth"], case["sync"], last_seed,
             {"": 0, "seed": 1, "step": 2, "look": 3}[kind], at, code, len(case["sizes"])]
    for d, v in sorted(case["sizes"].items()):
        words += [d, v]
    words.append(-1 if seeds is None else len(seeds))
    for d, v in sorted((seeds or {}).items()):
        words += [d, v]
    return " ".join(str(x) for x in words)


def _exe(san, tmp_path_factory):
    if san not in _built:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        out = str(tmp_path_factory.mktemp("frontier_walk") / "frontier_walk_check")
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", INC[0], "-I", INC[1], SRC, "-o", out]
        if san:
            cmd.insert(1, "-fsanitize=" + san)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode and san:
            pytest.skip("sanitizer runtime unavailable: " + r.stderr[-400:])
        assert r.returncode == 0, r.stderr[-2000:]
        _built[san] = out
    return _built[san]


def _walks(exe, tmp_path, cases):
    """[(calls, rc, final depth)] of the walk for every case, through one file."""
    path = tmp_path / "cases.txt"
    path.write_text("".join(_line(c) + "\n" for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out, calls = [], []
    for ln in r.stdout.splitlines():
        d = json.loads(ln)
        if "op" in d:
            calls.append((d["op"], d["depth"], d["n"]))
        else:
            out.append((calls, d["rc"], d["depth"]))
            calls = []
    assert len(out) == len(cases) and not calls
    return out


def _dying(start, die_at, width=5):
    """True sizes: `width` records a level from `start` on, none from die_at on."""
    return {d: width for d in range(start, die_at)}


def _plain_cases(shape, start, max_depth, **kw):
    """The endings the integrate and the batch shape share, for every sync_every: the frontier dying exactly at a
    look and between looks, a look that reads more than cap, max_depth reached with records left."""
    out = []
    for sync in SYNC:
        base = dict(shape=shape, sync=sync, **kw)
        for die_at in (start + 2 * sync, start + 2 * sync + 1, start + 3 * sync - 1, start + 1):
            out.append(dict(base, max_depth=max_depth, sizes=_dying(start, die_at), ending="dies"))
        over = _dying(start, start + 2 * sync)
        over[start + 2 * sync] = CAP + 1
        out.append(dict(base, max_depth=max_depth, sizes=over, ending="overflow"))
        for md in (max_depth, start + 2 * sync - 1, start + 2 * sync, start + 2 * sync + 1):   # (a look beside the end)
            out.append(dict(base, max_depth=md, sizes=_dying(start, ML + 2), ending="depth"))
        for kind, at in (("step", 0), ("step", 2 * sync), ("look", 0), ("look", 1)):
            out.append(dict(base, max_depth=max_depth, sizes=_dying(start, ML + 2), fail=(kind, at, -77), ending="fail"))
    return out


def _cases():
    out = []
    # (a) the integrate shape: the narrow top ends at 13, or at 0 under a small max_depth
    out += _plain_cases("integrate", 13, 40)
    out += _plain_cases("integrate", 13, ML - 1)
    for sync in SYNC:   # max_depth 1: no narrow top, the walk is levels 0 and 1
        base = dict(shape="integrate", sync=sync, max_depth=1, ending="small")
        out += [dict(base, sizes=sizes) for sizes in ({}, {1: 2}, {1: 2, 2: 4}, {1: CAP + 1}, {1: 2, 2: CAP + 1})]
        out += [dict(base, sizes={1: 2, 2: 4}, fail=fail) for fail in (("step", 0, -77), ("step", 1, -77), ("look", 0, -77))]
    # (b) the batch shape
    for n in (1, 5, CAP):
        out += _plain_cases("batch", 0, 30, n=n)
    out += _plain_cases("batch", 0, ML - 1, n=5)
    # (c) the refine shape (failing leaves of depth d seed depth d + 1)
    for sync in SYNC:
        base = dict(shape="refine", sync=sync, max_depth=40)
        # seeds at depths 3 and 7, the frontier empty at 5 and 6: on to 7
        # (a look reads what the steps left at its depth: the seeds of that depth join behind it)
        out.append(dict(base, failing={2: 2, 6: 1}, sizes={4: 3, 8: 1}, ending="gap"))
        out.append(dict(base, failing={2: 2, 6: 1}, sizes={}, ending="gap"))
        # bound + ns above cap: clamped
        out.append(dict(base, failing={1: 25, 2: 30, 3: 30}, sizes={d: CAP for d in range(2, 12)}, ending="clamp"))
        out.append(dict(base, failing={1: 25, 2: 30}, sizes={2: 50, 3: CAP + 1, 4: CAP + 1, 5: CAP + 1, 6: CAP + 1},
                        ending="overflow"))
        # seeds only at the last allowed depth: max_depth, and the last level there is
        out.append(dict(base, max_depth=9, failing={8: 3}, sizes={9: 6, 10: 4}, ending="last"))
        out.append(dict(base, max_depth=ML - 1, failing={ML - 2: 3}, sizes={ML - 1: 6, ML: 4}, ending="last"))
        out.append(dict(base, max_depth=ML - 1, failing={ML - 1: 3}, sizes={ML: 6}, ending="past"))
        # max_depth reached with records left; the frontier dying at and between looks behind the last seeds
        out.append(dict(base, max_depth=12, failing={2: 2}, sizes=_dying(3, ML + 2), ending="depth"))
        for die_at in (3 + 2 * sync, 3 + 2 * sync + 1, 4):
            out.append(dict(base, failing={2: 2}, sizes=_dying(3, die_at), ending="dies"))
        # no seeds at all
        out.append(dict(base, failing={}, sizes={}, ending="none"))
        for kind, at in (("seed", 0), ("seed", 1), ("step", 0), ("step", 3), ("look", 0), ("look", 1)):
            out.append(dict(base, failing={2: 2, 6: 1}, sizes=_dying(3, ML + 2), fail=(kind, at, -77), ending="fail"))
    return out


@pytest.mark.parametrize("san", SAN)
def test_walk_is_each_entry_points_loop(tmp_path, tmp_path_factory, san):
    cases = _cases()
    got = _walks(_exe(san, tmp_path_factory), tmp_path, cases)
    for case, (calls, rc, depth) in zip(cases, got):
        want_calls, want_rc, want_depth, _ = _want(case)
        assert (calls, rc, depth) == (want_calls, want_rc, want_depth), case
    assert {c["shape"] for c in cases} == {"integrate", "batch", "refine"} and {c["sync"] for c in cases} == set(SYNC)


def test_cases_reach_every_ending():
    """The restated loops on the cases above end the way each case is named for (so the comparison with the walk
    covers those endings)."""
    seen = set()
    for case in _cases():
        calls, rc, depth, walk = _want(case)
        shape, ending, sizes = case["shape"], case["ending"], case["sizes"]
        seen.add((shape, ending, case["sync"]))
        looks = [c for c in calls if c[0] == "look"]
        if ending == "dies":
            assert rc == 0 and sizes.get(depth, 0) == 0
            if shape != "refine":   # (these two know an empty level only from a look)
                assert calls[-1][0] == "look" and calls[-1][2] == 0
        elif ending == "overflow":
            assert rc == EOVERFLOW and calls[-1][0] == "look" and calls[-1][2] > CAP
        elif ending == "depth":
            assert rc == 0 and depth == case["max_depth"] + 1 and sizes[depth] > 0
        elif ending == "fail":
            kind, at, code = case["fail"]
            assert rc == code and calls[-1][0] == kind and sum(c[0] == kind for c in calls) == at + 1
        elif ending == "gap":
            assert rc == 0 and ("seed", 7, 2) in calls and ("step", 7, 2) in calls
            assert any(c[0] == "look" and c[1] <= 7 and c[2] == 0 for c in calls)   # ... and the loop went on
            assert [c for c in calls if c[0] == "step" and c[1] in (5, 6)]
        elif ending == "clamp":
            assert rc == 0 and ("seed", 3, 60) in calls and ("step", 3, CAP) in calls and depth > 4
        elif ending == "last":
            assert rc == 0 and [c[:2] for c in calls if c[0] != "look"] == [("seed", depth - 1), ("step", depth - 1)]
            assert depth == case["max_depth"] + 1 and sizes[depth] > 0
        elif ending == "past":   # seeds of depth AQ_MAX_LEVELS: no level steps them
            assert (calls, rc, depth) == ([], 0, ML)
        elif ending == "small":
            assert walk[:2] == (0, 1) and depth <= 2
        elif ending == "none":
            assert (calls, rc, depth, walk[:3]) == ([], 0, 0, (0, 0, -1))
        assert all(c[2] <= case.get("cap", CAP) for c in calls if c[0] == "step")
        assert all(b[1] - a[1] == case["sync"] for a, b in zip(looks, looks[1:]))
    for shape in ("integrate", "batch", "refine"):
        for sync in SYNC:
            assert {e for s, e, y in seen if (s, y) == (shape, sync)} >= {"dies", "overflow", "depth", "fail"}, (shape, sync)
    assert {e for s, e, y in seen if s == "refine"} >= {"gap", "clamp", "last", "none"}
