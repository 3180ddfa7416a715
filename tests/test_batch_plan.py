"""The batch front end's pipeline plan (`batch_plan` of `ppls_amd/csrc/aq_batch_plan.h`, what `batch_run` walks)
built alone with g++, plain and under AddressSanitizer + UBSan: (a) the plan against a restatement of the schedule,
two step lists pinned by hand; (b) a happens-before check over the printed plan and its resource table
(batch_plan_util.hazards) -- every two steps that touch the same buffer, one of them writing, are ordered -- which
must report a hazard when any needed wait is dropped, and none for the one wait the host's own synchronisation
implies."""
import itertools
import json

import pytest

from batch_plan_util import MAXK, SAN, brief as _brief, exe as _exe, hazards as _hazards, run as _run, run_cases

GRID = list(itertools.product([1, 63, 64, 200, 468, 1000, 3000, MAXK + 1, 2 * MAXK + 1000, 1000003, 5 * MAXK + 7],
                              [0, 16, 32, 64, 1024, 131072], [0, 20, 4096], [1, 0]))


def _plans(exe, tmp_path, cases, theta=1, err=1, fresh=1):
    """{(n, first, last, sort): (chunks, steps)}; a step is a dict of kind, chunk, stream, sorted, preset, waits,
    record and uses [[mode, resource, instance]]."""
    out = {}
    for case, p in zip(cases, run_cases(exe, "plan", [("host",) + case + (theta, err, fresh) for case in cases], tmp_path)):
        assert p["first_slot"] == [0] * len(p["chunks"]) and p["n_events"] == 4 * len(p["chunks"]) + 2
        for s in p["steps"]:
            s["sorted"], s["preset"] = (bool(s["chunk"] >= 0 and p[k][s["chunk"]]) for k in ("sorted", "preset"))
        out[case] = (p["chunks"], p["steps"])
    return out


def _chunks_rule(n, first, last):
    out, size = [], min(first, MAXK) if first else MAXK
    while n - sum(out) > size:
        out.append(size)
        size = min(2 * size, MAXK)
    rem = n - sum(out)
    if last and rem > 2 * last:
        return out + [rem - last, last]
    return out + [rem] if rem else out


def _schedule(chunks, sort):
    """The schedule as batch_run issued it before it walked a plan: the call's set-up, chunk 0's bounds, then per
    chunk its launch and gather, the next chunk's bounds (and size order), its copy back, and the previous chunk's
    rows on the host."""
    nc, steps = len(chunks), []
    srt = [bool(sort) and m >= 64 for m in chunks]

    def bounds(c):
        steps.append(("stage", c, "host", (), None))
        # (the ring slot chunk c - 2 used: free at its gather)
        steps.append(("h2d", c, "ctx" if c == 0 else "h2d", (f"gath:{c - 2}",) if c >= 2 else (), f"h2d:{c}"))
        if srt[c]:
            waits = (f"h2d:{c}",)
            if c == 1:   # the counts chunk 0's scatter zeroed -- or the call, behind an unsorted chunk 0
                waits += ("pre:0" if srt[0] else "zero",)
            steps.append(("pre", c, "ctx" if c == 0 else "pre", waits, f"pre:{c}"))

    steps.append(("start", -1, "ctx", (), "start"))
    steps.append(("fence", -1, "pre", ("start",), None))
    if sort:
        steps.append(("zero", -1, "ctx", (), None if srt[0] else "zero"))
    bounds(0)
    for c in range(nc):
        steps.append(("launch", c, "ctx", (f"pre:{c}" if srt[c] else f"h2d:{c}",), None))
        steps.append(("gather", c, "ctx", (f"d2h:{c - 2}",) if c >= 2 else (), f"gath:{c}"))
        if c + 1 < nc:
            bounds(c + 1)
        steps.append(("d2h", c, "ctx" if c + 1 == nc else "d2h", (f"gath:{c}",), f"d2h:{c}"))
        if c > 0:
            steps.append(("wait", c - 1, "host", (f"d2h:{c - 1}",), None))
            steps.append(("unpack", c - 1, "host", (), None))
    steps.append(("drain", -1, "host", (), None))
    steps.append(("unpack", nc - 1, "host", (), None))
    return srt, steps


@pytest.mark.parametrize("san", SAN)
def test_plan_is_todays_schedule(tmp_path, tmp_path_factory, san):
    exe = _exe(san, tmp_path_factory)
    k = json.loads(_run(exe, "--constants"))
    assert k == {"MAXK": MAXK, "PCU_MAXK": 12, "NPARTS": 16384, "BATCH_SORT_MIN": 64}
    plans = _plans(exe, tmp_path, GRID)
    assert len(plans) == 396
    for (n, first, last, sort), (chunks, steps) in plans.items():
        assert chunks == _chunks_rule(n, first, last), (n, first, last)
        srt, want = _schedule(chunks, sort)
        assert _brief(steps) == want, (n, first, last, sort)
        for s in steps:
            assert s["sorted"] == (s["chunk"] >= 0 and srt[s["chunk"]])
        # a fresh workload: the sorted chunks are preset until a launch of >= PCU_MAXK rows has measured a hint
        fresh = True
        for c, m in enumerate(chunks):
            assert {s["preset"] for s in steps if s["chunk"] == c} == {fresh and srt[c]}, (n, first, last, sort, c)
            fresh = fresh and m < 12
    # by hand: an unsorted chunk 0, so chunk 1's pre-pass waits for the zeroing ...
    chunks, steps = plans[(200, 32, 0, 1)]
    assert chunks == [32, 64, 104]
    assert _brief(steps) == [
        ("start", -1, "ctx", (), "start"), ("fence", -1, "pre", ("start",), None), ("zero", -1, "ctx", (), "zero"),
        ("stage", 0, "host", (), None), ("h2d", 0, "ctx", (), "h2d:0"),
        ("launch", 0, "ctx", ("h2d:0",), None), ("gather", 0, "ctx", (), "gath:0"),
        ("stage", 1, "host", (), None), ("h2d", 1, "h2d", (), "h2d:1"), ("pre", 1, "pre", ("h2d:1", "zero"), "pre:1"),
        ("d2h", 0, "d2h", ("gath:0",), "d2h:0"),
        ("launch", 1, "ctx", ("pre:1",), None), ("gather", 1, "ctx", (), "gath:1"),
        ("stage", 2, "host", (), None), ("h2d", 2, "h2d", ("gath:0",), "h2d:2"), ("pre", 2, "pre", ("h2d:2",), "pre:2"),
        ("d2h", 1, "d2h", ("gath:1",), "d2h:1"), ("wait", 0, "host", ("d2h:0",), None), ("unpack", 0, "host", (), None),
        ("launch", 2, "ctx", ("pre:2",), None), ("gather", 2, "ctx", ("d2h:0",), "gath:2"),
        ("d2h", 2, "ctx", ("gath:2",), "d2h:2"), ("wait", 1, "host", ("d2h:1",), None), ("unpack", 1, "host", (), None),
        ("drain", -1, "host", (), None), ("unpack", 2, "host", (), None)]
    assert [s["preset"] for s in steps if s["kind"] == "pre"] == [False, False]   # chunk 0's launch measured the hint
    # ... and every ring reused at both parities, an unsorted last chunk behind sorted ones
    chunks, steps = plans[(468, 64, 0, 1)]
    assert chunks == [64, 128, 256, 20]
    assert _brief(steps) == [
        ("start", -1, "ctx", (), "start"), ("fence", -1, "pre", ("start",), None), ("zero", -1, "ctx", (), None),
        ("stage", 0, "host", (), None), ("h2d", 0, "ctx", (), "h2d:0"), ("pre", 0, "ctx", ("h2d:0",), "pre:0"),
        ("launch", 0, "ctx", ("pre:0",), None), ("gather", 0, "ctx", (), "gath:0"),
        ("stage", 1, "host", (), None), ("h2d", 1, "h2d", (), "h2d:1"), ("pre", 1, "pre", ("h2d:1", "pre:0"), "pre:1"),
        ("d2h", 0, "d2h", ("gath:0",), "d2h:0"),
        ("launch", 1, "ctx", ("pre:1",), None), ("gather", 1, "ctx", (), "gath:1"),
        ("stage", 2, "host", (), None), ("h2d", 2, "h2d", ("gath:0",), "h2d:2"), ("pre", 2, "pre", ("h2d:2",), "pre:2"),
        ("d2h", 1, "d2h", ("gath:1",), "d2h:1"), ("wait", 0, "host", ("d2h:0",), None), ("unpack", 0, "host", (), None),
        ("launch", 2, "ctx", ("pre:2",), None), ("gather", 2, "ctx", ("d2h:0",), "gath:2"),
        ("stage", 3, "host", (), None), ("h2d", 3, "h2d", ("gath:1",), "h2d:3"),
        ("d2h", 2, "d2h", ("gath:2",), "d2h:2"), ("wait", 1, "host", ("d2h:1",), None), ("unpack", 1, "host", (), None),
        ("launch", 3, "ctx", ("h2d:3",), None), ("gather", 3, "ctx", ("d2h:1",), "gath:3"),
        ("d2h", 3, "ctx", ("gath:3",), "d2h:3"), ("wait", 2, "host", ("d2h:2",), None), ("unpack", 2, "host", (), None),
        ("drain", -1, "host", (), None), ("unpack", 3, "host", (), None)]
    assert [s["preset"] for s in steps if s["kind"] == "pre"] == [True, False, False]
    launch3 = next(s for s in steps if (s["kind"], s["chunk"]) == ("launch", 3))
    assert sorted(launch3["uses"]) == [["r", "bounds", 1], ["r", "theta", 1], ["w", "slots", 0]]
    # the resource table's conditions: without theta and error rows nothing names their rings; a context that
    # holds a measured hint presets nothing
    _, bare = _plans(exe, tmp_path, [(468, 64, 0, 1)], theta=0, err=0, fresh=0)[(468, 64, 0, 1)]
    assert _brief(bare) == _brief(steps) and not any(s["preset"] for s in bare)
    assert {r for s in steps for _, r, _ in s["uses"]} - {r for s in bare for _, r, _ in s["uses"]} == \
        {"theta", "thsorted", "errrows"}


def _issued_before_the_plan(chunks, sort, fail, code):
    """The steps (kind, chunk) the call issued when `fail` returned `code`, in the shape batch_run had before it
    walked a plan: set-up and chunk 0's bounds under one `rc`, then a loop over the chunks that breaks on a
    failure of its own steps and carries a failure of the next chunk's bounds (`rc_next`) to the loop's end; the
    streams are drained whatever happened, and the last chunk is unpacked only by a call that succeeded."""
    srt = [bool(sort) and m >= 64 for m in chunks]
    nc, out = len(chunks), []

    def do(kind, c):   # -> the step's code
        out.append((kind, c))
        return code if (kind, c) == fail else 0

    def bounds(c):
        rc = do("stage", c)
        if rc == 0:
            rc = do("h2d", c)
        if rc == 0 and srt[c]:
            rc = do("pre", c)
        return rc

    def loop():
        rc = do("start", -1) or do("fence", -1) or (do("zero", -1) if sort else 0) or bounds(0)
        for c in range(nc):
            if rc:
                return rc
            rc = do("launch", c) or do("gather", c)
            if rc:
                return rc
            rc_next = bounds(c + 1) if c + 1 < nc else 0
            rc = do("d2h", c)
            if rc:
                return rc
            if c > 0:
                rc = do("wait", c - 1)
                if rc:
                    return rc
                do("unpack", c - 1)
            rc = rc_next
        return rc

    rc = loop()
    do("drain", -1)
    if rc == 0:
        do("unpack", nc - 1)
    return out, rc


@pytest.mark.parametrize("san", SAN)
def test_a_failed_step_leaves_out_what_it_did_before(tmp_path, tmp_path_factory, san):
    """BatchWalk (what batch_run asks before every step) against the control flow batch_run had: every step of
    three plans failing in turn, with a bad bound's code for the staging and a device error's for the rest."""
    exe = _exe(san, tmp_path_factory)
    cases = [(468, 64, 0, 1), (200, 32, 0, 1), (3000, 1024, 20, 0), (63, 0, 0, 1)]
    plans = _plans(exe, tmp_path, cases)
    rows, want = [], []
    for case in cases:
        chunks, steps = plans[case]
        for f in range(-1, len(steps)):
            kind = steps[f]["kind"] if f >= 0 else None
            if kind in ("unpack", "drain"):   # (the host's unpacking returns nothing; a failed drain fails the call,
                continue                      # below)
            code = -1 if kind == "stage" else -2
            rows.append(("host",) + case + (f, code))
            issued, rc = _issued_before_the_plan(chunks, case[3], (kind, steps[f]["chunk"]) if f >= 0 else None, code)
            want.append(([i for i, s in enumerate(steps) if (s["kind"], s["chunk"]) in issued], rc))   # (in plan order)
    got = run_cases(exe, "walk", rows, tmp_path)
    assert len(got) == len(rows) and len(rows) > len(cases)
    for r, g, w in zip(rows, got, want):
        assert g == w, (r, g, w)
    # a failing drain fails a call that had succeeded so far, and the last chunk is then not unpacked
    chunks, steps = plans[(468, 64, 0, 1)]
    drain = next(i for i, s in enumerate(steps) if s["kind"] == "drain")
    assert _run(exe, "walk", "host", 468, 64, 0, 1, drain, -2).split() == [str(i) for i in range(drain + 1)] + ["rc", "-2"]


# every wait the schedule needs: (what is dropped, a case that shows it); chunk numbers by the step's own
MUTATIONS = [
    ("ev_zero from chunk 1's pre-pass", lambda s, e: s["kind"] == "pre" and e == "zero", (200, 32, 0, 1)),
    ("ev_pre(0) from chunk 1's pre-pass", lambda s, e: s["kind"] == "pre" and s["chunk"] == 1 and e == "pre:0", (468, 64, 0, 1)),
    ("ev_gath(c - 2) from the copies", lambda s, e: s["kind"] == "h2d" and e.startswith("gath:"), (468, 64, 0, 1)),
    ("ev_gath(c) from the copy-back", lambda s, e: s["kind"] == "d2h" and e.startswith("gath:"), (468, 64, 0, 1)),
    ("ev_pre(c) from the launches", lambda s, e: s["kind"] == "launch" and e.startswith("pre:"), (468, 64, 0, 1)),
    ("ev_h2d(c) from the launches", lambda s, e: s["kind"] == "launch" and e.startswith("h2d:"), (468, 64, 0, 1)),
    ("ev_h2d(c) from the pre-pass", lambda s, e: s["kind"] == "pre" and e.startswith("h2d:"), (468, 64, 0, 1)),
    ("the host's wait before unpacking", lambda s, e: s["kind"] == "wait", (468, 64, 0, 1)),
]


@pytest.mark.parametrize("san", SAN)
def test_every_ring_reuse_is_ordered(tmp_path, tmp_path_factory, san):
    plans = _plans(_exe(san, tmp_path_factory), tmp_path, GRID)
    for case, (_, steps) in plans.items():
        assert _hazards(steps) == [], case
    for what, drop, case in MUTATIONS:
        dropped = [(s["kind"], s["chunk"], e) for s in plans[case][1] for e in s["waits"] if drop(s, e)]
        assert dropped, what
        assert _hazards(plans[case][1], drop), what
    # the gather's wait for ev_d2h(c - 2) is implied: the host waited for that copy, one iteration earlier,
    # before it issued the gather. (Kept in the schedule as it was; this documents the redundancy.)
    redundant = lambda s, e: s["kind"] == "gather" and e.startswith("d2h:")   # noqa: E731
    assert any(redundant(s, e) for s in plans[(468, 64, 0, 1)][1] for e in s["waits"])
    for case, (_, steps) in plans.items():
        assert _hazards(steps, redundant) == [], case
