"""The device-resident batch's pipeline plan (`device_batch_plan` of `ppls_amd/csrc/aq_batch_plan.h`, what
`aq_integrate_batch_device` walks) built alone with g++, plain and under AddressSanitizer + UBSan: (a) the chunking
and the plan against a restatement of the schedule; (b) a happens-before check over the plan and its resource
table (batch_plan_util.hazards) -- every two steps that touch the same buffer, one of them writing, are ordered by
streams and event waits -- which must report a hazard when any needed wait is dropped; (c) no step is the host's,
launches and gathers run on the context's stream, and a chunk of fewer than PCU_MAXK rows is launched into slots
from NPARTS; (d) a failed step ends the call there."""
import itertools
import json

import pytest

import batch_plan_util
from batch_plan_util import MAXK, SAN, hazards as _hazards, run_cases

CHUNKS = [[5], [100], [100, 100, 5], [64] * 5]
FLAGS = list(itertools.product([1, 0], [0, 1], [0, 1], [1, 0]))   # sort, theta, err, caller


@pytest.fixture
def exe(tmp_path_factory):
    return batch_plan_util.exe(None, tmp_path_factory)   # (test_under_the_sanitizers: the same tests, that build)


def _json(exe, *args):
    return json.loads(batch_plan_util.run(exe, *args))


def _plan(exe, chunks, sort, theta, err, caller, fresh=1):
    return _json(exe, "plan", "dev", sort, theta, err, fresh, caller, *chunks)


def _schedule(chunks, sort, caller):
    """The schedule restated: the joins with the caller's stream, chunk 0's check (and size order) on the context's
    stream, then per chunk its launch and gather there and the next chunk's check (and size order) on the side
    stream; a check waits for the gather two chunks back, whose ring parity it overwrites."""
    nc, steps = len(chunks), []
    srt = [bool(sort) and m >= 64 for m in chunks]

    def feed(c):
        s = "ctx" if c == 0 else "pre"
        steps.append(("check", c, s, [f"gath:{c - 2}"] if c >= 2 else [], f"check:{c}"))
        if srt[c]:
            # (behind its check on the same stream; chunk 1's also behind the zeroing of its counts)
            steps.append(("pre", c, s, ["pre:0" if srt[0] else "zero"] if c == 1 else [], f"pre:{c}"))

    if caller:
        steps.append(("join_in", -1, "caller", [], "in"))
    steps.append(("start", -1, "ctx", ["in"] if caller else [], "start"))
    steps.append(("fence", -1, "pre", ["start"], None))
    if sort:
        steps.append(("zero", -1, "ctx", [], None if srt[0] else "zero"))
    feed(0)
    for c in range(nc):
        steps.append(("launch", c, "ctx", [f"pre:{c}" if srt[c] else f"check:{c}"], None))
        steps.append(("gather_soa", c, "ctx", [], f"gath:{c}" if c + 1 < nc else ("out" if caller else None)))
        if c + 1 < nc:
            feed(c + 1)
    if caller:
        steps.append(("join_out", -1, "caller", ["out"], None))
    return srt, steps


def test_chunks_are_full_launches_and_a_remainder(exe):
    assert _json(exe, "--constants") == {"MAXK": MAXK, "PCU_MAXK": 12, "NPARTS": 16384, "BATCH_SORT_MIN": 64}
    for n, env, want in [(1, MAXK, [1]), (MAXK, MAXK, [MAXK]), (MAXK + 1, MAXK, [MAXK, 1]),
                         (2 * MAXK + 1000, MAXK, [MAXK, MAXK, 1000]), (350, 100, [100, 100, 100, 50]),
                         (305, 100, [100, 100, 100, 5]), (3, 0, [1, 1, 1]), (3, -7, [1, 1, 1]),
                         (MAXK + 5, 10 * MAXK, [MAXK, 5])]:
        assert _json(exe, "chunks", n, env)["chunks"] == want, (n, env)


def test_plan_is_the_stated_schedule(exe):
    for chunks in CHUNKS + [[32, 64, 104], [MAXK, MAXK, 7]]:
        for sort, theta, err, caller in FLAGS:
            p = _plan(exe, chunks, sort, theta, err, caller)
            srt, want = _schedule(chunks, sort, caller)
            got = [(s["kind"], s["chunk"], s["stream"], s["waits"], s["record"]) for s in p["steps"]]
            assert got == want, (chunks, sort, caller)
            assert p["chunks"] == chunks and p["sorted"] == [int(x) for x in srt]
            # a chunk below the per-CU threshold has no bounds on the host to pass as kernel arguments: high slots
            assert p["first_slot"] == [16384 if m < 12 else 0 for m in chunks]
            # the host batch's preset rule: sorted chunks, until a launch of >= PCU_MAXK rows has measured a hint
            fresh, preset = True, []
            for m, s in zip(chunks, srt):
                preset.append(int(fresh and s))
                fresh = fresh and m < 12
            assert p["preset"] == preset
            assert _plan(exe, chunks, sort, theta, err, caller, fresh=0)["preset"] == [0] * len(chunks)
            events = {e for s in p["steps"] for e in s["waits"] + [s["record"]] if e}
            assert len(events) <= p["n_events"]


def test_no_host_step_and_launches_on_the_context_stream(exe):
    for chunks in CHUNKS:
        for sort, theta, err, caller in FLAGS:
            steps = _plan(exe, chunks, sort, theta, err, caller)["steps"]
            assert {s["stream"] for s in steps} <= {"ctx", "pre", "caller"}   # (no host stream exists in the plan)
            assert {s["kind"] for s in steps} <= {"join_in", "start", "fence", "zero", "check", "pre", "launch",
                                                  "gather_soa", "join_out"}
            for s in steps:
                if s["kind"] in ("launch", "gather_soa"):
                    assert s["stream"] == "ctx"
                if s["kind"] in ("join_in", "join_out"):
                    assert s["stream"] == "caller" and caller
            assert [s["chunk"] for s in steps if s["kind"] == "launch"] == list(range(len(chunks)))
            assert [s["chunk"] for s in steps if s["kind"] == "gather_soa"] == list(range(len(chunks)))
            # chunk c + 1's check is enqueued on the side stream, with no wait for chunk c's launch or gather
            for s in steps:
                if s["kind"] in ("check", "pre") and s["chunk"] > 0:
                    assert s["stream"] == "pre"
                    assert not any(e in (f"gath:{s['chunk'] - 1}", "out") for e in s["waits"])


def test_resource_table_conditions(exe):
    full = _plan(exe, [100, 100, 5], 1, 1, 1, 1)["steps"]
    bare = _plan(exe, [100, 100, 5], 1, 0, 0, 1)["steps"]
    names = lambda steps: {r for s in steps for _, r, _ in s["uses"]}   # noqa: E731
    assert names(full) - names(bare) == {"theta", "thsorted"}
    launch2 = next(s for s in full if (s["kind"], s["chunk"]) == ("launch", 2))   # the unsorted tail
    assert sorted(launch2["uses"]) == [["r", "bounds", 0], ["r", "theta", 0], ["w", "slots", 0]]
    launch1 = next(s for s in full if (s["kind"], s["chunk"]) == ("launch", 1))
    assert sorted(launch1["uses"]) == [["r", "sorted", 1], ["r", "thsorted", 1], ["w", "slots", 0]]
    gather1 = next(s for s in full if (s["kind"], s["chunk"]) == ("gather_soa", 1))
    assert sorted(gather1["uses"]) == [["add", "errbits", 0], ["r", "flag", 1], ["r", "perm", 1], ["w", "out", 1],
                                       ["w", "slots", 0]]
    join_out = full[-1]
    assert join_out["kind"] == "join_out" and sorted(join_out["uses"]) == \
        [["r", "out", c] for c in range(3)] + [["w", "in", c] for c in range(3)]


# every wait the schedule needs: (what is dropped, chunks, sort)
MUTATIONS = [
    ("ev_in from the start", lambda s, e: s["kind"] == "start" and e == "in", [100, 100, 5], 1),
    ("ev_start from the side stream's fence", lambda s, e: s["kind"] == "fence", [100, 100, 5], 1),
    ("ev_gath(c - 2) from the checks", lambda s, e: s["kind"] == "check" and e.startswith("gath:"), [64] * 5, 1),
    ("ev_gath(c - 2) from the checks, unsorted", lambda s, e: s["kind"] == "check" and e.startswith("gath:"), [64] * 5, 0),
    ("ev_pre(c) from the launches", lambda s, e: s["kind"] == "launch" and e.startswith("pre:"), [100, 100, 5], 1),
    ("ev_check(c) from the launches", lambda s, e: s["kind"] == "launch" and e.startswith("check:"), [100, 100, 5], 0),
    ("ev_pre(0) from chunk 1's pre-pass", lambda s, e: s["kind"] == "pre" and s["chunk"] == 1 and e == "pre:0",
     [100, 100, 5], 1),
    ("ev_zero from chunk 1's pre-pass", lambda s, e: s["kind"] == "pre" and e == "zero", [32, 64, 104], 1),
    ("ev_out from the caller's stream", lambda s, e: s["kind"] == "join_out", [100, 100, 5], 1),
]


def test_every_ring_reuse_is_ordered(exe):
    for chunks in CHUNKS + [[32, 64, 104], [MAXK, MAXK, 7]]:
        for sort, theta, err, caller in FLAGS:
            steps = _plan(exe, chunks, sort, theta, err, caller)["steps"]
            assert _hazards(steps) == [], (chunks, sort, theta, err, caller)
    for what, drop, chunks, sort in MUTATIONS:
        steps = _plan(exe, chunks, sort, 1, 1, 1)["steps"]
        assert [(s["kind"], s["chunk"], e) for s in steps for e in s["waits"] if drop(s, e)], what
        assert _hazards(steps, drop), what
    # a ring parity is reused: chunk 2's check writes what chunk 0's launch and gather read
    steps = _plan(exe, [64] * 5, 1, 1, 1, 1)["steps"]
    haz = _hazards(steps, lambda s, e: s["kind"] == "check" and e.startswith("gath:"))
    assert ("gather_soa", 0, "check", 2, "flag", 0) in haz and ("launch", 1, "pre", 3, "sorted", 1) in haz


@pytest.mark.parametrize("san", SAN)
def test_a_failed_step_ends_the_call_there(san, tmp_path_factory, tmp_path):
    """BatchWalk over the device plans: with each step failing in turn the steps issued are exactly those up to
    and including it -- nothing enqueued waits for an event that is never recorded, and the caller's stream is not
    joined behind a failed call -- and the call returns that step's code; with no failure every step is issued."""
    exe = batch_plan_util.exe(san, tmp_path_factory)
    rows, want = [], []
    for chunks, caller, sort in itertools.product(CHUNKS, [0, 1], [0, 1]):
        steps = _plan(exe, chunks, sort, 1, 1, caller)["steps"]
        assert steps[-1]["kind"] == ("join_out" if caller else "gather_soa")
        for f in range(-1, len(steps)):
            code = -3 - f % 5
            rows.append(("dev", sort, caller, f, code, *chunks))
            want.append((list(range(f + 1)), code) if f >= 0 else (list(range(len(steps))), 0))
    got = run_cases(exe, "walk", rows, tmp_path)
    assert len(got) == len(rows) and len(rows) > 16 * 4
    for r, g, w in zip(rows, got, want):
        assert g == w, (r, g, w)


@pytest.mark.parametrize("san", SAN[1:])
@pytest.mark.parametrize("test", [test_chunks_are_full_launches_and_a_remainder, test_plan_is_the_stated_schedule,
                                  test_no_host_step_and_launches_on_the_context_stream, test_resource_table_conditions,
                                  test_every_ring_reuse_is_ordered], ids=lambda t: t.__name__)
def test_under_the_sanitizers(test, san, tmp_path_factory):
    """Every test above once more, on the check program built with -fsanitize (as the host plans' tests are)."""
    test(batch_plan_util.exe(san, tmp_path_factory))
