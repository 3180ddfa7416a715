"""The launch plan of the persistent kernel (`ppls_amd/csrc/aq_launch_plan.h` plan_launch: instance, waves,
shares, seed depth, tail, job mode, hint state) built alone with g++ and replayed against the plans recorded
from launch_stream at the commit named in `tests/golden/launch_plans.json`: every field of every row is equal.
Table 0 was made with the default constants, table 1 with -DAQ_S_W=4, which reaches the seed-fit refusal."""
import functools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "launch_plan_check.cpp")
INC = [os.path.join(ROOT, "ppls_amd", "csrc"), os.path.join(ROOT, "include")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _plans(table):
    """The table's accepted rows as dicts of request, plan and hint-after columns."""
    cols = _golden()["columns"]
    out = []
    for req, hint, plan, after in table["rows"]:
        d = dict(zip(cols["req"], req))
        d.update(zip(cols["plan"], plan))
        d["hint_in"] = dict(zip(cols["hint"], hint))
        d["hint_after"] = dict(zip(cols["hint_after"], after))
        out.append(d)
    return out


def _num(x):
    return float(x).hex() if isinstance(x, float) else str(x)


def _replay(tmp_path, table, san=None):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "launch_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", INC[0], "-I", INC[1]] + table["defines"] + [SRC, "-o", exe]
    if san:
        cmd.insert(1, "-fsanitize=" + san)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and san:
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-400:])
    assert r.returncode == 0, r.stderr[-2000:]
    # the recorded plans hold for the constants they were made with
    consts = json.loads(subprocess.run([exe, "--constants"], capture_output=True, text=True, check=True).stdout)
    assert consts == table["constants"], "launch-shape constants changed: regenerate tests/golden/launch_plans.json"
    rows = tmp_path / "rows.txt"
    with open(rows, "w") as f:
        for req, hint, plan, after in table["rows"]:
            f.write(" ".join(_num(x) for x in req + hint + plan[:10] + after) + "\n")   # (plan[10]: sin_deeper)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(rows)], capture_output=True, text=True, timeout=120, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip() == "ok %d" % len(table["rows"])


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_plans_equal_recorded(tmp_path, san):
    _replay(tmp_path, _golden()["tables"][0], san)


def test_refusal_with_s_w_4(tmp_path):
    table = _golden()["tables"][1]
    assert table["defines"] == ["-DAQ_S_W=4"] and len(table["rows"]) <= 500
    assert any(plan[0] != 0 for _, _, plan, _ in table["rows"]), "no refused row"
    _replay(tmp_path, table)


def test_named_cosh4_rows():
    """The hand-derived cosh^4 plans at grid 256, unsharded, fresh hint: the first rows of table 0."""
    V = {v: i for i, v in enumerate(_golden()["variants"])}
    want = [  # k, variant, nwt, shares, D, tail_from, tail_mult, static_jobs
        (1, "LONE", 8, 2048, 13, 1, 1, 1),
        (11, "PCU", 12, 1536, 12, 11, 1, 1),
        (12, "HEAP", 12, 256, 10, 12, 1, 0),
        (3072, "PLAIN", 12, 16, 7, 2976, 4, 0),
    ]
    rows = _plans(_golden()["tables"][0])
    for (k, variant, nwt, shares, D, tail_from, tail_mult, static), p in zip(want, rows):
        assert (p["fid"], p["grid"], p["k"], p["shard_array"], p["nshards"], p["hint_in"]["valid"]) == (0, 256, k, 0, 1, 0)
        assert p["rc"] == 0
        assert (p["variant"], p["nwt"], p["shares"], p["D"], p["tail_from"], p["tail_mult"], p["static_jobs"]) == \
            (V[variant], nwt, shares, D, tail_from, tail_mult, static), p
    assert [p["adaptive"] for p in rows[:3]] == [0, 0, 2]


def test_table_covers_every_branch():
    doc = _golden()
    table = doc["tables"][0]
    assert len(table["rows"]) <= 4000 and len(doc["parent_commit"]) == 40
    rows = _plans(table)
    assert all(p["rc"] == 0 for p in rows)   # the default constants reach no refusal (table 1 does)
    assert {p["variant"] for p in rows} == set(range(len(doc["variants"])))
    assert {p["adaptive"] for p in rows} == {0, 2, 3, 7}
    assert {p["tail_mult"] > 1 for p in rows} == {False, True}
    assert {p["static_jobs"] for p in rows} == {0, 1}
    assert {p["sin_deeper"] for p in rows} == {-1, 0, 1}   # sin(1/x) deeper seeding: not eligible, not taken, taken
    # the deal of few whole integrals (static per-CU launches, default gsplit): k waves per share, halved until
    # it divides W; sin(1/x) keeps one wave per share up to 4 integrals; the lone instance is k == 1 only
    few = [p for p in rows if 2 <= p["k"] <= 11 and p["per_cu"] and p["nshards"] == 1 and not p["shard_array"] and
           p["gsplit_env"] == 0]
    for fid in (0, 1, 2):
        for diag in (0, 1):
            assert {2, 4, 5, 11} <= {p["k"] for p in few if p["fid"] == fid and p["diag"] == diag}, (fid, diag)
    for p in few:
        W, gs = p["grid"] * p["nwt"], p["k"]
        while gs > 1 and W % gs:
            gs >>= 1
        assert p["shares"] == (W if p["fid"] == 1 and p["k"] <= 4 else W // gs), p
        assert p["nwt"] == table["constants"]["NW"] and doc["variants"][p["variant"]] in ("PCU", "DIAG_PCU"), p
    # a hint left by a launch of another nshards is not the same workload
    assert any(p["adaptive"] == 2 and p["hint_in"]["valid"] and p["hint_in"]["eps"] == p["eps"] and
               p["hint_in"]["fid"] == p["fid"] and p["hint_in"]["nshards"] != p["nshards"] for p in rows)
