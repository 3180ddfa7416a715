"""What tests/test_batch_plan.py and tests/test_device_batch_plan.py share: the check program
(`tests/native/batch_plan_check.cpp` over `ppls_amd/csrc/aq_batch_plan.h`) built alone with g++, plain or under
AddressSanitizer + UBSan, and the happens-before check over a printed plan and its resource table."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batch_plan_check.cpp")
INC = [os.path.join(ROOT, "ppls_amd", "csrc"), os.path.join(ROOT, "include")]
SAN = [None, "address,undefined"]
MAXK = 262144
_built = {}


def exe(san, tmp_path_factory):
    """The check program, built once per session and sanitizer setting."""
    if san not in _built:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        out = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_check")
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", INC[0], "-I", INC[1], SRC, "-o", out]
        if san:
            cmd.insert(1, "-fsanitize=" + san)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode and san:
            pytest.skip("sanitizer runtime unavailable: " + r.stderr[-400:])
        assert r.returncode == 0, r.stderr[-2000:]
        _built[san] = out
    return _built[san]


def run(exe_path, *args):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe_path, *[str(a) for a in args]], capture_output=True, text=True, timeout=120, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def run_cases(exe_path, what, cases, tmp_path):
    """`what` ("plan" or "walk") for every case (a tuple of words) through one file: the output's lines."""
    path = tmp_path / (what + ".txt")
    path.write_text("".join(" ".join(str(x) for x in case) + "\n" for case in cases))
    lines = run(exe_path, what, "@" + str(path)).splitlines()
    assert len(lines) == len(cases)
    return [json.loads(ln) for ln in lines] if what == "plan" else \
        [([int(x) for x in ln.split("rc")[0].split()], int(ln.split("rc")[1])) for ln in lines]


def brief(steps):
    return [(s["kind"], s["chunk"], s["stream"], tuple(s["waits"]), s["record"]) for s in steps]


def hazards(steps, drop=lambda step, event: False):
    """Pairs of steps that conflict on a buffer -- the same instance of a resource, not both reading, not both
    atomic adds (two adds commute) -- and are not ordered. Order: steps of one stream (the host is one) follow
    each other; a wait puts the step behind the one that recorded the event (and all before that); where the plan
    has host steps, a device step follows the last host step issued before it and the drain follows everything.
    `drop(step, event)`: leave that wait out."""
    before, last_on, recorded, last_host = [], {}, {}, None
    for i, s in enumerate(steps):
        preds = [last_on.get(s["stream"])]
        preds += [recorded[e] for e in s["waits"] if not drop(s, e)]   # (KeyError: a wait for an event never recorded)
        if s["stream"] != "host":
            preds.append(last_host)
        if s["kind"] == "drain":
            preds += range(i)
        m = 0
        for p in preds:
            if p is not None:
                m |= before[p] | (1 << p)
        before.append(m)
        last_on[s["stream"]] = i
        if s["stream"] == "host":
            last_host = i
        if s["record"]:
            assert s["record"] not in recorded, s
            recorded[s["record"]] = i
    out = []
    for j, t in enumerate(steps):
        for i in range(j):
            if before[j] >> i & 1:
                continue
            for mi, ri, ii in steps[i]["uses"]:
                for mj, rj, ij in t["uses"]:
                    if (ri, ii) == (rj, ij) and not (mi == "r" and mj == "r") and not (mi == "add" and mj == "add"):
                        out.append((steps[i]["kind"], steps[i]["chunk"], t["kind"], t["chunk"], ri, ii))
    return out
