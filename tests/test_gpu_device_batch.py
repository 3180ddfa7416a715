"""The device-resident batch on the GPU: the cases of tests/device_batch_cases.py, run in ONE child process that
imports torch before libaquad.so is loaded.

Why a child: the call shares a HIP stream and device pointers with torch, so both must sit on one HIP runtime. A
torch wheel that bundles its own ROCm runtime gives that only when torch is imported first (the library then binds
to the runtime torch loaded, as in bench.py and smoke()); this process has long loaded the library -- the other test
files do -- when these tests start. The child is a pytest run of the cases file with a JUnit report; every case
below passes when its cases in the child passed, and shows the child's failure text otherwise."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "device_batch_cases.py")
# (name, the fewest parametrised cases of it the child must have run)
TESTS = [("test_parity_one_chunk", 8), ("test_parity_chunks", 3), ("test_fixed_families_err", 2),
         ("test_param_family_err", 3), ("test_invalid_rows_are_contained", 1), ("test_error_bits_reach_the_row", 1),
         ("test_stream_order", 1), ("test_call_only_enqueues", 1), ("test_coexistence", 1),
         ("test_host_checked_arguments", 1)]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    report = str(tmp_path_factory.mktemp("devbatch") / "report.xml")
    code = ("import torch, sys, pytest; "
            "sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-s', '-p', 'no:cacheprovider', '--junitxml', %r]))" % (CASES, report))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(HERE), timeout=900)
    print(r.stdout[-6000:])
    assert os.path.exists(report), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    out = {}
    for case in ET.parse(report).getroot().iter("testcase"):
        bad = [e for e in case if e.tag in ("failure", "error", "skipped")]
        out.setdefault(case.get("name").split("[")[0], []).append(
            (case.get("name"), "\n".join((e.get("message") or "") + "\n" + (e.text or "") for e in bad) if bad else None))
    return out


@pytest.mark.parametrize("name,at_least", TESTS)
def test_device_batch(child, name, at_least):
    ran = child.get(name, [])
    assert len(ran) >= at_least, (name, [c for c, _ in ran])
    failed = [(c, why) for c, why in ran if why is not None]
    assert not failed, "\n\n".join("%s:\n%s" % f for f in failed)
