"""Mesh moments on the GPU: the cases of tests/mesh_moments_cases.py, run in ONE child process that imports torch
before libaquad.so is loaded (the arrangement of tests/test_gpu_mesh_coarsen.py, and for its reason: the meshes, the
per-row centres and ranges and the outputs are torch CUDA tensors handed to the library as device pointers, so both
must sit on one HIP runtime). The child is a pytest run of the cases file with a JUnit report; every case below passes
when its cases in the child passed, and shows the child's failure text otherwise."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "mesh_moments_cases.py")
# (name, the fewest parametrised cases of it the child must have run)
TESTS = [("test_parity", 5), ("test_ranges", 2), ("test_arguments_and_memory", 1), ("test_interleaved_on_one_context", 1),
         ("test_python_surface", 1)]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    report = str(tmp_path_factory.mktemp("mesh_moments") / "report.xml")
    code = ("import torch, sys, pytest; "
            "sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-s', '-p', 'no:cacheprovider', '--junitxml', %r]))" % (CASES, report))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(HERE), timeout=600)
    print(r.stdout[-6000:])
    assert os.path.exists(report), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    out = {}
    for case in ET.parse(report).getroot().iter("testcase"):
        bad = [e for e in case if e.tag in ("failure", "error", "skipped")]
        out.setdefault(case.get("name").split("[")[0], []).append(
            (case.get("name"), "\n".join((e.get("message") or "") + "\n" + (e.text or "") for e in bad) if bad else None))
    return out


@pytest.mark.parametrize("name,at_least", TESTS)
def test_mesh_moments(child, name, at_least):
    ran = child.get(name, [])
    assert len(ran) >= at_least, (name, [c for c, _ in ran])
    failed = [(c, why) for c, why in ran if why is not None]
    assert not failed, "\n\n".join("%s:\n%s" % f for f in failed)
