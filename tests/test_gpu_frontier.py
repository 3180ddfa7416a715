"""The frontier engine's level kernels on the GPU: the cases of tests/frontier_cases.py, run in ONE child process
that imports torch before libaquad.so is loaded.

Why a child: the frontiers are torch CUDA tensors handed to the library as device pointers, so both must sit on one
HIP runtime, and the cases that cap the level step's grid (AQ_LEVEL_GRID) set the environment of contexts of their
own (the arrangement of tests/test_gpu_mesh.py). The child is a pytest run of the cases file with a JUnit report;
every case below passes when its cases in the child passed, and shows the child's failure text otherwise."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "frontier_cases.py")
# (name, the fewest parametrised cases of it the child must have run)
TESTS = [("test_level_f_bits", 8), ("test_step_chunk_edges", 19), ("test_step_overflow_two_short", 1),
         ("test_step_depth_cap", 1), ("test_chained_counts", 5), ("test_narrow_in_order", 72),
         ("test_narrow_zero_levels", 1), ("test_narrow_capacity", 1), ("test_narrow_depth_cap", 1),
         ("test_fold_past_lp_cap", 1), ("test_fold_on_accumulator_change", 1),
         ("test_defer_off_with_nothing_pending", 1), ("test_edge_tree_frontier", 26), ("test_mesh_case_frontier", 10),
         ("test_tree_capped_grid", 2)]


def test_at_least_is_the_parametrisation():
    """Every test of the cases file is listed above with exactly the number of cases its parametrisation makes."""
    import frontier_cases as fc
    listed = dict(TESTS)
    assert len(listed) == len(TESTS)
    assert sorted(listed) == sorted(n for n in dir(fc) if n.startswith("test_"))
    for name, at_least in TESTS:
        n = 1
        for m in getattr(getattr(fc, name), "pytestmark", []):
            if m.name == "parametrize":
                n *= len(m.args[1])
        assert n == at_least, (name, n)


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    report = str(tmp_path_factory.mktemp("frontier") / "report.xml")
    code = ("import torch, sys, pytest; "
            "sys.exit(pytest.main([%r, '-m', 'gpu', '-q', '-s', '-p', 'no:cacheprovider', '--durations=8', "
            "'--junitxml', %r]))" % (CASES, report))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    env = {k: v for k, v in os.environ.items() if k != "AQ_LEVEL_GRID"}   # the cases set their own
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(HERE), timeout=600, env=env)
    print(r.stdout[-6000:])
    assert os.path.exists(report), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    out = {}
    for case in ET.parse(report).getroot().iter("testcase"):
        bad = [e for e in case if e.tag in ("failure", "error", "skipped")]
        out.setdefault(case.get("name").split("[")[0], []).append(
            (case.get("name"), "\n".join((e.get("message") or "") + "\n" + (e.text or "") for e in bad) if bad else None))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,at_least", TESTS)
def test_frontier(child, name, at_least):
    ran = child.get(name, [])
    assert len(ran) >= at_least, (name, [c for c, _ in ran])
    failed = [(c, why) for c, why in ran if why is not None]
    assert not failed, "\n\n".join("%s:\n%s" % f for f in failed)
