"""The ring's lines (ppls_amd/csrc/aq_ring_window.h) without a GPU.

tests/ring_window_walk.cpp, a stand-alone program built against the header, walks every reachable
(ring, held, prefetch, cellar) state under the rules k_stream applies -- every number of pushes and of held
pairs a round can end with, a burst ending after any round, a cellar that fills up -- and stops at the first
step where the ring would hold more than WCAP pairs, a spill finds no whole chunk, a landing crosses the
line, or a burst's end moves out other than exactly the chunks it needs. It runs for WCAP = 256 with the
kernel's lines and for a small ring, plain and once built with -fsanitize=address,undefined.

tools/ring_sim.py --mode carried runs the same rules over a real (tiny) tree.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppls_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "ring_window_walk.cpp")
sys.path.insert(0, ROOT)

CXX = shutil.which("g++") or "g++"   # the host compiler the build needs anyway


def _macro(name, text):
    m = re.search(r"#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, text, re.M)
    assert m, name
    return m.group(1)


def kernel_lines():
    """(WCAP, line, PF_ISSUE, PF_BELOW, REFILL) as aq_stream.h / aq_shape.h define them by default."""
    with open(os.path.join(CSRC, "aq_stream.h")) as f:
        st = f.read()
    with open(os.path.join(CSRC, "aq_shape.h")) as f:
        sh = f.read()
    env = {"WCAP": int(_macro("AQ_WCAP", sh))}
    ev = lambda s: int(eval(s.replace("/", "//"), {}, env))   # noqa: E731  (integer macros: WCAP, + - / and parentheses)
    return (env["WCAP"], ev(_macro("AQ_SPILL_LINE", st)), ev(_macro("AQ_PF_ISSUE", st)), ev(_macro("AQ_PF_BELOW", st)),
            ev(_macro("AQ_REFILL", st)))


@pytest.fixture(scope="module")
def walkers(tmp_path_factory):
    d = tmp_path_factory.mktemp("ring_walk")
    plain, san = str(d / "walk"), str(d / "walk_san")
    base = [CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC]
    subprocess.check_call(base + ["-O2", "-o", plain])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san])
    return plain, san


def _walk(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    fig = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout))
    return p.returncode, p.stdout.strip() + p.stderr.strip(), fig


def test_kernel_lines_are_walked_clean(walkers):
    wcap, line, issue, below, refill = kernel_lines()
    assert wcap == 256 and line <= wcap
    rc, out, fig = _walk(walkers[0], wcap, line, issue, below, refill)
    print(out)
    assert rc == 0, out
    assert fig["max_ring"] <= wcap and fig["max_S"] <= line
    assert fig["spills"] > 0 and fig["landings"] > 0 and fig["exits"] > 0
    # a line at the capacity makes the burst's end move chunks out; a line 64 below never needs to
    assert (fig["exit_moves"] > 0) == (line > wcap - 64)


@pytest.mark.parametrize("lines", [(256, 256, 160, 64, 192), (256, 224, 160, 64, 192), (256, 192, 160, 64, 192),
                                   (256, 256, 191, 191, 256), (128, 128, 48, 32, 64), (128, 127, 63, 63, 64)])
def test_lines_are_walked_clean(walkers, lines):
    """The capacity line, an intermediate one, the old one, the extreme valid lines, and a small ring."""
    rc, out, fig = _walk(walkers[0], *lines)
    print(out)
    assert rc == 0, out
    assert fig["max_ring"] <= lines[0] and fig["max_S"] <= lines[1]
    assert (fig["exit_moves"] > 0) == (lines[1] > lines[0] - 64)


def test_sanitized_walk(walkers):
    """The same walks in the address / undefined-behaviour sanitized build, run directly."""
    for lines in ((256,) + kernel_lines()[1:], (128, 128, 48, 32, 64)):
        rc, out, _ = _walk(walkers[1], *lines)
        print(out)
        assert rc == 0, out


def test_walk_finds_what_it_looks_for(walkers):
    """Without the burst end's chunk move a line at the capacity overflows at the push-back, and the walk
    says so; lines the header calls invalid are refused."""
    rc, out, _ = _walk(walkers[0], 256, 256, 160, 64, 192, "--no-exit-drain")
    assert rc == 1 and "push-back overflows" in out, out
    rc, out, _ = _walk(walkers[0], 256, 192, 160, 64, 192, "--no-exit-drain")
    assert rc == 0, out   # the old line never needed it
    for bad in ((256, 320, 160, 64, 192), (256, 256, 160, 224, 192), (256, 120, 40, 32, 64), (256, 256, 160, 64, 320)):
        rc, out, _ = _walk(walkers[0], *bad)
        assert rc == 2, (bad, out)


@pytest.mark.parametrize("hi", [192, 224, 256])
def test_ring_sim_carried_tiny_tree(hi):
    """The carried-pair model on the eps = 1e-3 tree: every pair below the seed depth is evaluated once, and the
    ring stays within the line inside bursts (max_S) and within WCAP after every push-back (max_ring). A second,
    larger tree (1e-6) from deep seeds so that spills, landings and burst ends all happen."""
    from tools import ring_sim
    pairs = ring_sim.build_tree(1e-3)
    out = ring_sim.run_carried(pairs, D=3, shares=2, HI=hi, GIVE=4)
    assert out["pairs_done"] == out["pairs_total"] and out["tasks"] == 2 * out["pairs_done"]
    assert out["max_S"] <= hi and out["max_ring"] <= 256
    pairs = ring_sim.build_tree(1e-6)
    out = ring_sim.run_carried(pairs, D=4, shares=1, HI=hi, GIVE=16)
    print(out)
    assert out["pairs_done"] == out["pairs_total"]
    assert out["max_S"] <= hi and out["max_ring"] <= 256
    assert out["spill_per_round"] > 0 and out["land_per_round"] > 0
