"""The C ABI's HIP-free argument rules (`ppls_amd/csrc/aq_host_args.h`) built alone with g++, plain and under
AddressSanitizer + UBSan: the batch front end's chunk schedule against a restatement of its rule, and the
range rules every launch entry point shares (k, eps, depth, shards, slots) at their edges."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "host_args_check.cpp")
INC = [os.path.join(ROOT, "ppls_amd", "csrc"), os.path.join(ROOT, "include")]
SAN = [None, "address,undefined"]


def _exe(san, tmp_path):
    """The check program, built once per test."""
    exe = str(tmp_path / "host_args_check")
    if os.path.exists(exe):
        return exe
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", INC[0], "-I", INC[1], SRC, "-o", exe]
    if san:
        cmd.insert(1, "-fsanitize=" + san)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and san:
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-400:])
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(san, tmp_path, mode, rows=None):
    args = [_exe(san, tmp_path), mode]
    if rows is not None:
        path = tmp_path / (mode + ".txt")
        path.write_text("".join(" ".join(str(x) for x in row) + "\n" for row in rows))
        args.append(str(path))
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _constants(san, tmp_path):
    return json.loads(_run(san, tmp_path, "--constants"))


def _chunks_rule(n, first, last, maxk):
    """A first chunk of `first` (0: a whole launch), each next one twice the last up to a whole launch, the
    remainder last -- split so that the last chunk is `last` when the remainder is more than twice that."""
    out, size = [], min(first, maxk) if first else maxk
    while n - sum(out) > size:
        out.append(size)
        size = min(2 * size, maxk)
    rem = n - sum(out)
    if last and rem > 2 * last:
        return out + [rem - last, last]
    return out + [rem] if rem else out


@pytest.mark.parametrize("san", SAN)
def test_chunk_schedule(tmp_path, san):
    K = _constants(san, tmp_path)["MAXK"]
    assert K == 262144
    cases = list(itertools.product([0, 1, 63, 64, 200, K - 1, K, K + 1, 2 * K + 1000, 1000003],
                                   [0, 16, 32, 131072, K, 2 * K], [0, 4096]))
    lines = _run(san, tmp_path, "chunks", cases).splitlines()
    assert len(lines) == len(cases)
    got = {case: [] if ln == "-" else [int(x) for x in ln.split()] for case, ln in zip(cases, lines)}
    for (n, first, last), c in got.items():
        assert c == _chunks_rule(n, first, last, K), (n, first, last, c)
        assert sum(c) == n and all(1 <= x <= K for x in c), (n, first, last, c)
        assert n or c == []
    # by hand: the defaults over three launches' worth, and the unsorted-then-sorted schedule of
    # test_gpu.py::test_batch_small_first_chunk_twice
    assert got[(2 * K + 1000, 131072, 0)] == [131072, 262144, 132072]
    assert got[(200, 32, 0)] == [32, 64, 104] and got[(200, 16, 0)] == [16, 32, 64, 88]
    assert got[(1000003, 0, 4096)] == [K, K, K, 1000003 - 3 * K - 4096, 4096]


@pytest.mark.parametrize("san", SAN)
def test_launch_range_rules(tmp_path, san):
    k = _constants(san, tmp_path)
    K, S, L = k["MAXK"], k["NSLOTS"], k["AQ_MAX_LEVELS"]
    ok = dict(k=1, eps=1e-3, max_depth=0, shard=0, nshards=1, shard_array=0, first_slot=0, slot_limit=S)
    table = [  # (what differs from `ok`, accepted)
        ({}, 1),
        (dict(k=0), 0), (dict(k=K), 1), (dict(k=K + 1), 0), (dict(k=K + 1, slot_limit=S + 1), 0), (dict(k=-1), 0),
        (dict(nshards=0), 0), (dict(nshards=64, shard=63), 1), (dict(nshards=65, shard=0), 0),
        (dict(nshards=65, shard_array=1), 0), (dict(nshards=0, shard_array=1), 0),
        (dict(shard=-1), 0), (dict(shard=1), 0), (dict(nshards=8, shard=8), 0), (dict(nshards=8, shard=7), 1),
        (dict(shard=-1, shard_array=1), 1), (dict(nshards=8, shard=8, shard_array=1), 1),   # the array names the shards
        (dict(k=100, first_slot=S - 100), 1), (dict(k=100, first_slot=S - 99), 0), (dict(first_slot=-1), 0),
        (dict(first_slot=S), 0), (dict(first_slot=S, slot_limit=S + 1), 1), (dict(k=2, first_slot=S, slot_limit=S + 1), 0),
        (dict(k=2, first_slot=2 ** 31 - 1), 0),
        (dict(eps=0.0), 1), (dict(eps=-0.0), 1), (dict(eps=float("nan")), 0), (dict(eps=-1.0), 0),
        (dict(eps=float("inf")), 1), (dict(eps=-5e-324), 0),
        (dict(max_depth=-1), 0), (dict(max_depth=L - 1), 1), (dict(max_depth=L), 0),
    ]
    cols = ["k", "eps", "max_depth", "shard", "nshards", "shard_array", "first_slot", "slot_limit"]
    rows = []
    for diff, _ in table:
        row = dict(ok, **diff)
        row["eps"] = float(row["eps"]).hex()
        rows.append([row[c] for c in cols])
    got = [int(x) for x in _run(san, tmp_path, "ranges", rows).split()]
    assert got == [want for _, want in table], [(d, g) for (d, w), g in zip(table, got) if g != w]


@pytest.mark.parametrize("san", SAN)
def test_slot_ranges_and_error_codes(tmp_path, san):
    k = _constants(san, tmp_path)
    S = k["NSLOTS"]
    # a slot's error bits: timeout (1) before overflow (2) before depth (4); aquad.h's codes
    assert k["err_from_bits"] == [0, -3, -4, -3, -5, -3, -4, -3]
    table = [((0, 0), 1), ((0, S), 1), ((0, S + 1), 0), ((S - 1, 1), 1), ((S, 0), 0), ((-1, 1), 0), ((0, -1), 0)]
    got = [int(x) for x in _run(san, tmp_path, "slots", [list(r) for r, _ in table]).split()]
    assert got == [w for _, w in table]
