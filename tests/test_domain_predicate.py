"""The domain predicate that the host's argument checks and the device-resident batch's check kernel share
(`ppls_amd/csrc/aq_domain.h`), compiled with g++ and compared with the documented rule -- include/aquad.h's
AQ_EINVAL text: finite bounds, b >= a, each bound 0 or 2^-900 <= |x| <= 2^900, cosh^4 within |x| <= 170, and the
shipped plug-ins' own domains (within +-1e150; a finite theta row with a non-zero inverse scale) -- on a fixed
table of edge values, every ordered pair of them as [a, b]."""
import itertools
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "domain_check.cpp")
INC = [os.path.join(ROOT, "ppls_amd", "csrc"), os.path.join(ROOT, "include")]
COSH4, SIN_RECIP, USER, PARAM = 0, 1, 2, 3
INF, NAN = math.inf, math.nan
LO, HI = 2.0 ** -900, 2.0 ** 900
EDGES = [0.0, -0.0, LO, -LO, math.nextafter(LO, 0.0), -math.nextafter(LO, 0.0), 5e-324, 1e-300, HI, -HI,
         math.nextafter(HI, INF), -math.nextafter(HI, INF), 170.0, -170.0, math.nextafter(170.0, INF),
         -math.nextafter(170.0, INF), 171.0, 1.0, -1.0, 5.0, 1e150, -1e150, math.nextafter(1e150, INF),
         -math.nextafter(1e150, INF), NAN, INF, -INF]
THETAS = [(0.0, 1.0), (0.5, -3.0), (1e150, 1e150), (-1e150, -1e150), (0.0, 0.0), (0.0, -0.0), (NAN, 1.0), (0.0, NAN),
          (INF, 1.0), (0.0, -INF), (math.nextafter(1e150, INF), 1.0), (0.0, -math.nextafter(1e150, INF)), (0.0, 5e-324)]


def documented(f, a, b, th=None):
    """include/aquad.h, AQ_EINVAL and the integrands' comments, restated."""
    if not (math.isfinite(a) and math.isfinite(b)) or b < a:
        return False
    for x in (a, b):
        if x != 0.0 and not (LO <= abs(x) <= HI):
            return False
    if f == COSH4:
        return max(abs(a), abs(b)) <= 170.0
    if f in (USER, PARAM) and not (a >= -1e150 and b <= 1e150):
        return False
    if f == PARAM:
        return all(math.isfinite(t) and abs(t) <= 1e150 for t in th) and th[1] != 0.0
    return True


def test_shared_predicate_is_the_documented_rule(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "domain_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC[0], "-I", INC[1], SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [(f, a, b, (0.0, 1.0)) for f in (COSH4, SIN_RECIP, USER, PARAM) for a, b in itertools.product(EDGES, EDGES)]
    rows += [(PARAM, a, b, th) for th in THETAS for a, b in [(0.0, 1.0), (-2.0, -2.0), (LO, HI), (-1.0, 1e150), (1.0, 0.5)]]
    path = tmp_path / "rows.txt"
    path.write_text("".join("%d %s %s %s\n" % (f, float(a).hex(), float(b).hex(), " ".join(float(t).hex() for t in th))
                            for f, a, b, th in rows))
    got = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert len(got) == len(rows)
    want = [documented(*r) for r in rows]
    bad = [(r, g) for r, g, w in zip(rows, got, want) if (g == "1") != w]
    assert not bad, bad[:10]
    # the table reaches both answers for every family, and each edge the issue names
    for f in (COSH4, SIN_RECIP, USER, PARAM):
        assert {w for r, w in zip(rows, want) if r[0] == f} == {True, False}
    assert documented(COSH4, 170.0, 170.0) and not documented(COSH4, 0.0, math.nextafter(170.0, INF))
    assert documented(SIN_RECIP, -HI, HI) and not documented(SIN_RECIP, 0.0, math.nextafter(HI, INF))
    assert documented(SIN_RECIP, -LO, LO) and not documented(SIN_RECIP, 0.0, math.nextafter(LO, 0.0))
    assert documented(COSH4, -0.0, 0.0) and not documented(COSH4, 1.0, -1.0)
