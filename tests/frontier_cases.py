"""The level-synchronous frontier engine on the GPU, record by record: aq_level_step, aq_level_step_chained,
aq_level_narrow, aq_level_defer_fold and aq_frontier_integrate against oracle.pyoracle.level_step, which shares
nothing with the code under test.

The bounds. Children, counts and error bits: bit for bit the oracle's (as a set for aq_level_step, whose blocks
append in any order; in input order for aq_level_narrow, which appends behind a block-wide prefix). F(mid) of both
kernels: the committed libm bits of tests/golden. The accumulator d_acc[0..1] is a double-double of terms that are
the reference's own doubles, so with res = fsum(leaves + [-hi, -lo]) -- the correctly rounded exact residual --
|res| <= n * 2^-100 * sum|leaf| (include/aquad.h; derived from dd_add / dd_add_dd, not measured), hi + lo within
one ulp of fsum(leaves), and res == 0 for a single leaf. Every output tensor is filled with a poison value before
a call and nothing past the reported count may change.

AQ_LEVEL_GRID=<n> (read when a context is created) caps aq_level_step's grid, so that a level of a few thousand
records runs several chunks per workgroup; the tests that need it set it and create their own context.

Not collected by name: tests/test_gpu_frontier.py runs this file as one child pytest process that imports torch
before the library is loaded (one HIP runtime for both), and reports each test below as one of its own."""
import functools
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
from conftest import GOLDEN

import mesh_reference as mr
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

COSH4, SIN_RECIP, USER = O.COSH4, O.SIN_RECIP, O.USER
FNAME = {COSH4: "cosh4", SIN_RECIP: "sin_recip", USER: "gauss"}
DOMAIN = {COSH4: (0.0, 5.0), SIN_RECIP: (1e-3, 1.0), USER: (-4.0, 4.0)}
POISON = -7.25
PAD = 8                     # poisoned records past every capacity handed to a kernel
ERR_OVERFLOW, ERR_DEPTH = 2, 4
CHUNK = 1024                # records per workgroup and chunk of aq_level_step (256 lanes x 4), and per chunk of aq_level_narrow
TREE_CAP = 1 << 17          # records per frontier buffer of the whole-tree runs: their widest level holds 27 782


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture
def capped_ctx(monkeypatch):
    """A context of its own whose level steps run at most `grid` workgroups (AQ_LEVEL_GRID, read at create)."""
    made = []

    def make(grid):
        from ppls_amd import Context
        monkeypatch.setenv("AQ_LEVEL_GRID", str(grid))
        made.append(Context(0))
        return made[-1]

    yield make
    for c in made:
        c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _row_set(a):
    """The distinct rows of a (bit patterns), sorted."""
    return np.unique(_bits(np.asarray(a, np.float64).reshape(-1, np.shape(a)[-1])), axis=0)


def _by_l(a):
    return a[np.argsort(a[:, 0], kind="stable")]


def _dev(torch, a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to("cuda:0")


def _poison(torch, rows):
    return torch.full((rows, 4), POISON, dtype=torch.float64, device="cuda:0")


def _untouched(a):
    return bool(np.all(a == POISON))


# ---- the references (CPU, computed once) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records(fid, n):
    """n disjoint records on the integrand's interval: record i starts its cell [lo + w i, lo + w (i + 1)) and takes a
    seeded random share of it, so every l -- and every child's l -- is unique."""
    lo, hi = DOMAIN[fid]
    rng = np.random.default_rng(7919 * fid + n)
    edge = lo + (hi - lo) * np.arange(n + 1) / n
    l = edge[:-1]
    r = l + rng.uniform(0.3, 0.9, n) * (edge[1:] - l)
    assert np.all(l < r) and np.all(r[:-1] < l[1:])
    fin = np.stack([l, r, O.F(l, fid), O.F(r, fid)], axis=1)
    fin.setflags(write=False)
    return fin


def errors(fin, fid):
    """|(larea + rarea) - lrarea| of every record, in the oracle's expressions (aquadPartA.c:185-191)."""
    l, r, fl, fr = (np.ascontiguousarray(c) for c in np.asarray(fin).T)
    mid = (l + r) / 2
    fmid = O.F(mid, fid)
    return np.abs(((fl + fmid) * (mid - l) / 2 + (fmid + fr) * (r - mid) / 2) - (fl + fr) * (r - l) / 2)


@functools.lru_cache(maxsize=None)
def eps_quantile(fid, n, q):
    return float(np.quantile(errors(records(fid, n), fid), q))


@functools.lru_cache(maxsize=None)
def walk(fid, n, eps, d0, levels, max_depth):
    """oracle.level_step iterated `levels` times from records(fid, n) at depth d0: per level (children, leaf areas,
    tasks, error bits)."""
    out, fin = [], records(fid, n)
    for k in range(levels):
        kids, leaves, tasks, err = O.level_step(fin, eps, d0 + k, max_depth, fid)
        out.append((kids, leaves, tasks, err))
        fin = kids
    return out


def check_area(hi, lo, leaves):
    """The double-double accumulator against its terms, exactly (the module's docstring)."""
    leaves = [float(v) for v in leaves]
    res = math.fsum(leaves + [-float(hi), -float(lo)])
    bound = len(leaves) * 2.0 ** -100 * math.fsum(abs(v) for v in leaves)
    want = math.fsum(leaves)
    print("  area: leaves", len(leaves), "residual", res, "bound", bound, "hi+lo", float(hi + lo).hex(), "fsum", want.hex())
    assert abs(res) <= bound, (res, bound)
    assert abs(float(hi + lo) - want) <= math.ulp(want), (float(hi + lo).hex(), want.hex())
    if len(leaves) <= 1:
        assert res == 0.0, res


def check_acc(acc, tasks, leaves, err, depth_plus_1):
    assert (acc[2], acc[3], acc[4], acc[5]) == (tasks, len(leaves), err, depth_plus_1), acc
    assert acc[6] == 0.0 and acc[7] == 0.0
    check_area(acc[0], acc[1], leaves)


# ---- the calls ------------------------------------------------------------------------------------------------
def run_step(torch, ctx, fid, fin, cap, eps, depth, max_depth):
    """aq_level_step on fresh tensors: (*d_n_out, the whole output buffer of cap + PAD records, d_acc)."""
    from ppls_amd.frontier import HipStepper
    tin = _dev(torch, fin)
    out = _poison(torch, cap + PAD)
    nout = torch.full((1,), 12345, dtype=torch.int32, device="cuda:0")
    acc = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = HipStepper(ctx)
    st.step(fid, tin, fin.shape[0], out, cap, eps, depth, max_depth, nout, acc)
    st.sync()
    return int(nout.item()), out.cpu().numpy(), acc.cpu().numpy()


def run_narrow(torch, ctx, fid, fin, cap, eps, d0, levels, max_depth):
    """aq_level_narrow on fresh tensors: (counts, [buf0, buf1] of cap + PAD records each, d_acc)."""
    from ppls_amd.frontier import HipStepper
    n = fin.shape[0]
    assert n <= cap
    bufs = [_poison(torch, cap + PAD), _poison(torch, cap + PAD)]
    bufs[0][:n] = _dev(torch, fin)
    counts = torch.full((d0 + levels + 3,), 77, dtype=torch.int32, device="cuda:0")
    counts[d0] = n
    acc = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = HipStepper(ctx)
    st.narrow(fid, bufs, counts, d0, levels, cap, eps, max_depth, acc)
    st.sync()
    return counts.cpu().numpy(), [b.cpu().numpy() for b in bufs], acc.cpu().numpy()


# ---- 2. F of the level kernels against the committed libm bits -------------------------------------------------------
# in-domain points, rows kept, rows that refine (the one that does not: the smallest subnormal, whose d is 0).
# recip_hard_bits.npz (tests/golden/make_golden.py recip_hard): cosh^4 where 0.5 / exp(x), the second term of glibc's
# cosh, lies within 100 * 2^-106 (relative) above a rounding midpoint -- a reciprocal with one Newton step too few
# passes every point of libm_bits.npz and fails here.
FIXTURE_ROWS = {"libm_bits": (8024, 8021, 8020), "sin_bits": (11559, 11553, 11553), "plugin_bits": (5213, 5211, 5211),
                "recip_hard_bits": (798, 798, 798)}


@functools.lru_cache(maxsize=None)
def fixture_records(name):
    """(fid, records, x, committed F(x)) of a fixture: one record [x - d, x + d] with fl = fr = 3 per in-domain point
    whose midpoint is x exactly, shuffled so that a lane's four records mix the evaluation paths."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = z["x"].view(np.float64)
    with np.errstate(all="ignore"):
        if name in ("libm_bits", "recip_hard_bits"):
            c = z["cosh"].view(np.float64)
            fid, want, dom = COSH4, ((c * c) * c) * c, np.abs(x) <= 170.0   # the reference macro's ((c*c)*c)*c
        elif name == "sin_bits":
            fid, want = SIN_RECIP, z["F"].view(np.float64)
            dom = (np.abs(1.0 / x) < 105414350.0) & (np.abs(x) >= 2.0 ** -900) & (np.abs(x) <= 2.0 ** 900)
        else:
            fid, want, dom = USER, z["F"].view(np.float64), np.ones(x.shape, bool)
        x, want = x[dom], want[dom]
        d = np.ldexp(1.0, np.frexp(x)[1] - 11)      # 2^-10 x the power of two not above |x| (there is none for 0)
        l, r = x - d, x + d
        keep = (x != 0.0) & ((l + r) / 2 == x) & (x - l == d) & (r - x == d)
    n_dom = x.size
    x, want, l, r = x[keep], want[keep], l[keep], r[keep]
    perm = np.random.default_rng(20261).permutation(x.size)
    x, want, l, r = x[perm], want[perm], l[perm], r[perm]
    fin = np.stack([l, r, np.full(x.size, 3.0), np.full(x.size, 3.0)], axis=1)
    kids, leaves, tasks, err = O.level_step(fin, 0.0, 0, 96, fid)
    refines = errors(fin, fid) > 0.0
    print(name, "in-domain points", n_dom, "rows kept", x.size, "rows that refine", int(refines.sum()))
    assert x.size >= 0.99 * n_dom and refines.sum() >= 0.99 * x.size and err == 0
    assert (n_dom, x.size, int(refines.sum())) == FIXTURE_ROWS[name]
    assert kids.shape[0] == 2 * refines.sum()
    # the oracle's own F(mid) is the committed value, row for row
    assert np.array_equal(_bits(kids[0::2, 1]), _bits(x[refines])) and np.array_equal(_bits(kids[0::2, 3]), _bits(want[refines]))
    return fid, fin, kids, leaves, np.stack([x[refines], want[refines]], axis=1)


@pytest.mark.parametrize("kernel", ["step", "narrow"])
@pytest.mark.parametrize("name", ["libm_bits", "sin_bits", "plugin_bits", "recip_hard_bits"])
def test_level_f_bits(ctx, torch, name, kernel):
    """integrand_k<FID, 4> (aq_level_step) and integrand_k<FID, 1> (aq_level_narrow, one level) at every fixture
    point: the children bit for bit the oracle's, their F(mid) the committed libm bits. recip_hard_bits: the points
    where the division inside cosh is hardest to round (FIXTURE_ROWS)."""
    fid, fin, kids, leaves, xf = fixture_records(name)
    n, cap = fin.shape[0], 2 * fin.shape[0]
    if kernel == "step":
        n_out, out, acc = run_step(torch, ctx, fid, fin, cap, 0.0, 0, 96)
        got = out[:n_out]
    else:
        counts, bufs, acc = run_narrow(torch, ctx, fid, fin, cap, 0.0, 0, 1, 96)
        n_out, out = int(counts[1]), bufs[1]
        got = out[:n_out]
        assert np.array_equal(_bits(bufs[0][:n]), _bits(fin)) and _untouched(bufs[0][n:])
        assert np.array_equal(_bits(got), _bits(kids))       # (in input order, too)
    assert n_out == kids.shape[0]
    assert _untouched(out[n_out:])
    assert np.array_equal(_row_set(got), _row_set(kids))
    first = got[0::2]                                        # [l, mid] of every pair: mid = x, F(mid) in column 3
    assert np.array_equal(_row_set(first[:, [1, 3]]), _row_set(xf))
    check_acc(acc, n, leaves, 0, 1)


# ---- 3. aq_level_step at its chunk edges -------------------------------------------------------------------------
STEP_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
STEP_CASES = ([(COSH4, n, None) for n in STEP_N] + [(COSH4, 4101, 1), (COSH4, 4101, 3)] +
              [(f, n, g) for f in (SIN_RECIP, USER) for n, g in ((65, None), (1025, None), (4101, 1))])
STEP_DEPTH = 9


@pytest.mark.parametrize("fid,n,grid", STEP_CASES, ids=["%s-%d-grid%s" % (FNAME[f], n, g) for f, n, g in STEP_CASES])
def test_step_chunk_edges(ctx, capped_ctx, torch, fid, n, grid):
    """One step over n disjoint records of which about a quarter refine, the output buffer exactly as large as the
    children need (the tight fit of pos + 1 < cap_out). grid 1: five chunks in one workgroup, both parities of the
    children counts used more than once; grid 3: workgroups of two, two and one chunk."""
    fin, eps = records(fid, n), eps_quantile(fid, n, 0.75)
    (kids, leaves, tasks, err), = walk(fid, n, eps, STEP_DEPTH, 1, 96)
    assert err == 0 and tasks == n and kids.shape[0] + 2 * leaves.size == 2 * n
    cap = kids.shape[0]
    n_out, out, acc = run_step(torch, capped_ctx(grid) if grid else ctx, fid, fin, cap, eps, STEP_DEPTH, 96)
    print(FNAME[fid], n, "grid", grid, "children", cap, "leaves", leaves.size)
    assert n_out == cap
    assert _untouched(out[cap:])
    assert np.array_equal(_bits(_by_l(out[:cap])), _bits(_by_l(kids)))
    check_acc(acc, n, leaves, 0, STEP_DEPTH + 1)


def test_step_overflow_two_short(ctx, torch):
    """cap_out two records short: the overflow bit, the full count, only children of the oracle's below cap_out (each
    once) and nothing at or past it."""
    fid, n = COSH4, 1025
    fin, eps = records(fid, n), eps_quantile(fid, n, 0.75)
    (kids, leaves, tasks, err), = walk(fid, n, eps, STEP_DEPTH, 1, 96)
    cap = kids.shape[0] - 2
    assert cap > 0
    n_out, out, acc = run_step(torch, ctx, fid, fin, cap, eps, STEP_DEPTH, 96)
    assert n_out == kids.shape[0]
    assert _untouched(out[cap:])
    got, want = _row_set(out[:cap]), _row_set(kids)
    assert got.shape[0] == cap                               # distinct rows
    assert not _untouched(out[:cap]) and (got[:, None, :] == want[None, :, :]).all(axis=2).any(axis=1).all()
    check_acc(acc, n, leaves, ERR_OVERFLOW, STEP_DEPTH + 1)


def test_step_depth_cap(ctx, torch):
    """depth + 1 == max_depth: the refining records raise bit 4 and have no children; every record is a task, only
    the accepted ones count as leaves and in the area."""
    fid, n = COSH4, 1025
    fin, eps = records(fid, n), eps_quantile(fid, n, 0.75)
    (kids, leaves, tasks, err), = walk(fid, n, eps, STEP_DEPTH, 1, STEP_DEPTH + 1)
    assert err == ERR_DEPTH and kids.shape[0] == 0 and 0 < leaves.size < n
    n_out, out, acc = run_step(torch, ctx, fid, fin, 2 * n, eps, STEP_DEPTH, STEP_DEPTH + 1)
    assert n_out == 0 and _untouched(out)
    check_acc(acc, n, leaves, ERR_DEPTH, STEP_DEPTH + 1)


# ---- 4. aq_level_step_chained -------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 700, 1025, 3000])
def test_chained_counts(ctx, torch, count):
    """The input count read on the device and clamped to n_in_max = 1025; the children appended behind the 10 records
    counts[d + 1] already holds. A count of 0 leaves the accumulator and counts[d + 1] as they were."""
    from ppls_amd.frontier import HipStepper
    fid, n_max, d, preset = COSH4, 1025, 5, 10
    fin = records(fid, 3000)
    eps = float(np.quantile(errors(fin[:n_max], fid), 0.75))   # a quarter of the first 1025 refine
    m = min(count, n_max)
    kids, leaves, tasks, err = O.level_step(fin[:m], eps, d, 96, fid)
    assert err == 0 and (m < 700 or 0 < leaves.size < m)
    cap = preset + kids.shape[0]
    tin, out = _dev(torch, fin), _poison(torch, cap + PAD)
    counts = torch.zeros(d + 3, dtype=torch.int32, device="cuda:0")
    counts[d], counts[d + 1], counts[d + 2] = count, preset, 55
    acc0 = np.array([1.5, 2.0 ** -60, 7.0, 3.0, 0.0, 2.0, 0.0, 0.0]) if count == 0 else np.zeros(8)
    acc = _dev(torch, acc0)
    torch.cuda.synchronize()
    st = HipStepper(ctx)
    st.chain_step(fid, tin, counts, d, n_max, out, cap, eps, 96, acc)
    st.sync()
    counts, out, acc = counts.cpu().numpy(), out.cpu().numpy(), acc.cpu().numpy()
    assert counts[d] == count and counts[d + 2] == 55 and np.all(counts[:d] == 0)
    assert counts[d + 1] == preset + kids.shape[0]
    assert _untouched(out[:preset]) and _untouched(out[cap:])
    assert np.array_equal(_bits(_by_l(out[preset:cap])), _bits(_by_l(kids)))
    if count == 0:
        assert np.array_equal(_bits(acc), _bits(acc0))
    else:
        check_acc(acc, m, leaves, 0, d + 1)


# ---- 5. aq_level_narrow, in order ---------------------------------------------------------------------------------
NARROW_N = (1, 63, 64, 65, 1023, 1024, 1025, 2500)
NARROW_CASES = ([(COSH4, n, d0, lv) for n in NARROW_N for d0 in (0, 7) for lv in (1, 2, 3)] +
                [(f, n, d0, lv) for f in (SIN_RECIP, USER) for n in (65, 1025) for d0 in (0, 7) for lv in (1, 2, 3)])
NARROW_Q = 0.4   # eps: this quantile of the start frontier's errors -- most records refine, and their children again


def _check_narrow(counts, bufs, acc, fid, n, eps, d0, levels, max_depth, cap):
    ref = walk(fid, n, eps, d0, levels, max_depth)
    assert np.all(counts[:d0] == 77) and counts[d0] == n and np.all(counts[d0 + levels + 1:] == 77)
    for k, (kids, _, _, _) in enumerate(ref):
        assert counts[d0 + k + 1] == kids.shape[0], (k, counts)
    last = ref[-1][0]
    out = bufs[levels & 1]
    assert np.array_equal(_bits(out[:last.shape[0]]), _bits(last))
    assert _untouched(bufs[0][cap:]) and _untouched(bufs[1][cap:])
    tasks = sum(t for _, _, t, _ in ref)
    err = 0
    for e in ref:
        err |= e[3]
    deepest = max(d0 + k + 1 for k, e in enumerate(ref) if e[2])
    check_acc(acc, tasks, np.concatenate([e[1] for e in ref]), err, deepest)
    return ref


@pytest.mark.parametrize("fid,n,d0,levels", NARROW_CASES,
                         ids=["%s-%d-d%d-l%d" % (FNAME[f], n, d, lv) for f, n, d, lv in NARROW_CASES])
def test_narrow_in_order(ctx, torch, fid, n, d0, levels):
    """`levels` levels in one launch: every level's count, the last level's children whole, in order and in
    d_buf{levels & 1}, the other buffer holding the level before; 2500 records run three chunks at every level."""
    fin, eps = records(fid, n), eps_quantile(fid, n, NARROW_Q)
    ref = walk(fid, n, eps, d0, levels, 96)
    sizes = [n] + [e[0].shape[0] for e in ref]
    print(FNAME[fid], "start", n, "d0", d0, "records per level", sizes)
    if n == 2500:
        assert all(s > 2 * CHUNK for s in sizes[:levels])
    cap = max(sizes + [2])
    counts, bufs, acc = run_narrow(torch, ctx, fid, fin, cap, eps, d0, levels, 96)
    _check_narrow(counts, bufs, acc, fid, n, eps, d0, levels, 96, cap)
    # the other buffer: the input of the last level (the start frontier where levels == 1), and nothing behind it
    before = fin if levels == 1 else ref[-2][0]
    other = bufs[(levels & 1) ^ 1]
    assert np.array_equal(_bits(other[:before.shape[0]]), _bits(before))
    written = [sizes[k] for k in range(levels + 1) if (k & 1) == ((levels & 1) ^ 1)]
    assert _untouched(other[max(written):])
    assert _untouched(bufs[levels & 1][max(sizes[k] for k in range(levels + 1) if (k & 1) == (levels & 1)):])


def test_narrow_zero_levels(ctx, torch):
    """levels = 0 returns AQ_OK and touches nothing."""
    from ppls_amd.frontier import HipStepper
    fin = records(COSH4, 65)
    bufs = [_poison(torch, 200), _poison(torch, 200)]
    bufs[0][:65] = _dev(torch, fin)
    counts = torch.full((12,), 77, dtype=torch.int32, device="cuda:0")
    counts[3] = 65
    acc0 = np.array([1.5, 2.0 ** -60, 7.0, 3.0, 0.0, 2.0, 0.0, 0.0])
    acc = _dev(torch, acc0)
    torch.cuda.synchronize()
    st = HipStepper(ctx)
    st.narrow(COSH4, bufs, counts, 3, 0, 200, 0.0, 96, acc)
    st.sync()
    want = np.full(12, 77)
    want[3] = 65
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc0))
    assert np.array_equal(_bits(bufs[0][:65].cpu().numpy()), _bits(fin))
    assert _untouched(bufs[0][65:].cpu().numpy()) and _untouched(bufs[1].cpu().numpy())


def test_narrow_capacity(ctx, torch):
    """cap equal to the widest level's children: clean. Two less: bit 2, the level's count still whole, every record
    below cap the oracle's and in order, nothing at or past cap."""
    fid, n, d0, levels = COSH4, 1025, 4, 2
    fin, eps = records(fid, n), eps_quantile(fid, n, NARROW_Q)
    ref = walk(fid, n, eps, d0, levels, 96)
    sizes = [n] + [e[0].shape[0] for e in ref]
    assert sizes[2] > sizes[1] > sizes[0]                    # the widest level is the last
    counts, bufs, acc = run_narrow(torch, ctx, fid, fin, sizes[2], eps, d0, levels, 96)
    _check_narrow(counts, bufs, acc, fid, n, eps, d0, levels, 96, sizes[2])
    cap = sizes[2] - 2
    counts, bufs, acc = run_narrow(torch, ctx, fid, fin, cap, eps, d0, levels, 96)
    assert [int(counts[d0 + k]) for k in range(3)] == sizes
    assert np.array_equal(_bits(bufs[0][:cap]), _bits(ref[1][0][:cap]))
    assert _untouched(bufs[0][cap:]) and _untouched(bufs[1][sizes[1]:])
    check_acc(acc, sizes[0] + sizes[1], np.concatenate([ref[0][1], ref[1][1]]), ERR_OVERFLOW, d0 + 2)


def test_narrow_depth_cap(ctx, torch):
    """max_depth = d0 + 2 under three levels: the second level's refining records raise bit 4 and have no children,
    the third level sees no record."""
    fid, n, d0, levels = COSH4, 1025, 7, 3
    fin, eps = records(fid, n), eps_quantile(fid, n, NARROW_Q)
    ref = walk(fid, n, eps, d0, levels, d0 + 2)
    sizes = [n] + [e[0].shape[0] for e in ref]
    assert sizes[1] > 0 and sizes[2:] == [0, 0] and ref[1][3] == ERR_DEPTH and ref[2][2] == 0
    assert 0 < ref[1][1].size < sizes[1]
    cap = max(sizes)
    counts, bufs, acc = run_narrow(torch, ctx, fid, fin, cap, eps, d0, levels, d0 + 2)
    _check_narrow(counts, bufs, acc, fid, n, eps, d0, levels, d0 + 2, cap)
    assert acc[4] == ERR_DEPTH and acc[5] == d0 + 2
    assert np.array_equal(_bits(bufs[1][:sizes[1]]), _bits(ref[0][0])) and _untouched(bufs[1][sizes[1]:])
    assert np.array_equal(_bits(bufs[0][:n]), _bits(fin)) and _untouched(bufs[0][n:])


# ---- 7. folds -----------------------------------------------------------------------------------------------------
FOLD_N, FOLD_GRID = 262144, 256     # 256 workgroups of one chunk each: 256 partial rows a step
LP_CAP = 65536                      # rows the library holds for one deferred fold (aq_abi.inc)


@functools.lru_cache(maxsize=None)
def fold_reference():
    """(records, the one step's leaf areas, their exact sum, sum |leaf|): every record accepts at eps = 1e300."""
    fin = records(COSH4, FOLD_N)
    kids, leaves, tasks, err = O.level_step(fin, 1e300, 0, 96, COSH4)
    assert kids.shape[0] == 0 and leaves.size == FOLD_N and err == 0
    X = 0                                                    # the exact sum as an integer multiple of 2^-1200
    for v in leaves.tolist():
        m, e = math.frexp(v)
        X += int(m * 2 ** 53) << (e - 53 + 1200)
    S = Fraction(X, 2 ** 1200)
    assert float(S) == math.fsum(leaves)
    return fin, leaves, S, Fraction(math.fsum(np.abs(leaves)))


def _fold_area(acc, steps):
    fin, leaves, S, A = fold_reference()
    got = Fraction(float(acc[0])) + Fraction(float(acc[1]))
    bound = steps * FOLD_N * Fraction(1, 2 ** 100) * A       # (A: one step's sum |leaf| -- the tighter reading)
    print("  fold: steps", steps, "residual", float(got - steps * S), "bound", float(bound))
    assert (acc[2], acc[3], acc[4], acc[5]) == (steps * FOLD_N, steps * FOLD_N, 0, 1), acc
    assert abs(got - steps * S) <= bound


def test_fold_past_lp_cap(capped_ctx, torch):
    """300 deferred steps into one accumulator: the pending rows reach LP_CAP after step 256, so step 257 folds
    early; no row is lost or folded twice."""
    from ppls_amd.frontier import HipStepper
    fin = fold_reference()[0]
    assert 256 * FOLD_GRID == LP_CAP and FOLD_N == FOLD_GRID * CHUNK
    c = capped_ctx(FOLD_GRID)
    tin, out = _dev(torch, fin), _poison(torch, PAD)
    nout = torch.full((1,), 12345, dtype=torch.int32, device="cuda:0")
    acc = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = HipStepper(c)
    st.defer_folds(True)
    try:
        for _ in range(300):
            st.step(COSH4, tin, FOLD_N, out, 2, 1e300, 0, 96, nout, acc)
    finally:
        st.defer_folds(False)
    st.sync()
    assert int(nout.item()) == 0 and _untouched(out.cpu().numpy())
    _fold_area(acc.cpu().numpy(), 300)


def test_fold_on_accumulator_change(capped_ctx, torch):
    """Deferred steps into A, B, A, B, A, then aq_synchronize alone with deferring left on: three steps in A, two in
    B, exactly. Turning deferring off afterwards, with nothing pending, changes nothing."""
    from ppls_amd.frontier import HipStepper
    fin = fold_reference()[0]
    c = capped_ctx(FOLD_GRID)
    tin, out = _dev(torch, fin), _poison(torch, PAD)
    nout = torch.full((1,), 12345, dtype=torch.int32, device="cuda:0")
    A, B = (torch.zeros(8, dtype=torch.float64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    st = HipStepper(c)
    st.defer_folds(True)
    try:
        for acc in (A, B, A, B, A):
            st.step(COSH4, tin, FOLD_N, out, 2, 1e300, 0, 96, nout, acc)
        c.synchronize()
        a, b = A.cpu().numpy(), B.cpu().numpy()
        _fold_area(a, 3)
        _fold_area(b, 2)
    finally:
        st.defer_folds(False)
    st.sync()
    assert np.array_equal(_bits(A.cpu().numpy()), _bits(a)) and np.array_equal(_bits(B.cpu().numpy()), _bits(b))
    assert _untouched(out.cpu().numpy())


def test_defer_off_with_nothing_pending(ctx, torch):
    """On and off again with no step between: no fold runs, an accumulator used before keeps its bits."""
    from ppls_amd.frontier import HipStepper
    fid, n = COSH4, 65
    fin, eps = records(fid, n), eps_quantile(fid, n, 0.75)
    (kids, leaves, tasks, err), = walk(fid, n, eps, 0, 1, 96)
    tin, out = _dev(torch, fin), _poison(torch, 2 * n)
    nout = torch.full((1,), 12345, dtype=torch.int32, device="cuda:0")
    acc = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = HipStepper(ctx)
    st.defer_folds(False)                                    # off while off
    st.step(fid, tin, n, out, 2 * n, eps, 0, 96, nout, acc)  # not deferred: folded with the step
    st.sync()
    before = acc.cpu().numpy()
    check_acc(before, n, leaves, 0, 1)
    st.defer_folds(True)
    st.defer_folds(False)
    st.sync()
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(before))


# ---- 8. whole trees through aq_frontier_integrate -----------------------------------------------------------------
with open(os.path.join(GOLDEN, "edges.json")) as _f:
    EDGES = json.load(_f)
EDGE_FID = {"cosh4": COSH4, "sin_recip": SIN_RECIP, "gauss": USER}
# every leaf area of this tree is a multiple of 2^-1074 and the total is below 2^-1022: every partial sum, in any
# order, is exact in double (tests/test_gpu_matrix.py EXACT_AREA)
EXACT_AREA = ("user_tail_eps0",)


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """The tree walked with oracle.level_step: (tasks per level, leaves per level, fsum of the leaf areas)."""
    g = EDGES[name]
    fid = EDGE_FID[g["integrand"]]
    a, b = float.fromhex(g["a_hex"]), float.fromhex(g["b_hex"])
    fin = np.array([[a, b, O.F(a, fid), O.F(b, fid)]])
    tpl, lpl, areas, depth = [], [], [], 0
    while fin.shape[0]:
        kids, leaves, tasks, err = O.level_step(fin, g["eps"], depth, 96, fid)
        assert err == 0
        tpl.append(tasks)
        lpl.append(leaves.size)
        areas.extend(leaves.tolist())
        fin, depth = kids, depth + 1
    assert (tpl, lpl) == (g["tasks_per_level"], g["leaves_per_level"])
    return tpl, lpl, math.fsum(areas)


def _check_tree(r, tasks, leaves, levels, tpl, lpl, want, exact):
    assert (r.tasks, r.accepted, r.levels) == (tasks, leaves, levels), r
    assert r.tasks_per_level == tpl and r.leaves_per_level == lpl
    print("  area", float(r.area).hex(), "want", float(want).hex())
    if exact or want == 0.0:
        assert r.area == want, (float(r.area).hex(), float(want).hex())
    else:
        assert abs(r.area - want) <= math.ulp(want), (float(r.area).hex(), float(want).hex())


def _edge_tree(c, name, sync_every):
    from ppls_amd import Problem
    from ppls_amd.frontier import HipStepper
    g = EDGES[name]
    tpl, lpl, want = edge_reference(name)
    assert want == 0.0 or abs(want - float.fromhex(g["area_hex"])) <= math.ulp(want)
    assert (want == 0.0) == (float.fromhex(g["area_hex"]) == 0.0)
    p = Problem(EDGE_FID[g["integrand"]], float.fromhex(g["a_hex"]), float.fromhex(g["b_hex"]), g["eps"])
    r = HipStepper(c).integrate_one_gpu(p, TREE_CAP, sync_every)
    _check_tree(r, g["tasks"], g["leaves"], g["levels"], tpl, lpl, want, name in EXACT_AREA)


def _mesh_tree(c, case, sync_every):
    from ppls_amd import Problem
    from ppls_amd.frontier import HipStepper
    name, fid, a, b, eps = case
    want = O.integrate(fid, a, b, eps)
    m = mr.reference_mesh(fid, a, b, eps)
    r = HipStepper(c).integrate_one_gpu(Problem(fid, a, b, eps), TREE_CAP, sync_every)
    _check_tree(r, want.tasks, want.leaves, want.levels, want.tasks_per_level, want.leaves_per_level,
                float(m.cum[-1]), False)


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_tree_frontier(ctx, name, sync_every):
    """A tree of tests/golden/edges.json through aq_frontier_integrate: the fixture's counts and histograms, the area
    within one ulp of the correctly rounded sum of the oracle's leaf areas (exactly it where every sum is exact)."""
    _edge_tree(ctx, name, sync_every)


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_mesh_case_frontier(ctx, case, sync_every):
    _mesh_tree(ctx, case, sync_every)


@pytest.mark.parametrize("name", ["cosh4_0_5_1e-6", "cosh_170"])
def test_tree_capped_grid(capped_ctx, name):
    """Two workgroups for every level step: the wide levels run many chunks per workgroup."""
    c = capped_ctx(2)
    if name in EDGES:
        _edge_tree(c, name, 4)
    else:
        _mesh_tree(c, [k for k in mr.CASES if k[0] == name][0], 4)
