"""Mesh coarsening on the CPU (no GPU, nothing of the library): what aq_mesh_thresholds_batch, aq_mesh_budget_batch
and aq_mesh_coarsen_batch must return, restated BY DEFINITION from a reference Batch's node arrays alone -- offsets, x,
f, level.

Per row the binary tree is rebuilt from the depth sequence of its leaves, recursively: the node of depth k over leaf j
is that leaf when level says so, else two children of depth k + 1. Every internal node's |d| comes from
mesh_refine_reference.leaf_d's expressions (aquadPartA.c:185-191) on the node's l, mid, r -- the bounds of its first
leaf, of its right child's first leaf, and of the leaf behind it. From these:

  thresholds   the minimum of |d| over the node whose midpoint a leaf starts at, and over its ancestors
  coarsen      top down, the first node with not (|d| > e) becomes a leaf; the rows are formed by
               mesh_refine_reference._row, cum by Fractions
  budget_eps   the K-th largest threshold of a row of more than K leaves, by sorting

No positions, no searches, no parent chains: nothing here is shared with the kernels.

A helper module, not a conftest: the CPU and GPU tests import it and share its cached results.
"""
import functools
import sys

import numpy as np

import mesh_batch_reference as mbr
import mesh_refine_reference as mrr

sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))


class Tree:
    """One row's tree: per internal node (preorder, so a parent comes before its children) the leaf indices of its
    start, midpoint and end, its depth, its parent (-1: the root) and its two children (>= 0: an internal node, < 0:
    leaf ~c); `d`, the nodes' |d|; `lv`, the row's leaf records (mesh_refine_reference.leaves_of); `root`."""

    def __init__(self, lv):
        self.lv = lv
        depth = lv[:, 6].astype(np.int64)
        L = depth.size
        start, mid, end, dep, parent, kids = [], [], [], [], [], []

        def build(k, j, up):
            """The node of depth k that starts at leaf j: (its reference, the leaf behind it)."""
            assert j < L and depth[j] >= k, "the depths are no tree's"
            if depth[j] == k:
                return ~j, j + 1
            i = len(start)
            start.append(j), mid.append(-1), end.append(-1), dep.append(k), parent.append(up), kids.append([0, 0])
            kids[i][0], m = build(k + 1, j, i)
            kids[i][1], e = build(k + 1, m, i)
            mid[i], end[i] = m, e
            return i, e

        self.root, e = build(0, 0, -1)
        assert e == L, "the depths are no tree's"
        self.start, self.mid, self.end, self.depth, self.parent = (np.array(v, np.int64) for v in (start, mid, end, dep, parent))
        self.kids = kids
        x = np.concatenate([lv[:, 0], lv[-1:, 1]])      # the L + 1 even nodes
        f = np.concatenate([lv[:, 2], lv[-1:, 4]])
        s, m, e = self.start, self.mid, self.end
        self.rec = np.stack([x[s], x[e], f[s], f[m], f[e], x[m], self.depth.astype(np.float64)], axis=1)
        self.d = np.abs(mrr.leaf_d(self.rec)[0]) if s.size else np.empty(0)
        assert not np.isnan(self.d).any()


_TREES = {}


def tree(batch, i):
    """Row i's Tree, built once per Batch object (which the cache keeps alive, so its id stays its own)."""
    key = (id(batch), i)
    if key not in _TREES:
        _TREES[key] = (batch, Tree(mrr.leaves_of(batch, i)))
    return _TREES[key][1]


def thresholds(batch):
    """aq_mesh_thresholds_batch: per node +inf at a row's two ends, 0 at its odd nodes, the threshold at its even
    interior nodes."""
    thr = np.zeros(batch.n_nodes)
    for i in range(len(batch.offsets) - 1):
        o0, o1 = int(batch.offsets[i]), int(batch.offsets[i + 1])
        if o1 - o0 < 3:
            continue
        t = tree(batch, i)
        thr[o0] = thr[o1 - 1] = np.inf
        low = np.empty(t.d.size)
        for k in range(t.d.size):                       # preorder: the parent's minimum is known
            low[k] = t.d[k] if t.parent[k] < 0 else min(t.d[k], low[t.parent[k]])
            thr[o0 + 2 * t.mid[k]] = low[k]
    return thr


def _row_eps(batch, eps):
    n = len(batch.offsets) - 1
    return np.full(n, float(eps)) if np.ndim(eps) == 0 else np.asarray(eps, np.float64).reshape(n)


def coarsen(batch, eps):
    """aq_mesh_coarsen_batch: the Batch of `batch`'s rows at eps (a float, or one per row; negative or NaN: the row
    unchanged). A row in which nothing merges is the input's row."""
    out = []
    for i, e in enumerate(_row_eps(batch, eps)):
        row = batch.rows[i]
        if row is None or not e >= 0.0:
            out.append(row)
            continue
        t = tree(batch, i)
        keep, merged, todo = [], False, [t.root]
        while todo:
            c = todo.pop()
            if c < 0:
                keep.append(t.lv[~c])
            elif t.d[c] > e:                            # :191, strict
                todo.extend(t.kids[c])
            else:
                keep.append(t.rec[c])
                merged = True
        out.append(mrr._row(np.array(keep)) if merged else row)
    return mbr.Batch(out)


def budget_eps(batch, max_leaves):
    """aq_mesh_budget_batch: -1.0 for a row of at most max_leaves leaves, else its max_leaves-th largest threshold."""
    thr = thresholds(batch)
    eps = np.full(len(batch.offsets) - 1, -1.0)
    for i in range(eps.size):
        o0, o1 = int(batch.offsets[i]), int(batch.offsets[i + 1])
        if o1 - o0 >= 3 and (o1 - o0 - 1) // 2 > max_leaves:
            eps[i] = np.sort(thr[o0 + 2:o1 - 1:2])[-max_leaves]
    return eps


# ---- the synthetic row `comb` -------------------------------------------------------------------------------------
COMB_DEPTH = 100


def comb_row():
    """[0, 1] with leaves [2^-k, 2^-(k-1)] at depth k = 1 .. 99 and [0, 2^-100], [2^-100, 2^-99] at depth 100: every
    bound and mid an exact power of two, F(x) = x^-1/2 with F(0) = 0. Its positions cross bit 64 of the 128-bit word
    and its depth exceeds AQ_DEFAULT_MAX_DEPTH."""
    F = lambda x: np.where(x > 0, np.maximum(x, 1e-300) ** -0.5, 0.0)   # noqa: E731
    D = COMB_DEPTH
    l = np.array([0.0] + [2.0 ** -k for k in range(D, 0, -1)])
    r = np.array([2.0 ** -k for k in range(D, 0, -1)] + [1.0])
    depth = np.array([D] + list(range(D, 0, -1)), np.float64)
    mid = (l + r) / 2
    return mrr._row(np.stack([l, r, F(l), F(mid), F(r), mid, depth], axis=1))


@functools.lru_cache(maxsize=None)
def comb():
    """The Batch [an ordinary row, comb, an ordinary row]: comb sits at an odd offset."""
    _, _, _, _, _, sin = mbr.case("sin")
    batch = mbr.Batch([sin.rows[1], comb_row(), sin.rows[2]])
    assert batch.offsets[1] % 2 == 1
    return batch


@functools.lru_cache(maxsize=None)
def fine(name):
    """The fine Batch of a case: mesh_batch_reference's four, or comb."""
    return comb() if name == "comb" else mbr.case(name)[5]
