"""Shared by the duplicate-group tests (tests/test_gpu_components.py,
tests/test_components_cpu.py): the truth -- the pairs of the self range search
(tests/self_cases.py range_self_truth, from the oracle's ranked lists), joined
by a plain union-find, every row labelled with the smallest row of its
component -- and the chain column, whose components hold together only through
long runs of links.  CPU only."""
from __future__ import annotations

import numpy as np

from self_cases import f32, range_self_truth


def components_truth(full, threshold, metric, ids=None):
    """(labels uint32 [n], components, pairs) of the ranked lists ``full``:
    the connected components of range_self_truth's pairs; ``ids``: the
    ascending parent row numbers the labels are reported in."""
    offsets, idx, _ = range_self_truth(full, threshold, metric)
    n = offsets.size - 1
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(n):
        js = idx[offsets[i]:offsets[i + 1]].astype(np.int64)
        if js.size == 0:
            continue
        ri = find(i)
        for j in js[parent[js] != ri].tolist():  # (already under i's root: nothing to join)
            rj = find(j)
            if rj != ri:
                lo, hi = (ri, rj) if ri < rj else (rj, ri)
                parent[hi] = lo
                ri = lo
    labels = np.array([find(i) for i in range(n)], dtype=np.int64)
    # the lower root always wins, so a root is the smallest row of its component
    components = int((labels == np.arange(n)).sum())
    if ids is not None:
        labels = np.asarray(ids, dtype=np.int64)[labels]
    return labels.astype(np.uint32), components, int(offsets[-1])


CHAIN_THRESHOLD = 1.5
CHAIN_LENGTHS = (257, 130, 64, 3, 2)


def chain_column(n, d, seed):
    """(column f32 [n, d], chains, isolated) for euclidean at CHAIN_THRESHOLD.
    Chain c: CHAIN_LENGTHS[c] points on a line at spacing 1.0 -- only
    consecutive points are within 1.5, so the chain is one component only
    through all its links -- centred on axis 0, 8 (c + 1) away from it on axis
    1 + c, so no two chains come closer than 8.  The points sit at permuted
    rows (``chains[c]``: the rows in line order), so links cross block and tile
    bounds, and the smallest row of a chain of three or more points is an
    interior point.  The other rows (``isolated``) are 3 apart on axis 0 and 40
    away on the last axis.  Every coordinate is a small integer: the squared
    distances 1 and 4 are far from the threshold's 2.25 in f32."""
    rs = np.random.RandomState(seed)
    assert d >= len(CHAIN_LENGTHS) + 2 and n > sum(CHAIN_LENGTHS)
    perm = rs.permutation(n)
    c = np.zeros((n, d), dtype=np.float32)
    chains, off = [], 0
    for ci, L in enumerate(CHAIN_LENGTHS):
        rows = perm[off:off + L].copy()
        off += L
        if L >= 3:
            lo = int(np.argmin(rows))
            if lo in (0, L - 1):  # the smallest row: an interior point
                rows[lo], rows[L // 2] = rows[L // 2], rows[lo]
        c[rows, 0] = np.arange(L) - L // 2
        c[rows, 1 + ci] = 8.0 * (ci + 1)
        chains.append(rows.astype(np.int64))
    isolated = np.sort(perm[off:]).astype(np.int64)
    c[isolated, 0] = 3.0 * (np.arange(isolated.size) - isolated.size // 2)
    c[isolated, d - 1] = 40.0
    return f32(c), chains, isolated
