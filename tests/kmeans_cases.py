"""The restatement of pmm_kmeans_f32_corpus (include/pmm.h) that the k-means
tests compare against, bit for bit, and the inputs they share.

``assign`` is ``oracle.topk(X, C, 1, metric)``; ``update`` is a plain NumPy
loop over a cluster's members in ascending row order, cut into pieces of ``P``
consecutive members: each piece summed sequentially in f64 from +0.0, the piece
sums added sequentially from +0.0, divided by the count and rounded to f32.
``piece=None`` sums a cluster in ONE level instead, which tests/test_kmeans_cpu.py
uses to show that the piece order is visible in the result.

A plain module, not a test file.
"""
from __future__ import annotations

import numpy as np

import oracle

P = 256  # PMM_KMEANS_PIECE
NO_GROUP = np.uint32(0xFFFFFFFF)
QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
ZERO_NORM = np.float32(1e-6)  # the reference's zero-norm rule
EUC, COS = oracle.EUCLIDEAN, oracle.COSINE


def assign(x, c, metric):
    """(labels uint32 [n], scores float32 [n]): the exact f32 top-1 of every
    row among the rows of c; a NaN best score gives NO_GROUP and the quiet NaN."""
    idx, sc = oracle.topk(x, c, 1, metric)
    labels = idx[:, 0].astype(np.uint32)
    scores = sc[:, 0].astype(np.float32)
    nan = np.isnan(scores)
    labels[nan] = NO_GROUP
    scores[nan] = QNAN
    return labels, scores


def cluster_sum(x, members, norms, piece=P):
    """(f64 sum per column, counted members) of one cluster's terms; norms:
    the rows' f32 cosine norms (cosine) or None (euclidean)."""
    d = x.shape[1]
    step = piece if piece else max(1, len(members))
    total = np.zeros(d, dtype=np.float64)
    count = 0
    for p0 in range(0, len(members), step):
        acc = np.zeros(d, dtype=np.float64)
        for i in members[p0:p0 + step]:
            if norms is None:
                acc = acc + x[i].astype(np.float64)
            else:
                if norms[i] <= ZERO_NORM:
                    continue  # keeps its place in the piece, adds no term, is not counted
                acc = acc + x[i].astype(np.float64) / np.float64(norms[i])
            count += 1
        total = total + acc
    return total, count


def update(x, labels, c, metric, norms=None, piece=P):
    out = c.copy()
    with np.errstate(all="ignore"):
        for k in range(c.shape[0]):
            members = np.flatnonzero(labels == np.uint32(k))
            total, count = cluster_sum(x, members, norms if metric == COS else None, piece)
            if count > 0:
                out[k] = (total / np.float64(count)).astype(np.float32)
    return out


def kmeans_ref(x, init, metric, max_iter, piece=P):
    """(centroids, labels, scores, updates, converged, changes): ``changes[u]``
    is the number of labels the assignment after update u + 1 changed."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = np.ascontiguousarray(init, dtype=np.float32).copy()
    norms = oracle.norms(x) if metric == COS else None
    updates, converged, prev, changes = 0, False, None, []
    while True:
        labels, scores = assign(x, c, metric)
        if updates > 0:
            changes.append(int(np.count_nonzero(labels != prev)))
            if changes[-1] == 0:
                converged = True
                break
        if updates == max_iter:
            break
        c = update(x, labels, c, metric, norms, piece)
        prev = labels
        updates += 1
    return c, labels, scores, updates, converged, changes


def planted(n, d, centres, seed, noise=1.0, spread=3.0):
    """n float32 rows drawn around `centres` planted centres (round-robin, so
    every centre has rows), the planted label of every row, and the centres."""
    rs = np.random.RandomState(seed)
    mu = (spread * rs.randn(centres, d)).astype(np.float32)
    truth = (np.arange(n) % centres).astype(np.uint32)
    x = (mu[truth] + noise * rs.randn(n, d)).astype(np.float32)
    return np.ascontiguousarray(x), truth, mu


def default_init(x, k, seed=0):
    ids = np.sort(np.random.RandomState(seed).choice(x.shape[0], k, replace=False))
    return np.ascontiguousarray(x[ids])


BIG = np.float32(2.0 ** 54)


def piece_edge_rows(sizes=(255, 256, 257, 512, 513), seed=5):
    """(x [sum(sizes), 4], init [len(sizes), 4]): cluster c has exactly
    sizes[c] members under euclidean (column 0 = c * 2^58 separates them; the
    rows of the clusters interleave), and columns 1 and 2 mix the magnitudes
    2^54 and 1 so that the order of the f64 additions shows in the f32 mean:
    column 1 is +2^54 at a cluster's first member, -2^54 at its last and 1 in
    between; column 2 draws from {+2^54, -2^54, 1, 3}."""
    rs = np.random.RandomState(seed)
    cid = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    cid = cid[rs.permutation(cid.size)]
    x = np.zeros((cid.size, 4), dtype=np.float32)
    x[:, 0] = cid.astype(np.float32) * np.float32(2.0 ** 58)
    for c, s in enumerate(sizes):
        rows = np.flatnonzero(cid == c)
        col = np.ones(s, dtype=np.float32)
        col[0], col[-1] = BIG, -BIG
        x[rows, 1] = col
        x[rows, 2] = rs.choice(np.array([BIG, -BIG, 1.0, 3.0], dtype=np.float32), s)
        x[rows, 3] = rs.randn(s).astype(np.float32)
    init = np.zeros((len(sizes), 4), dtype=np.float32)
    init[:, 0] = np.arange(len(sizes), dtype=np.float32) * np.float32(2.0 ** 58)
    return np.ascontiguousarray(x), init
