"""Shared by the self-search tests (tests/test_gpu_self.py, tests/test_self_cpu.py):
the data of the ragged case and the truth -- the oracle's ranked list of the
column against itself, cut at the threshold, with the entries at positions
j <= i removed (range) or j = i removed (top-k).  CPU only."""
from __future__ import annotations

import numpy as np

import oracle
from polars_matmul import _native

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def ragged_column(metric):
    """Case 1: n = 300, d = 37."""
    return f32(np.random.RandomState(61 + metric).randn(300, 37))


def ranked_self(c, metric):
    """The oracle's full ranked lists of c against itself: (indices, f32 scores), n per row."""
    oi, osc = oracle.topk(c, c, c.shape[0], ORACLE_METRIC[metric])
    return np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(np.float32)


def hit_mask(full, threshold, metric):
    """Which entries of the ranked lists pass the threshold (IEEE: a NaN score fails)."""
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        return (full[1] <= t) if metric == EUC else (full[1] >= t)


def csr(full, keep):
    counts = keep.sum(axis=1).astype(np.int64)
    offsets = np.zeros(full[0].shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, full[0][keep], full[1][keep]


def range_self_truth(full, threshold, metric):
    """CSR (offsets, idx, scores): row i's hits, best first, without the entries j <= i."""
    above = full[0].astype(np.int64) > np.arange(full[0].shape[0])[:, None]
    return csr(full, hit_mask(full, threshold, metric) & above)


def topk_self_truth(full, k):
    """(idx, scores) [n][k]: row i's ranked list without row i, cut at k."""
    n = full[0].shape[0]
    other = full[0].astype(np.int64) != np.arange(n)[:, None]
    assert (other.sum(axis=1) == n - 1).all()
    return full[0][other].reshape(n, n - 1)[:, :k], full[1][other].reshape(n, n - 1)[:, :k]


def median_threshold(full):
    return float(np.median(full[1][np.isfinite(full[1])]))


def assert_same_csr(got, want, label):
    assert np.array_equal(got[0], want[0]), f"{label}: offsets differ\n{got[0]}\n{want[0]}"
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), f"{label}: indices differ"
    assert np.array_equal(f32(got[2]).view(np.uint32), f32(want[2]).view(np.uint32)), f"{label}: score bits differ"


def assert_same_lists(got, want, label):
    assert got[0].shape == want[0].shape, f"{label}: shape {got[0].shape}, wanted {want[0].shape}"
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]), f"{label}: indices differ"
    # (a NaN score equals a NaN score, as in tests/test_gpu_parity.py: no entry
    # pins a NaN's payload; a range list never holds one)
    a, b = f32(got[1]), f32(want[1])
    assert ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all(), f"{label}: score bits differ"
