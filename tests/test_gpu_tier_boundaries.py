"""The shared sort driver at its tier boundaries (DESIGN.md §4d "Piece planner
and sort driver"): rows of exactly 0, 1, 2, 127, 128, 129, smax - 1, smax,
smax + 1, 2 smax, 2 smax + 1 and 3 smax keys under a lowered
PMM_RANGE_SORT_MAX, through the candidate search and the range search, on a
clean and on a poisoned arena.  Bit-equal to the oracle; no tolerances."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from polars_matmul import _native
from test_gpu_candidates import assert_same as assert_same_lists, f32, truth
from test_gpu_range import assert_same as assert_same_csr, cut, ranked

pytestmark = pytest.mark.gpu

DOT = _native.METRIC_DOT


def lengths(smax):
    return [0, 1, 2, 127, 128, 129, smax - 1, smax, smax + 1, 2 * smax, 2 * smax + 1, 3 * smax]


@functools.lru_cache(maxsize=None)
def candidate_case(smax, k):
    L, n, d = lengths(smax), 3 * smax, 33
    rs = np.random.RandomState(smax + k)
    q, c = f32(rs.randn(len(L), d)), f32(rs.randn(n, d))
    offsets = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    ids = np.concatenate([np.sort(rs.choice(n, size=x, replace=False)) for x in L]).astype(np.uint32)
    return q, c, offsets, ids, truth(q, c, offsets, ids, k, DOT)


@functools.lru_cache(maxsize=None)
def range_case(smax):
    """Query i = e_i; corpus row j has component i = 1 + j / 4096 for j < L_i,
    else 0: at threshold 0.5 row i hits exactly rows 0 .. L_i - 1, with
    distinct scores (exact in f32)."""
    L = np.array(lengths(smax))
    m, n = L.size, 3 * smax
    j = np.arange(n)
    q = f32(np.eye(m))
    c = f32(np.where(j[:, None] < L[None, :], 1.0 + j[:, None] / 4096.0, 0.0))
    want = cut(ranked(q, c, DOT), 0.5, DOT)
    return q, c, want


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("wide", [False, True])  # k = 10, or 2 smax + 1
@pytest.mark.parametrize("smax", [128, 256])
def test_candidates_at_the_tier_boundaries(smax, wide, poison, monkeypatch):
    k = 2 * smax + 1 if wide else 10
    q, c, offsets, ids, want = candidate_case(smax, k)
    assert np.diff(offsets).tolist() == lengths(smax)
    monkeypatch.setenv("PMM_RANGE_SORT_MAX", str(smax))
    if poison:
        monkeypatch.setenv("PMM_ARENA_POISON", "0xFF")
    dc = _native.DeviceCorpus(c)
    try:
        assert_same_lists(dc.topk_candidates(q, offsets, ids, k, DOT), want, f"smax {smax} k {k} poison {poison}")
    finally:
        dc.close()


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("smax", [128, 256])
def test_range_at_the_tier_boundaries(smax, poison, monkeypatch):
    q, c, want = range_case(smax)
    assert np.diff(want[0]).tolist() == lengths(smax)  # (the construction, on the oracle)
    assert all(np.unique(want[2][a:b]).size == b - a for a, b in zip(want[0][:-1], want[0][1:]))
    monkeypatch.setenv("PMM_RANGE_SORT_MAX", str(smax))
    if poison:
        monkeypatch.setenv("PMM_ARENA_POISON", "0xFF")
    dc = _native.DeviceCorpus(c)
    try:
        assert_same_csr(dc.range(q, 0.5, DOT), want, f"smax {smax} poison {poison}")
    finally:
        dc.close()
