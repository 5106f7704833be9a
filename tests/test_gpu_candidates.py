"""Candidate search on resident corpus handles (pmm_topk_f32_candidates,
``DeviceCorpus.topk_candidates``, ``candidates=`` on ``_topk`` / ``topk``):
exact top-k of every query row over its own list of corpus rows.

The truth for a row is the oracle on that row and its candidate rows alone --
``oracle.topk(q[i:i+1], c[S_i], min(k, |S_i|), metric)`` with its indices mapped
through the ascending S_i.  Indices, score bits, lengths and padding must be
equal; there are no tolerances in this file.
"""
from __future__ import annotations

import functools

import numpy as np
import pyarrow as pa
import pytest

import oracle
import polars_matmul
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm
from value_cases import SIGNED_ZERO_ROWS, value_case

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
M, N = 37, 1237
EMPTY = 0xFFFFFFFF


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def truth(q, c, offsets, ids, k, metric):
    """(idx [m, k], scores f32 [m, k], lens [m]) by the per-row oracle, padded
    as the entry pads (index 0xFFFFFFFF, score +0.0)."""
    m = q.shape[0]
    idx = np.full((m, k), EMPTY, dtype=np.uint32)
    sc = np.zeros((m, k), dtype=np.float32)
    lens = np.zeros(m, dtype=np.uint32)
    for i in range(m):
        S = ids[offsets[i]:offsets[i + 1]]
        kk = min(k, S.size)
        lens[i] = kk
        if kk:
            oi, osc = oracle.topk(q[i:i + 1], np.ascontiguousarray(c[S]), kk, ORACLE_METRIC[metric])
            idx[i, :kk] = S[np.asarray(oi)[0]]
            sc[i, :kk] = np.asarray(osc)[0].astype(np.float32)
    return idx, sc, lens


def assert_same(got, want, label):
    gi, gs, gl = got
    wi, ws, wl = want
    assert gl.dtype == np.uint32 and np.array_equal(gl, wl), f"{label}: lengths differ\n{gl}\n{wl}"
    assert gi.dtype == np.uint32 and gi.shape == wi.shape
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, f"{label}: indices differ in rows {bad[:8]}: {gi[bad[0]][:12]} vs {wi[bad[0]][:12]}"
    a, b = f32(gs).view(np.uint32), f32(ws).view(np.uint32)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"{label}: score bits differ in rows {bad[:8]}"


def lists(counts, n, seed):
    """CSR lists with the given lengths: random strictly ascending row ids."""
    rs = np.random.RandomState(seed)
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    ids = np.concatenate([np.sort(rs.choice(n, size=int(cn), replace=False)) for cn in counts] or [[]])
    return offsets, np.ascontiguousarray(ids, dtype=np.uint32)


def csr(rows):
    """CSR (offsets, ids) of explicit ascending lists."""
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return offsets, np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]), dtype=np.uint32)


def boundary_counts(k, n=N, m=M):
    """Every lane, wave, unit and sort-tier boundary, and the cut at k."""
    base = [0, 1, k - 1, k, k + 1, 63, 64, 65, 128, 129, 255, 256, 257, 300, n]
    base = [min(max(x, 0), n) for x in base]
    return [base[i % len(base)] for i in range(m)]


@functools.lru_cache(maxsize=None)
def data(d):
    rs = np.random.RandomState(100 + d)
    return f32(rs.randn(M, d)), f32(rs.randn(N, d))


@pytest.fixture(scope="module")
def corpora():
    made = {}

    def get(d):
        if d not in made:
            made[d] = _native.DeviceCorpus(data(d)[1])
        return made[d]

    yield get
    for dc in made.values():
        dc.close()


@functools.lru_cache(maxsize=None)
def case(d, metric, k):
    q, c = data(d)
    offsets, ids = lists(boundary_counts(k), N, 7 * d + k)
    return offsets, ids, truth(q, c, offsets, ids, k, metric)


# ---- 1. every boundary, every metric, every chunk count ----
@pytest.mark.parametrize("k", [1, 10, 100, 1500])
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
@pytest.mark.parametrize("d", [1, 20, 33, 256, 800])
def test_lists_equal_the_per_row_oracle(corpora, d, metric, k):
    offsets, ids, want = case(d, metric, k)
    got = corpora(d).topk_candidates(data(d)[0], offsets, ids, k, metric)
    assert_same(got, want, f"d={d} {NAME[metric]} k={k}")
    unused = np.arange(k)[None, :] >= want[2][:, None].astype(np.int64)
    assert (got[0][unused] == EMPTY).all() and (f32(got[1]).view(np.uint32)[unused] == 0).all()


# ---- 2. value edges ----
def test_duplicate_rows_tie_to_the_lower_index(corpora):
    q, c = data(33)
    c = c.copy()
    c[900] = c[500] = c[10]
    c[1236] = c[3]
    rs = np.random.RandomState(3)
    offsets, ids = csr([np.arange(N), np.union1d(rs.choice(N, 297, replace=False), [10, 500, 900]),
                        np.union1d(rs.choice(N, 60, replace=False), [3, 10, 900, 1236]), [500]])
    dc = _native.DeviceCorpus(c)
    try:
        for metric in (COS, DOT, EUC):
            for k in (3, 400):
                want = truth(q[:4], c, offsets, ids, k, metric)
                assert_same(dc.topk_candidates(q[:4], offsets, ids, k, metric), want, f"ties {NAME[metric]} k={k}")
                if k == 400:  # (row 1's whole list: the three equal rows are adjacent, lower index first)
                    row = want[0][1, :want[2][1]].tolist()
                    assert row.index(10) + 2 == row.index(500) + 1 == row.index(900)
    finally:
        dc.close()


def test_zero_rows_under_cosine(corpora):
    q, c = data(20)
    q, c = q.copy(), c.copy()
    q[1] = 0.0
    c[[0, 77, 600]] = 0.0
    offsets, ids = lists([N, N, 129, 65], N, 5)
    dc = _native.DeviceCorpus(c)
    try:
        for k in (5, N):
            want = truth(q[:4], c, offsets, ids, k, COS)
            assert_same(dc.topk_candidates(q[:4], offsets, ids, k, COS), want, f"zero rows k={k}")
    finally:
        dc.close()


@pytest.mark.parametrize("metric", [COS, DOT])
def test_planted_negative_zero_keeps_its_sign(metric):
    q, c = value_case("signed_zero", np.float32, 5, 320, 24)
    rows = np.array(sorted(SIGNED_ZERO_ROWS), dtype=np.uint32)
    offsets = np.arange(6, dtype=np.int64) * rows.size
    ids = np.tile(rows, 5)
    dc = _native.DeviceCorpus(c)
    try:
        want = truth(q, c, offsets, ids, rows.size, metric)
        bits = want[1].view(np.uint32)
        assert (bits == 0x80000000).any() and (bits == 0).any()  # both zeros are in the truth
        assert_same(dc.topk_candidates(q, offsets, ids, rows.size, metric), want, f"signed zero {NAME[metric]}")
        every = np.arange(320, dtype=np.uint32)
        off2 = np.arange(6, dtype=np.int64) * 320
        want = truth(q, c, off2, np.tile(every, 5), 320, metric)
        assert_same(dc.topk_candidates(q, off2, np.tile(every, 5), 320, metric), want, "signed zero, every row")
    finally:
        dc.close()


@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_nan_row_inside_and_outside_k(metric):
    q, c = data(33)
    c = c.copy()
    c[40, 2] = np.nan
    c[41] = np.nan
    rs = np.random.RandomState(9)
    pool = np.setdiff1d(np.arange(N), [40, 41])
    offsets, ids = csr([np.union1d(rs.choice(pool, cnt - 2, replace=False), [40, 41]) for cnt in (70, 70, 300)])
    dc = _native.DeviceCorpus(c)
    try:
        for k in (10, 69, 70, 300):  # outside k; one NaN inside; both inside
            want = truth(q[:3], c, offsets, ids, k, metric)
            got = dc.topk_candidates(q[:3], offsets, ids, k, metric)
            assert_same(got, want, f"NaN {NAME[metric]} k={k}")
        if metric == DOT:  # (the reference's cosine scores a NaN norm 0, its euclidean a NaN square 0)
            assert np.isnan(got[1][0, 69]) and got[0][0, 68:70].tolist() == [40, 41]
    finally:
        dc.close()


# ---- 3. against the whole-corpus search ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_every_row_equals_the_corpus_topk(corpora, metric):
    d = 256
    q, _ = data(d)
    every = np.arange(N, dtype=np.uint32)
    offsets = np.arange(M + 1, dtype=np.int64) * N
    for k in (10, N):
        gi, gs, gl = corpora(d).topk_candidates(q, offsets, np.tile(every, M), k, metric)
        ti, ts = corpora(d).topk(q, k, metric)
        assert (gl == k).all() and np.array_equal(gi, ti)
        assert np.array_equal(gs.view(np.uint32), ts.view(np.uint32))


# ---- 4. the long-row path and poisoned scratch: the same bits ----
@pytest.mark.parametrize("metric", [COS, EUC])
@pytest.mark.parametrize("k", [10, 100, 1500])
def test_lowered_sort_max_takes_the_long_row_path(corpora, monkeypatch, metric, k):
    d = 33
    offsets, ids, want = case(d, metric, k)
    assert (np.diff(offsets) > 256).sum() >= 3  # the 257-, 300- and n-candidate rows
    monkeypatch.setenv("PMM_RANGE_SORT_MAX", "256")
    assert_same(corpora(d).topk_candidates(data(d)[0], offsets, ids, k, metric), want, f"sort max 256, k={k}")


@pytest.mark.parametrize("poison", ["0xFF", "0x7F", "0x01"])
def test_poisoned_arena_gives_the_same_bits(corpora, monkeypatch, poison):
    d = 33
    for metric, k, smax in ((COS, 100, None), (DOT, 10, None), (EUC, 1500, "256")):
        offsets, ids, want = case(d, metric, k)
        clean = corpora(d).topk_candidates(data(d)[0], offsets, ids, k, metric)
        monkeypatch.setenv("PMM_ARENA_POISON", poison)
        if smax:
            monkeypatch.setenv("PMM_RANGE_SORT_MAX", smax)
        got = corpora(d).topk_candidates(data(d)[0], offsets, ids, k, metric)
        monkeypatch.delenv("PMM_ARENA_POISON")
        monkeypatch.delenv("PMM_RANGE_SORT_MAX", raising=False)
        assert_same(got, clean, f"poison {poison} {NAME[metric]}")
        assert_same(got, want, f"poison {poison} {NAME[metric]} vs the oracle")


# ---- 5. refusals ----
def raw(dc, q, offsets, ids, k, metric):
    q = f32(q)
    m = q.shape[0]
    offsets = np.ascontiguousarray(offsets, np.int64)
    ids = np.ascontiguousarray(ids, np.uint32)
    oi = np.zeros((m, k), np.uint32)
    os_ = np.zeros((m, k), np.float32)
    ol = np.zeros(m, np.uint32)
    rc = _native.lib().pmm_topk_f32_candidates(dc._h, _native.ptr(q), m, _native.ptr(offsets), _native.ptr(ids), k,
                                               metric, _native.ptr(oi), _native.ptr(os_), _native.ptr(ol))
    return rc, _native.last_error()


def test_bad_lists_are_reported_and_the_handle_serves_on(corpora):
    d = 20
    q, c = data(d)
    dc = corpora(d)
    offsets = np.array([0, 3, 5], dtype=np.int64)
    for ids, text in (([5, 9, 7, 1, 2], "strictly ascending"), ([5, 9, 9, 1, 2], "strictly ascending"),
                      ([5, 9, 10, 1, N], "not a row of the corpus"), ([5, 9, 10, 1, 0xFFFFFFFF], "not a row")):
        rc, msg = raw(dc, q[:2], offsets, ids, 2, COS)
        assert rc == _native.PMM_ERR_ARG and text in msg, (ids, rc, msg)
        # the process and the handle serve a correct call afterwards
        good_off, good_ids = lists([3, 2], N, 1)
        assert_same(dc.topk_candidates(q[:2], good_off, good_ids, 2, COS), truth(q[:2], c, good_off, good_ids, 2, COS),
                    "after a refusal")
    # host-side refusals: before any device call
    for off, text in (([1, 3, 5], "start at 0"), ([0, 4, 3], "descend")):
        rc, msg = raw(dc, q[:2], off, [1, 2, 3, 4, 5], 2, COS)
        assert rc == _native.PMM_ERR_ARG and text in msg, msg
    rc, msg = raw(dc, q[:2], offsets, [1, 2, 3, 4, 5], 2, 7)
    assert rc == _native.PMM_ERR_ARG
    with pytest.raises(_native.PmmError) as ei:
        dc.topk_candidates(q[:2], offsets, [1, 2, 3, 4, 5], 0, COS)
    assert ei.value.code == _native.PMM_ERR_ARG and "k must be >= 1" in str(ei.value)
    L = _native.lib()
    assert L.pmm_topk_f32_candidates(dc._h, None, 0, None, None, 1, COS, None, None, None) == _native.PMM_OK
    assert L.pmm_topk_f32_candidates(dc._h, None, 2, None, None, 1, COS, None, None, None) == _native.PMM_ERR_ARG
    assert L.pmm_topk_f32_candidates(dc._h, None, -1, None, None, 1, COS, None, None, None) == _native.PMM_ERR_ARG


def test_other_handles_are_refused():
    q, c = data(20)
    offsets, ids = lists([3, 2], 100, 1)
    made = []
    try:
        f = _native.DeviceCorpus(c)
        made.append(f)
        labels = (np.arange(N) % 3).astype(np.uint32)
        others = [("f64", _native.DeviceCorpus(c.astype(np.float64))), ("bf16", _native.DeviceCorpus(c, compute="bf16")),
                  ("int8", _native.DeviceCorpus.int8((c * 10).astype(np.int8))),
                  ("derived", f.subset(np.arange(0, N, 2, dtype=np.uint32))), ("partitioned", f.partition(labels, 3))]
        made += [dc for _, dc in others]
        for what, dc in others:
            rc, msg = raw(dc, q[:2], offsets, ids, 2, COS)
            assert rc == _native.PMM_ERR_ARG and what in msg, (what, rc, msg)
        assert raw(f, q[:2], offsets, ids, 2, COS)[0] == _native.PMM_OK
    finally:
        for dc in made:
            dc.close()


# ---- 6. the Python surface ----
def ragged(want):
    idx, sc, lens = want
    return [[(int(idx[i, j]), float(sc[i, j])) for j in range(int(lens[i]))] for i in range(idx.shape[0])]


def as_pairs(out):
    return [[(e["index"], e["score"]) for e in row] for row in out.to_pylist()]


def same_ragged(out, want):
    got, exp = as_pairs(out), ragged(want)
    assert [[p[0] for p in r] for r in got] == [[p[0] for p in r] for r in exp]
    a = np.array([p[1] for r in got for p in r], dtype=np.float64)
    b = np.array([p[1] for r in exp for p in r], dtype=np.float64)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("metric", [COS, EUC])
def test_topk_keyword_through_the_cache_and_the_fallback(monkeypatch, metric):
    d, k = 256, 100
    q, c = data(d)
    offsets, ids, want = case(d, metric, k)
    # the caller's lists: unsorted, with duplicates, one null
    rs = np.random.RandomState(2)
    rows = []
    for i in range(M):
        S = ids[offsets[i]:offsets[i + 1]].astype(np.int64)
        rows.append(None if S.size == 0 and i % 2 else rs.permutation(np.concatenate([S, S[:3]])).tolist())
    cand = pa.array(rows, type=pa.large_list(pa.int64()))
    corpus = pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1)), d)  # 1.2 MiB: cacheable
    queries = pa.FixedSizeListArray.from_arrays(pa.array(q.reshape(-1)), d)
    pm.clear_corpus_cache()
    try:
        monkeypatch.setattr(pm, "_CACHE_ON", True)
        same_ragged(pm._topk(queries, corpus, k, NAME[metric], candidates=cand), want)
        assert len(pm._cache) == 1  # searched on the cached handle
        pm.clear_corpus_cache()
        monkeypatch.setattr(pm, "_CACHE_ON", False)  # the forced fallback: the union's rows, renumbered lists
        same_ragged(pm._topk(queries, corpus, k, NAME[metric], candidates=cand), want)
        same_ragged(pm._topk(queries, corpus, k, NAME[metric], candidates=(offsets, ids)), want)
        assert len(pm._cache) == 0
        # k clips to the longest list; the numpy level pads with 0xFFFFFFFF / NaN
        gi, gs = polars_matmul.topk(q, c, 5000, NAME[metric], candidates=(offsets, ids))
        full = truth(q, c, offsets, ids, N, metric)
        assert gi.shape == (M, N) and np.array_equal(gi, full[0])
        unused = np.arange(N)[None, :] >= full[2][:, None].astype(np.int64)
        assert np.isnan(gs[unused]).all()
        assert np.array_equal(gs[~unused].view(np.uint64), full[1].astype(np.float64)[~unused].view(np.uint64))
    finally:
        pm.clear_corpus_cache()
