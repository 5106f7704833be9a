"""Range search on resident corpus handles (pmm_range_f32_corpus,
``DeviceCorpus.range``, ``polars_matmul.within``): every corpus row whose score
passes a threshold, per query row, as CSR lists, best first.

The truth everywhere is the oracle's ranked list: ``oracle.topk`` with k = n on
the same f32 inputs, each row cut where the comparison with the threshold first
fails.  Offsets, indices and score bits must be equal; there are no tolerances
in this file.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import oracle
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def ranked(q, c, metric):
    """The oracle's full ranked lists: (indices, f32 scores), n per row."""
    oi, osc = oracle.topk(q, c, c.shape[0], ORACLE_METRIC[metric])
    return np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(np.float32)


def cut(full, threshold, metric):
    """CSR (offsets, idx, scores) of the ranked lists cut where the comparison
    first fails (IEEE: a NaN score fails, the two zeros are equal)."""
    oi, osc = full
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        ok = (osc <= t) if metric == EUC else (osc >= t)
    counts = np.where(ok.all(axis=1), ok.shape[1], np.argmin(ok, axis=1)).astype(np.int64)
    offsets = np.zeros(oi.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    keep = np.arange(oi.shape[1])[None, :] < counts[:, None]
    return offsets, oi[keep], osc[keep]


def assert_same(got, want, label):
    assert np.array_equal(got[0], want[0]), f"{label}: offsets differ\n{got[0]}\n{want[0]}"
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), f"{label}: indices differ"
    a, b = f32(got[2]), f32(want[2])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{label}: score bits differ"


def crange(dc, q, threshold, metric, cap, idx=None, sc=None):
    """The C entry as it is: (rc, offsets, total)."""
    q = f32(q)
    offsets = np.full(q.shape[0] + 1, -1, dtype=np.int64)
    total = ctypes.c_int64(-1)
    rc = _native.lib().pmm_range_f32_corpus(dc._h, _native.ptr(q), q.shape[0], threshold, metric, cap,
                                            _native.ptr(offsets), None if idx is None else _native.ptr(idx),
                                            None if sc is None else _native.ptr(sc), ctypes.byref(total))
    return rc, offsets, total.value


def median_threshold(full):
    s = full[1][np.isfinite(full[1])]
    return float(np.median(s))


# ---- 1. ragged in every dimension, about half of the elements hit ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_ragged_shape_at_the_median(metric):
    m, n, d = 33, 300, 37
    rs = np.random.RandomState(21 + metric)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    full = ranked(q, c, metric)
    t = median_threshold(full)
    want = cut(full, t, metric)
    counts = np.diff(want[0])
    assert 0.3 * m * n < want[0][-1] < 0.7 * m * n
    # rows in the workgroup tier (the wave tier's short rows: tests 2 and 3)
    assert (counts > 128).any() and counts.max() <= 8192, counts
    dc = _native.DeviceCorpus(c)
    try:
        assert_same(dc.range(q, t, metric), want, NAME[metric])
    finally:
        dc.close()


# ---- 2. across a query block and a corpus tile of every instantiated variant ----
@pytest.fixture(scope="module")
def tile_case():
    m, n, d = 257, 513, 64
    rs = np.random.RandomState(5)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    return q, c, {metric: ranked(q, c, metric) for metric in (COS, DOT, EUC)}


@pytest.mark.parametrize("variant", [0, 3])
def test_tile_boundaries_under_every_variant(tile_case, variant, monkeypatch):
    q, c, fulls = tile_case
    monkeypatch.setenv("PMM_GEMM_VARIANT", str(variant))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in (COS, DOT, EUC):
            full = fulls[metric]
            # about 5% of the elements: the last query row (block 2 of 128- and
            # 256-row blocks) and the last corpus row (tile 3 of 256) included
            s = np.sort(full[1][np.isfinite(full[1])])
            t = float(s[int(0.05 * s.size)] if metric == EUC else s[int(0.95 * s.size)])
            want = cut(full, t, metric)
            assert want[0][-1] > 0 and (np.diff(want[0])[-1] > 0) and (want[1] == 512).any()
            assert_same(dc.range(q, t, metric), want, f"variant {variant} {NAME[metric]}")
    finally:
        dc.close()


# ---- 3. the threshold is an entry's exact score: included, the next one not ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_boundary_inclusion(metric):
    m, n, d, r = 5, 300, 37, 6
    rs = np.random.RandomState(31 + metric)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    full = ranked(q, c, metric)
    assert full[1][0, r] != full[1][0, r + 1]
    t = float(full[1][0, r])
    want = cut(full, t, metric)
    assert want[0][1] == r + 1
    dc = _native.DeviceCorpus(c)
    try:
        got = dc.range(q, t, metric)
        assert_same(got, want, NAME[metric])
        assert got[0][1] == r + 1 and got[1][r] == full[0][0, r]
        assert np.float32(got[2][r]).view(np.uint32) == np.float32(t).view(np.uint32)
    finally:
        dc.close()


# ---- 4. ties: duplicated corpus rows leave lower index first ----
def test_ties_lower_index_first():
    n, d = 300, 37
    rs = np.random.RandomState(4)
    c = f32(rs.randn(n, d))
    c[250] = c[130] = c[7]
    q = f32(np.vstack([c[7:8], rs.randn(2, d)]))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in (COS, DOT, EUC):
            full = ranked(q, c, metric)
            t = float(full[1][0, 9])
            got = dc.range(q, t, metric)
            assert got[1][:3].tolist() == [7, 130, 250], (NAME[metric], got[1][:5])
            assert_same(got, cut(full, t, metric), NAME[metric])
    finally:
        dc.close()


# ---- 5. the zero-norm / NaN fixture of the parity tests ----
@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_edge_fixture(metric, poison):
    z = np.load(os.path.join(GOLD, "edge_f32_6x70x37.npz"))
    q, c = f32(z["q"]), f32(z["c"]).copy()
    if poison:
        # the fixture's zero-norm rows, and NaN scores: a NaN element, and an
        # infinite one (inf - inf in the chain, an infinite norm)
        c[11, 3] = np.nan
        c[12, 0] = np.inf
        c[13, 1] = -np.inf
    full = ranked(q, c, metric)
    if poison and metric != EUC:  # (a NaN squared distance is a distance of 0: the reference's max rule)
        assert np.isnan(full[1]).any()
    finite_or_inf = ~np.isnan(full[1])
    dc = _native.DeviceCorpus(c)
    try:
        res = {}
        for t in (0.0, -0.0, -INF, INF, 1.0, -1.0):
            res[t if t != 0.0 else ("-0" if np.signbit(t) else "+0")] = got = dc.range(q, t, metric)
            assert_same(got, cut(full, t, metric), f"{NAME[metric]} threshold {t}")
            assert not np.isnan(got[2]).any()  # a NaN score never hits
        assert_same(res["+0"], res["-0"], "the two zeros")
        every = res[INF] if metric == EUC else res[-INF]
        assert np.array_equal(np.diff(every[0]), finite_or_inf.sum(axis=1))
        if metric != EUC:
            assert res[INF][0][-1] == np.isposinf(full[1]).sum()  # (+inf scores, if any, equal the threshold)
        if metric == COS:
            # zero-norm rows score 0 and hit a threshold of 0
            zc = np.flatnonzero(np.linalg.norm(c.astype(np.float64), axis=1) == 0)
            zq = np.flatnonzero(np.linalg.norm(q.astype(np.float64), axis=1) == 0)
            assert zc.size and zq.size
            o, gi, gs = res["+0"]
            for i in zq:  # a zero-norm query: every column scores 0, all hit, ascending index
                assert gi[o[i]:o[i + 1]].tolist() == list(range(c.shape[0]))
                assert not gs[o[i]:o[i + 1]].any()
            for i in range(q.shape[0]):
                if not np.isnan(q[i]).any():
                    assert set(zc) <= set(gi[o[i]:o[i + 1]].tolist()), i
    finally:
        dc.close()


# ---- 6. no hits, capacity, count-only ----
def test_no_hits_and_capacity():
    m, n, d = 33, 300, 37
    rs = np.random.RandomState(6)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    full = ranked(q, c, COS)
    dc = _native.DeviceCorpus(c)
    try:
        idx, sc = np.full(64, 0xDEADBEEF, np.uint32), np.full(64, 1234.5, np.float32)
        rc, offsets, total = crange(dc, q, 2.0, COS, 64, idx, sc)  # no cosine reaches 2
        assert rc == _native.PMM_OK and total == 0 and not offsets.any()
        assert (idx == 0xDEADBEEF).all() and (sc == 1234.5).all()

        t = median_threshold(full)
        want = cut(full, t, COS)
        tot = int(want[0][-1])
        idx, sc = np.full(tot, 0xDEADBEEF, np.uint32), np.full(tot, 1234.5, np.float32)
        rc, offsets, total = crange(dc, q, t, COS, tot - 1, idx, sc)
        assert rc == _native.PMM_OK and total == tot and np.array_equal(offsets, want[0])
        assert (idx == 0xDEADBEEF).all() and (sc == 1234.5).all()  # too small: nothing written
        rc, offsets, total = crange(dc, q, t, COS, 0)  # count-only, null buffers
        assert rc == _native.PMM_OK and total == tot and np.array_equal(offsets, want[0])
        rc, offsets, total = crange(dc, q, t, COS, tot, idx, sc)
        assert rc == _native.PMM_OK and total == tot
        assert_same((offsets, idx, sc), want, "cap = total")
        # the Python entry: a forced tiny first capacity and a large one agree
        assert_same(dc.range(q, t, COS, cap=1), want, "cap=1")
        assert_same(dc.range(q, t, COS, cap=m * n), want, "cap=m*n")
        rc, offsets, total = crange(dc, q[:0], t, COS, 0)  # m = 0
        assert rc == _native.PMM_OK and total == 0 and offsets[0] == 0
    finally:
        dc.close()


# ---- 7. the three sort tiers ----
@pytest.mark.parametrize("n,sort_max", [(2000, None), (2000, 1024), (8192, None), (8193, None)])
def test_long_segments_workgroup_sort_and_anyk_route(n, sort_max, monkeypatch):
    # segments of 2000 keys: the workgroup's LDS sort, or with
    # PMM_RANGE_SORT_MAX=1024 the handle's ordinary top-k with k = 2000; 8192
    # keys: the largest segment the LDS sort takes (64 KiB), 8193: the first
    # that goes to the top-k route without the knob
    # (the wave tier: test_tile_boundaries_under_every_variant, test_boundary_inclusion)
    m, d = 3, 8
    rs = np.random.RandomState(7)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    if sort_max is not None:
        monkeypatch.setenv("PMM_RANGE_SORT_MAX", str(sort_max))
    want = cut(ranked(q, c, DOT), -INF, DOT)
    assert np.diff(want[0]).tolist() == [n] * m
    dc = _native.DeviceCorpus(c)
    try:
        assert_same(dc.range(q, -INF, DOT), want, f"sort_max {sort_max}")
    finally:
        dc.close()


# ---- 8. derived handles return the parent's numbers ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_subset_handle_equals_the_parent_result_filtered(metric):
    m, n, d = 33, 300, 37
    rs = np.random.RandomState(81 + metric)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    c[200] = c[100] = c[3]  # a tie across the selection
    mask = rs.rand(n) < 0.5
    mask[[0, n - 1, 100, 200]] = True
    mask[3] = False
    ids = np.flatnonzero(mask).astype(np.uint32)
    full = ranked(q, c, metric)
    t = median_threshold(full)
    dc = _native.DeviceCorpus(c)
    try:
        po, pi, ps = dc.range(q, t, metric)
        assert_same((po, pi, ps), cut(full, t, metric), "parent")
        keep = mask[pi]
        rows = np.repeat(np.arange(m), np.diff(po))
        fo = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=m), out=fo[1:])
        want = (fo, pi[keep], ps[keep])
        for how, sel in (("mask", mask), ("ids", ids)):
            sub = dc.subset(sel)
            try:
                assert_same(sub.range(q, t, metric), want, f"{NAME[metric]} by {how}")
            finally:
                sub.close()
    finally:
        dc.close()


# ---- 9. refusals ----
def test_refused_handles():
    n, d = 300, 37
    rs = np.random.RandomState(9)
    c, q = f32(rs.randn(n, d)), f32(rs.randn(4, d))
    dc = _native.DeviceCorpus(c)
    part = dc.partition(np.arange(n, dtype=np.uint32) % 3, 3)
    d64 = _native.DeviceCorpus(c.astype(np.float64))
    b16 = _native.DeviceCorpus(c, compute="bf16")
    try:
        for h, word in ((part, "partitioned"), (d64, "f32 handle"), (b16, "f32 handle")):
            rc, _, _ = crange(h, q, 0.5, COS, 0)
            assert rc == _native.PMM_ERR_ARG and word in _native.last_error(), _native.last_error()
        with pytest.raises(_native.PmmError) as ei:
            part.range(q, 0.5, COS)
        assert ei.value.code == _native.PMM_ERR_ARG
    finally:
        for h in (part, d64, b16, dc):
            h.close()
    _native.set_devices([0, 0])
    try:
        sharded = _native.DeviceCorpus(c)
        try:
            assert sharded.shards == 2
            rc, _, _ = crange(sharded, q, 0.5, COS, 0)
            assert rc == _native.PMM_ERR_UNSUPPORTED and _native.last_error()
        finally:
            sharded.close()
    finally:
        _native.set_devices([])


# ---- 10. the numpy path, through the corpus cache ----
def test_numpy_within_equals_range_and_caches_the_corpus(monkeypatch):
    import polars_matmul

    m, n, d = 9, 4200, 64  # (n * d * 4 >= 1 MiB: cacheable)
    rs = np.random.RandomState(10)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    created = []

    class Counting(_native.DeviceCorpus):
        def __init__(self, *a, **k):
            created.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(_native, "DeviceCorpus", Counting)
    pm.clear_corpus_cache()
    try:
        t = 0.3
        o1, i1, s1 = polars_matmul.within(q, c, t, "cosine")
        o2, i2, s2 = polars_matmul.within(q, c, t, "cosine")
        assert len(created) == 1, "the second call made a second handle"
        assert s1.dtype == np.float64
        assert_same((o2, i2, s2), (o1, i1, s1), "second call")
        assert_same((o1, i1, s1), cut(ranked(q, c, COS), t, COS), "oracle")
        dc = _native.DeviceCorpus(c)
        try:
            assert_same((o1, i1, s1), dc.range(q, t, COS), "DeviceCorpus.range")
        finally:
            dc.close()
        mask = rs.rand(n) < 0.5
        so, si, ss = polars_matmul.within(q, c, t, "cosine", subset=mask)
        keep = mask[i1]
        assert np.array_equal(si, i1[keep]) and np.array_equal(f32(ss).view(np.uint32), f32(s1[keep]).view(np.uint32))
        # the Arrow entry on the same rows
        import pyarrow as pa

        arr = pm._within(pa.FixedSizeListArray.from_arrays(pa.array(q.reshape(-1)), d),
                         pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1)), d), t, "cosine")
        assert np.array_equal(arr.offsets.to_numpy(), o1)
        assert np.array_equal(arr.values.field("index").to_numpy(), i1)
        assert np.array_equal(arr.values.field("score").to_numpy(), s1)
    finally:
        pm.clear_corpus_cache()
