"""Self search on resident corpus handles (pmm_range_f32_self, pmm_topk_f32_self,
``DeviceCorpus.range_self`` / ``.topk_self``, ``within_self`` / ``topk_self``):
one column against itself, each pair once and no row with itself.

The truth everywhere is the oracle's ranked list of the column against itself
(``oracle.topk(c, c, n)``), cut at the threshold, with the entries at positions
j <= i removed for the range entry and j = i removed for top-k
(tests/self_cases.py).  Offsets, indices and score bits must be equal; there are
no tolerances in this file.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from polars_matmul import _native
from polars_matmul import _polars_matmul as pm
from self_cases import (COS, DOT, EUC, NAME, assert_same_csr, assert_same_lists, f32, hit_mask, median_threshold,
                        ragged_column, range_self_truth, ranked_self, topk_self_truth)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
METRICS = [COS, DOT, EUC]


def everything(metric):
    """The threshold every finite score passes."""
    return INF if metric == EUC else -INF


def crange_self(dc, threshold, metric, cap, idx=None, sc=None):
    """The C entry as it is: (rc, offsets, total)."""
    offsets = np.full(dc.n + 1, -1, dtype=np.int64)
    total = ctypes.c_int64(-1)
    rc = _native.lib().pmm_range_f32_self(dc._h, threshold, metric, cap, _native.ptr(offsets),
                                          None if idx is None else _native.ptr(idx),
                                          None if sc is None else _native.ptr(sc), ctypes.byref(total))
    return rc, offsets, total.value


def ctopk_self(dc, k, metric, idx, sc):
    return _native.lib().pmm_topk_f32_self(dc._h, k, metric, None if idx is None else _native.ptr(idx),
                                           None if sc is None else _native.ptr(sc))


@pytest.fixture(scope="module")
def ragged():
    """Case 1 (n = 300, d = 37): per metric the column and its ranked lists."""
    out = {}
    for metric in METRICS:
        c = ragged_column(metric)
        out[metric] = (c, ranked_self(c, metric))
    return out


# ---- 1. ragged in every dimension, about half of the pairs hit ----
@pytest.mark.parametrize("metric", METRICS)
def test_ragged_shape_at_the_median(ragged, metric):
    c, full = ragged[metric]
    t = median_threshold(full)
    want = range_self_truth(full, t, metric)
    counts = np.diff(want[0])
    assert (counts > 128).any() and counts.max() <= 8192, counts  # the workgroup sort tier
    assert counts[-1] == 0  # the last row has no later row
    dc = _native.DeviceCorpus(c)
    try:
        assert_same_csr(dc.range_self(t, metric), want, NAME[metric])
    finally:
        dc.close()


# ---- 2. tiles that straddle the diagonal, under both variants ----
@pytest.fixture(scope="module")
def diagonal_case():
    n, d = 513, 64
    c = f32(np.random.RandomState(5).randn(n, d))
    out = {}
    for metric in METRICS:
        full = ranked_self(c, metric)
        s = np.sort(full[1][np.isfinite(full[1])])
        t = float(s[int(0.05 * s.size)] if metric == EUC else s[int(0.95 * s.size)])
        out[metric] = (full, t, range_self_truth(full, t, metric))
    return c, out


def check_diagonal_case(full, t, want, got, metric, label):
    n = full[0].shape[0]
    rows = np.repeat(np.arange(n), np.diff(want[0]))
    cols = want[1].astype(np.int64)
    same_tile = (rows // 128 == cols // 128) & (rows < cols)
    assert same_tile.any(), "no kept hit inside a diagonal tile"
    # the same tiles hold hits of the full call below the diagonal (and the
    # diagonal itself), which must be absent
    hit = hit_mask(full, t, metric)
    frows = np.repeat(np.arange(n), hit.sum(axis=1))
    fcols = full[0][hit].astype(np.int64)
    below = (frows // 128 == fcols // 128) & (fcols < frows)
    assert (below & np.isin(frows // 128, np.unique(rows[same_tile] // 128))).any()
    assert want[0][-1] == want[0][-2], "row 512 has no later row"
    assert_same_csr(got, want, label)
    grows = np.repeat(np.arange(n), np.diff(got[0]))
    assert (got[1].astype(np.int64) > grows).all()


@pytest.mark.parametrize("variant", [0, 3])
def test_diagonal_tiles_under_every_variant(diagonal_case, variant, monkeypatch):
    c, cases = diagonal_case
    monkeypatch.setenv("PMM_GEMM_VARIANT", str(variant))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            full, t, want = cases[metric]
            check_diagonal_case(full, t, want, dc.range_self(t, metric), metric, f"variant {variant} {NAME[metric]}")
    finally:
        dc.close()


# ---- 3. everything hits ----
@pytest.mark.parametrize("n", [1, 2, 130])
def test_everything_hits(n):
    c = f32(np.random.RandomState(30 + n).randn(n, 8))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            want = range_self_truth(ranked_self(c, metric), everything(metric), metric)
            assert np.diff(want[0]).tolist() == [n - 1 - i for i in range(n)]
            got = dc.range_self(everything(metric), metric)
            assert got[0][-1] == n * (n - 1) // 2
            assert_same_csr(got, want, f"n={n} {NAME[metric]}")
    finally:
        dc.close()


# ---- 4. the zero-norm / tie fixture, with NaN rows, and with duplicated rows ----
def edge_columns():
    c = f32(np.load(os.path.join(GOLD, "edge_f32_6x70x37.npz"))["c"]).copy()
    poisoned = c.copy()
    poisoned[11, 3] = np.nan
    poisoned[12, 0] = np.inf
    poisoned[13, 1] = -np.inf
    dup = poisoned.copy()
    dup[40], dup[41], dup[66] = dup[5], dup[5], dup[20]  # duplicates with a lower row number
    return {"fixture": c, "nan": poisoned, "duplicates": dup}


@pytest.mark.parametrize("which", ["fixture", "nan", "duplicates"])
def test_edge_values(which):
    c = edge_columns()[which]
    n = c.shape[0]
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            full = ranked_self(c, metric)
            if which == "duplicates":
                # row 40's copy at row 5 outranks row 40 itself in the unfiltered list
                r40 = full[0][40].tolist()
                assert r40.index(5) < r40.index(40)
            for t in (0.0, -0.0, -INF, INF, 1.0, -1.0):
                got = dc.range_self(t, metric)
                assert_same_csr(got, range_self_truth(full, t, metric), f"{which} {NAME[metric]} threshold {t}")
                assert not np.isnan(got[2]).any()  # a NaN score never hits
            for k in (1, 10, n - 1):
                assert_same_lists(dc.topk_self(k, metric), topk_self_truth(full, k),
                                  f"{which} {NAME[metric]} k={k}")
    finally:
        dc.close()


# ---- 5. rows past the in-LDS sort: cut into pieces and merged ----
def test_long_rows_piece_and_merge(monkeypatch):
    n, d = 600, 16
    c = f32(np.random.RandomState(7).randn(n, d))
    monkeypatch.setenv("PMM_RANGE_SORT_MAX", "128")
    want = range_self_truth(ranked_self(c, DOT), -INF, DOT)
    counts = np.diff(want[0])
    assert counts.max() == n - 1 and (counts > 128).sum() > 400 and (counts % 128 == 0).any()
    dc = _native.DeviceCorpus(c)
    try:
        assert_same_csr(dc.range_self(-INF, DOT), want, "sort max 128")
    finally:
        dc.close()


# ---- 6. the cap protocol through the C entry ----
def test_cap_protocol(ragged):
    c, full = ragged[COS]
    t = median_threshold(full)
    want = range_self_truth(full, t, COS)
    tot = int(want[0][-1])
    dc = _native.DeviceCorpus(c)
    try:
        rc, offsets, total = crange_self(dc, t, COS, 0)  # count-only, null lists
        assert rc == _native.PMM_OK and total == tot and np.array_equal(offsets, want[0])
        idx, sc = np.full(tot, 0xDEADBEEF, np.uint32), np.full(tot, 1234.5, np.float32)
        rc, offsets, total = crange_self(dc, t, COS, tot - 1, idx, sc)
        assert rc == _native.PMM_OK and total == tot and np.array_equal(offsets, want[0])
        assert (idx == 0xDEADBEEF).all() and (sc == 1234.5).all()  # too small: nothing written
        rc, offsets, total = crange_self(dc, t, COS, tot, idx, sc)
        assert rc == _native.PMM_OK and total == tot
        assert_same_csr((offsets, idx, sc), want, "cap = total")
        rc, offsets, total = crange_self(dc, 2.0, COS, tot, idx, sc)  # no cosine reaches 2
        assert rc == _native.PMM_OK and total == 0 and not offsets.any()
        # the Python entry: a forced tiny first capacity and the largest agree
        assert_same_csr(dc.range_self(t, COS, cap=1), want, "cap=1")
        assert_same_csr(dc.range_self(t, COS, cap=10 ** 9), want, "cap clipped to the pairs")
    finally:
        dc.close()


# ---- 7. derived handles return the parent's numbers ----
@pytest.mark.parametrize("metric", METRICS)
def test_derived_handle(metric):
    n, d = 300, 37
    rs = np.random.RandomState(81 + metric)
    c = f32(rs.randn(n, d))
    c[200] = c[100] = c[3]  # ties across the selection
    mask = rs.rand(n) < 0.5
    mask[[0, n - 1, 100, 200]] = True
    mask[3] = False
    ids = np.flatnonzero(mask).astype(np.uint32)
    full = ranked_self(f32(c[mask]), metric)
    t = median_threshold(full)
    wo, wi, ws = range_self_truth(full, t, metric)
    ti, ts = topk_self_truth(full, 10)
    dc = _native.DeviceCorpus(c)
    try:
        sub = dc.subset(mask)
        try:
            assert_same_csr(sub.range_self(t, metric), (wo, ids[wi], ws), f"range {NAME[metric]}")
            assert_same_lists(sub.topk_self(10, metric), (ids[ti], ts), f"top-k {NAME[metric]}")
        finally:
            sub.close()
    finally:
        dc.close()


# ---- 8. poisoned scratch ----
@pytest.mark.parametrize("poison", ["0x00", "0xFF"])
@pytest.mark.parametrize("variant", [0, 3])
def test_poisoned_scratch(diagonal_case, variant, poison, monkeypatch):
    c, cases = diagonal_case
    monkeypatch.setenv("PMM_GEMM_VARIANT", str(variant))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            _, t, want = cases[metric]
            monkeypatch.delenv("PMM_ARENA_POISON", raising=False)
            plain = dc.range_self(t, metric)
            plain_k = dc.topk_self(100, metric)
            monkeypatch.setenv("PMM_ARENA_POISON", poison)
            assert_same_csr(dc.range_self(t, metric), plain, f"poison {poison} {NAME[metric]}")
            assert_same_lists(dc.topk_self(100, metric), plain_k, f"poison {poison} top-k {NAME[metric]}")
            assert_same_csr(plain, want, NAME[metric])
    finally:
        dc.close()


# ---- 9. top-k ----
@pytest.mark.parametrize("metric", METRICS)
def test_topk_ragged(ragged, metric):
    c, full = ragged[metric]
    dc = _native.DeviceCorpus(c)
    try:
        for k in (1, 10, 299):
            assert_same_lists(dc.topk_self(k, metric), topk_self_truth(full, k), f"{NAME[metric]} k={k}")
    finally:
        dc.close()


@pytest.mark.parametrize("variant", [0, 3])
def test_topk_across_tiles(diagonal_case, variant, monkeypatch):
    c, cases = diagonal_case
    monkeypatch.setenv("PMM_GEMM_VARIANT", str(variant))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            assert_same_lists(dc.topk_self(100, metric), topk_self_truth(cases[metric][0], 100),
                              f"variant {variant} {NAME[metric]}")
    finally:
        dc.close()


def test_topk_past_the_fused_limit():
    n, d, k = 1100, 16, 1024  # k + 1 = 1025 > 1024: the route for every k
    c = f32(np.random.RandomState(9).randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in (COS, EUC):
            assert_same_lists(dc.topk_self(k, metric), topk_self_truth(ranked_self(c, metric), k), NAME[metric])
    finally:
        dc.close()


def test_topk_screened(monkeypatch):
    n, d, k = 47, 700, 10  # the smallest many-row shape of the screened-handle tests
    c = f32(np.random.RandomState(1000 * 33 + n + d + k).randn(n, d))
    c[30] = c[4]  # an exact duplicate: the row itself leaves, the duplicate stays
    want = topk_self_truth(ranked_self(c, COS), k)
    assert want[0][30, 0] == 4 and want[0][4, 0] == 30
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        got = dc.topk_self(k, COS)
        assert dc.nbytes > base, "the call did not build the screen image: it did not screen"
        assert_same_lists(got, want, "screened")
    finally:
        dc.close()


def test_topk_k_limits():
    n, d = 20, 8
    c = f32(np.random.RandomState(3).randn(n, d))
    full = ranked_self(c, COS)
    dc = _native.DeviceCorpus(c)
    one = _native.DeviceCorpus(c[:1])
    try:
        idx, sc = np.zeros((n, n), np.uint32), np.zeros((n, n), np.float32)
        for k in (n, n + 5):
            assert ctopk_self(dc, k, COS, idx, sc) == _native.PMM_ERR_ARG and "n - 1" in _native.last_error()
        assert ctopk_self(dc, 0, COS, idx, sc) == _native.PMM_ERR_ARG
        assert ctopk_self(one, 1, COS, idx, sc) == _native.PMM_ERR_ARG
        for k in (n - 1, n, 1000):  # Python clips to n - 1
            assert_same_lists(dc.topk_self(k, COS), topk_self_truth(full, n - 1), f"k={k}")
        gi, gs = one.topk_self(5, COS)
        assert gi.shape == (1, 0) and gs.shape == (1, 0)
        o, i, s = one.range_self(-INF, COS)
        assert o.tolist() == [0, 0] and i.size == 0 and s.size == 0
    finally:
        one.close()
        dc.close()


# ---- 10. refusals ----
def test_refused_handles_and_arguments():
    n, d = 300, 37
    c = f32(np.random.RandomState(9).randn(n, d))
    dc = _native.DeviceCorpus(c)
    part = dc.partition(np.arange(n, dtype=np.uint32) % 3, 3)
    d64 = _native.DeviceCorpus(c.astype(np.float64))
    b16 = _native.DeviceCorpus(c, compute="bf16")
    i8 = _native.DeviceCorpus.int8(np.clip(c * 40, -127, 127).astype(np.int8))
    idx, sc = np.zeros((n, 2), np.uint32), np.zeros((n, 2), np.float32)
    try:
        for h, code, word in ((part, _native.PMM_ERR_ARG, "partitioned"), (d64, _native.PMM_ERR_ARG, "f32 handle"),
                              (b16, _native.PMM_ERR_ARG, "f32 handle"),
                              (i8, _native.PMM_ERR_UNSUPPORTED, "f32 handle")):
            rc, _, _ = crange_self(h, 0.5, COS, 0)
            assert rc == code and word in _native.last_error(), _native.last_error()
            assert ctopk_self(h, 2, COS, idx, sc) == code and word in _native.last_error(), _native.last_error()
        for call in (lambda: part.range_self(0.5, COS), lambda: d64.topk_self(2, COS)):
            with pytest.raises(_native.PmmError) as ei:
                call()
            assert ei.value.code == _native.PMM_ERR_ARG
        rc, _, _ = crange_self(dc, float("nan"), COS, 0)
        assert rc == _native.PMM_ERR_ARG and "NaN" in _native.last_error()
        rc, _, _ = crange_self(dc, 0.5, COS, 8)  # cap > 0 without lists
        assert rc == _native.PMM_ERR_ARG
        assert ctopk_self(dc, 2, COS, None, sc) == _native.PMM_ERR_ARG
        assert ctopk_self(dc, 2, COS, idx, None) == _native.PMM_ERR_ARG
    finally:
        for h in (part, d64, b16, i8, dc):
            h.close()
    _native.set_devices([0, 0])
    try:
        sharded = _native.DeviceCorpus(c)
        try:
            assert sharded.shards == 2
            rc, _, _ = crange_self(sharded, 0.5, COS, 0)
            assert rc == _native.PMM_ERR_UNSUPPORTED and _native.last_error()
            assert ctopk_self(sharded, 2, COS, idx, sc) == _native.PMM_ERR_UNSUPPORTED
        finally:
            sharded.close()
    finally:
        _native.set_devices([])


# ---- 11. the public entries ----
@pytest.mark.parametrize("metric", METRICS)
def test_public_entries_equal_the_handles(ragged, metric):
    import pyarrow as pa

    import polars_matmul

    c, full = ragged[metric]
    t, k = median_threshold(full), 10
    dc = _native.DeviceCorpus(c)
    try:
        ho, hi, hs = dc.range_self(t, metric)
        ki, ks = dc.topk_self(k, metric)
    finally:
        dc.close()
    o, i, s = polars_matmul.within_self(c, t, NAME[metric])
    assert s.dtype == np.float64 and np.array_equal(s, hs.astype(np.float64))
    assert_same_csr((o, i, s), (ho, hi, hs), "within_self")
    ti, ts = polars_matmul.topk_self(c, k, NAME[metric])
    assert ts.dtype == np.float64 and np.array_equal(ts, ks.astype(np.float64))
    assert_same_lists((ti, ts), (ki, ks), "topk_self")
    col = pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1)), c.shape[1])
    arr = pm._within_self(col, t, NAME[metric])
    assert arr.type == pa.large_list(pm._TOPK_STRUCT) and len(arr) == c.shape[0]
    assert np.array_equal(arr.offsets.to_numpy(), ho)
    assert np.array_equal(arr.values.field("index").to_numpy(), hi)
    assert np.array_equal(arr.values.field("score").to_numpy(), hs.astype(np.float64))
    arr = pm._topk_self(col, k, NAME[metric])
    assert arr.type == pa.large_list(pm._TOPK_STRUCT) and len(arr) == c.shape[0]
    assert np.array_equal(arr.offsets.to_numpy(), np.arange(c.shape[0] + 1) * k)
    assert np.array_equal(arr.values.field("index").to_numpy(), ki.reshape(-1))
    assert np.array_equal(arr.values.field("score").to_numpy(), ks.astype(np.float64).reshape(-1))
