"""Subset search on resident corpus handles: a handle derived on the device
from a parent handle and a set of allowed rows (``DeviceCorpus.subset``,
pmm_corpus_subset_mask / pmm_corpus_subset_ids) and ``subset=`` on ``_topk``.

The truth, unless another is named, is ``oracle.topk`` on ``c[ids]`` with its
indices mapped through ``ids``; "exact" is equality of every index and of every
score's bits.  There are no tolerances in this file.
"""
from __future__ import annotations

import threading

import numpy as np
import pyarrow as pa
import pytest

import oracle
from parity import exact_match_rate
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}


def same_bits(a, b, dtype):
    a, b = np.ascontiguousarray(a, dtype), np.ascontiguousarray(b, dtype)
    u = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def truth(q, c, ids, k, metric):
    """oracle.topk on c[ids], its indices in c's numbering."""
    oi, osc = oracle.topk(q, np.ascontiguousarray(c[ids]), k, ORACLE_METRIC[metric])
    return np.asarray(ids)[np.asarray(oi).astype(np.int64)].astype(np.uint32), np.asarray(osc)


def assert_exact(got, want, label, dtype=np.float32):
    assert got[0].shape == want[0].shape, f"{label}: {got[0].shape} vs {want[0].shape}"
    assert exact_match_rate(got[0], want[0]) == 1.0 and np.array_equal(got[0], want[0]), f"{label}: indices differ"
    assert same_bits(got[1], want[1], dtype), f"{label}: score bits differ"


def half_mask(n, seed):
    """About half the rows, rows 0 and n - 1 among them."""
    mask = np.random.RandomState(seed).rand(n) < 0.5
    mask[0] = mask[n - 1] = True
    return mask


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def image_bytes(s, d):
    return _native.subset_device_bytes(s, d, screen=True) - _native.subset_device_bytes(s, d)


# ---- 1. f32 handle, three metrics; ragged in every dimension (dp = 64) ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_f32_subset_by_mask_and_by_ids(metric):
    m, n, d, k = 33, 1037, 37, 10
    rs = np.random.RandomState(11 + metric)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    mask = half_mask(n, 5)
    ids = np.flatnonzero(mask).astype(np.uint32)
    want = truth(q, c, ids, k, metric)
    dc = _native.DeviceCorpus(c)
    try:
        assert dc.index_map() is None
        for how, sel in (("mask", mask), ("ids", ids)):
            sub = dc.subset(sel)
            try:
                assert sub.n == ids.size and sub.d == d and sub.shards == 1
                assert sub.device_dtype == _native.DTYPE_F32
                assert sub.nbytes == _native.subset_device_bytes(ids.size, d)
                assert np.array_equal(sub.index_map(), ids), how
                assert_exact(sub.topk(q, k, metric), want, f"{NAME[metric]} by {how}")
            finally:
                sub.close()
    finally:
        dc.close()


# ---- 2. ties: the lower PARENT index first, an excluded duplicate never ----
def test_ties_break_by_parent_index():
    n, d = 1037, 37
    rs = np.random.RandomState(2)
    c = f32(rs.randn(n, d))
    c[400] = c[900] = c[5]
    q = f32(c[5:6])
    dc = _native.DeviceCorpus(c)
    try:
        for drop, first_two in ((5, [400, 900]), (400, [5, 900]), (900, [5, 400])):
            mask = np.ones(n, bool)
            mask[drop] = False
            mask[1::7] = False  # (and some others; 5, 400, 900 are not among them)
            mask[[x for x in (5, 400, 900) if x != drop]] = True
            ids = np.flatnonzero(mask)
            sub = dc.subset(mask)
            try:
                for metric in (COS, DOT, EUC):
                    got = sub.topk(q, 10, metric)
                    assert got[0][0, :2].tolist() == first_two, (drop, NAME[metric], got[0][0])
                    assert drop not in got[0]
                    assert_exact(got, truth(q, c, ids, 10, metric), f"drop {drop} {NAME[metric]}")
            finally:
                sub.close()
    finally:
        dc.close()


# ---- 3. edges ----
def test_edges_all_rows_one_row_k_equals_s():
    m, n, d = 33, 1037, 37
    rs = np.random.RandomState(3)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        # every row selected: the parent's own lists
        sub = dc.subset(np.ones(n, bool))
        try:
            assert np.array_equal(sub.index_map(), np.arange(n))
            for metric in (COS, DOT, EUC):
                pi, ps = dc.topk(q, 10, metric)
                assert_exact(sub.topk(q, 10, metric), (pi, ps), f"all rows {NAME[metric]}")
        finally:
            sub.close()
        # one row, k = 1
        sub = dc.subset(np.array([777], dtype=np.uint32))
        try:
            got = sub.topk(q, 1, COS)
            assert (got[0] == 777).all()
            assert_exact(got, truth(q, c, np.array([777]), 1, COS), "s = 1")
            with pytest.raises(_native.PmmError) as ei:  # the C entry does not clip
                sub.topk(q, 2, COS)
            assert ei.value.code == _native.PMM_ERR_ARG
        finally:
            sub.close()
        # k = s exactly
        ids = np.array([0, 3, 64, 65, 500, 1000, 1036], dtype=np.uint32)
        sub = dc.subset(ids)
        try:
            for metric in (COS, DOT, EUC):
                got = sub.topk(q, ids.size, metric)
                assert all(sorted(r) == ids.tolist() for r in got[0].tolist())
                assert_exact(got, truth(q, c, ids, ids.size, metric), f"k = s {NAME[metric]}")
        finally:
            sub.close()
    finally:
        dc.close()


# ---- 4. bitmap compaction: n = 70001 crosses five compaction blocks (a block
# of 256 lanes x one 64-bit word takes 16384 rows); d = 8 keeps the gather trivial
@pytest.mark.parametrize("bit_offset", [0, 3, 13])
def test_bitmap_compaction(bit_offset):
    n, d, block = 70001, 8, 16384
    rs = np.random.RandomState(40 + bit_offset)
    c = f32(rs.randn(n, d))
    masks = {"all ones": np.ones(n, bool), "last row": np.zeros(n, bool), "first row": np.zeros(n, bool),
             "one word per block": np.zeros(n, bool), "random": rs.rand(n) < 0.37}
    masks["last row"][n - 1] = True
    masks["first row"][0] = True
    for b0 in range(0, n, block):
        masks["one word per block"][b0 + 7 * 64:b0 + 8 * 64] = True
    dc = _native.DeviceCorpus(c)
    try:
        for label, mask in masks.items():
            # the selection sits at bit `bit_offset` of a longer bitmap whose
            # other bits are set: they must not be read as rows
            arr = pa.array(np.concatenate([np.ones(bit_offset, bool), mask, np.ones(11, bool)])).slice(bit_offset, n)
            assert arr.offset == bit_offset and len(arr) == n
            sub = dc.subset(arr)
            try:
                want = np.flatnonzero(mask)
                got = sub.index_map()
                assert got.dtype == np.uint32 and np.array_equal(got, want), f"{label} at offset {bit_offset}"
                assert sub.n == want.size
            finally:
                sub.close()
        # the gathered rows are the selected ones: a search of the last case finds each row by itself
        ids = np.flatnonzero(masks["one word per block"])
        sub = dc.subset(masks["one word per block"])
        try:
            got = sub.topk(c[ids[-3:]], 1, EUC)
            assert got[0].reshape(-1).tolist() == ids[-3:].tolist()
        finally:
            sub.close()
        with pytest.raises(_native.PmmError) as ei:
            dc.subset(np.zeros(n, bool))
        assert ei.value.code == _native.PMM_ERR_ARG and "empty selection" in str(ei.value)
    finally:
        dc.close()


# ---- 5. the materialised route (k > 1024) behind the remap ----
def test_materialised_route_on_a_derived_handle():
    m, n, d, s, k = 8, 2200, 32, 1100, 1025
    rs = np.random.RandomState(5)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    ids = np.sort(rs.permutation(n)[:s]).astype(np.uint32)
    dc = _native.DeviceCorpus(c)
    try:
        sub = dc.subset(ids)
        try:
            assert_exact(sub.topk(q, k, DOT), truth(q, c, ids, k, DOT), "k = 1025 dot")
        finally:
            sub.close()
    finally:
        dc.close()


# ---- 6. the screen on derived handles (the existing screened route test's shape) ----
SM, SN, SD, SK = 70, 3037, 256, 10


def screen_case(seed):
    rs = np.random.RandomState(seed)
    q, c = f32(rs.randn(SM, SD)), f32(rs.randn(SN, SD))
    mask = half_mask(SN, seed + 1)
    return q, c, mask, np.flatnonzero(mask)


def unscreened_subset_lists(monkeypatch, q, c, mask):
    """The same subset searched under PMM_F32_SCREEN=0 (leaves the knob at 1)."""
    monkeypatch.setenv("PMM_F32_SCREEN", "0")
    dc = _native.DeviceCorpus(c)
    try:
        sub = dc.subset(mask)
        try:
            got = sub.topk(q, SK, COS)
            assert sub.nbytes == _native.subset_device_bytes(sub.n, SD), "knob off built an image"
        finally:
            sub.close()
    finally:
        dc.close()
        monkeypatch.setenv("PMM_F32_SCREEN", "1")
    return got


def test_screen_image_is_gathered_from_a_parent_that_has_one(monkeypatch):
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    q, c, mask, ids = screen_case(60)
    dc = _native.DeviceCorpus(c)
    try:
        dc.topk(q, SK, COS)  # the parent builds its image
        assert dc.nbytes == _native.corpus_device_bytes(SN, SD, np.float32, screen=True)
        sub = dc.subset(mask)
        try:
            full = _native.subset_device_bytes(ids.size, SD, screen=True)
            assert sub.nbytes == full, "no gathered image before the first call"
            got = sub.topk(q, SK, COS)
            assert sub.nbytes == full
            assert_exact(got, truth(q, c, ids, SK, COS), "gathered image vs oracle")
            assert_exact(got, unscreened_subset_lists(monkeypatch, q, c, mask), "gathered image vs unscreened")
        finally:
            sub.close()
    finally:
        dc.close()


def test_screen_image_is_built_by_the_derived_handle_of_a_fresh_parent(monkeypatch):
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    q, c, mask, ids = screen_case(61)
    dc = _native.DeviceCorpus(c)
    try:
        sub = dc.subset(mask)
        try:
            base = _native.subset_device_bytes(ids.size, SD)
            assert sub.nbytes == base
            got = sub.topk(q, SK, COS)
            assert sub.nbytes == base + image_bytes(ids.size, SD), "the first screened call built no image"
            assert dc.nbytes == _native.corpus_device_bytes(SN, SD, np.float32)  # (the parent was never called)
            assert_exact(got, truth(q, c, ids, SK, COS), "own image vs oracle")
            assert_exact(got, unscreened_subset_lists(monkeypatch, q, c, mask), "own image vs unscreened")
        finally:
            sub.close()
    finally:
        dc.close()


def test_never_screened_parent_is_not_inherited(monkeypatch):
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    q, c, mask, _ = screen_case(62)
    c[1500] = 0.0  # an unsafe row: the parent keeps no image and never screens
    dc = _native.DeviceCorpus(c)
    try:
        dc.topk(q, SK, COS)
        assert dc.nbytes == _native.corpus_device_bytes(SN, SD, np.float32)
        for with_row in (False, True):
            mask[1500] = with_row
            ids = np.flatnonzero(mask)
            sub = dc.subset(mask)
            try:
                base = _native.subset_device_bytes(ids.size, SD)
                assert sub.nbytes == base
                got = sub.topk(q, SK, COS)
                assert sub.nbytes == base + (0 if with_row else image_bytes(ids.size, SD)), f"with the row: {with_row}"
                assert_exact(got, truth(q, c, ids, SK, COS), f"zero row selected: {with_row}")
            finally:
                sub.close()
    finally:
        dc.close()


# ---- 7. bf16 handle: the handle / host-entry relation holds for derived handles ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_bf16_subset_equals_the_host_entry_on_the_taken_rows(metric):
    m, n, d, k = 130, 4099, 96, 10
    rs = np.random.RandomState(70 + metric)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    mask = half_mask(n, 71)
    ids = np.flatnonzero(mask).astype(np.uint32)
    hi, hs = _native.topk_host(q, np.ascontiguousarray(c[ids]), k, metric, compute=_native.COMPUTE_BF16)
    dc = _native.DeviceCorpus(c, compute="bf16")
    try:
        sub = dc.subset(mask)
        try:
            assert sub.device_dtype == _native.DTYPE_BF16 and sub.compute == "bf16"
            assert sub.nbytes == _native.subset_device_bytes(ids.size, d, compute="bf16")
            assert_exact(sub.topk(q, k, metric), (ids[hi], hs), f"bf16 {NAME[metric]}")
        finally:
            sub.close()
    finally:
        dc.close()


# ---- 8. f64 handle, both f64 paths ----
@pytest.mark.parametrize("fused", ["1", "0"])
def test_f64_subset(monkeypatch, fused):
    monkeypatch.setenv("PMM_F64_FUSED", fused)
    m, n, d, k = 30, 1000, 20, 10
    rs = np.random.RandomState(8)
    q, c = rs.randn(m, d), rs.randn(n, d)
    mask = half_mask(n, 81)
    ids = np.flatnonzero(mask).astype(np.uint32)
    dc = _native.DeviceCorpus(c)
    try:
        for sel in (mask, ids):
            sub = dc.subset(sel)
            try:
                assert sub.device_dtype == _native.DTYPE_F64
                assert sub.nbytes == _native.subset_device_bytes(ids.size, d, np.float64)
                for metric in (COS, DOT, EUC):
                    assert_exact(sub.topk(q, k, metric), truth(q, c, ids, k, metric), f"f64 {NAME[metric]}",
                                 np.float64)
            finally:
                sub.close()
    finally:
        dc.close()


# ---- 9. through _topk on Arrow arrays (corpora past the cache's 1 MiB floor) ----
def arrow_rows(a, kind):
    vals = pa.array(a.reshape(-1))
    if kind == "fixed":
        return pa.FixedSizeListArray.from_arrays(vals, a.shape[1])
    return pa.ListArray.from_arrays(pa.array(np.arange(a.shape[0] + 1, dtype=np.int32) * a.shape[1]), vals)


def lists_of(out, m):
    flat = out.values
    idx = flat.field("index").to_numpy(zero_copy_only=False).reshape(m, -1)
    return idx, flat.field("score").to_numpy(zero_copy_only=False).reshape(m, -1)


@pytest.fixture
def clean_cache():
    pm.clear_corpus_cache()
    yield
    pm.clear_corpus_cache()


@pytest.mark.parametrize("kind", ["fixed", "list"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_topk_subset_on_arrow_arrays(monkeypatch, clean_cache, kind, dtype):
    m, n, d, k = 9, 4111, 64, 10
    rs = np.random.RandomState(90)
    q, c = rs.randn(m, d).astype(dtype), rs.randn(n, d).astype(dtype)
    mask = half_mask(n, 91)
    ids = np.flatnonzero(mask)
    aq, ac = arrow_rows(q, kind), arrow_rows(c, kind)
    made = []
    real = _native.DeviceCorpus.subset

    def counting(self, sel):
        made.append(sel)
        return real(self, sel)

    monkeypatch.setattr(_native.DeviceCorpus, "subset", counting)
    wi, ws = truth(q, c, ids, k, COS)
    sels = (pa.array(mask), pa.array(ids[::-1].astype(np.uint32)))  # (the ids unsorted: sorted on the host)
    for sel in sels:
        for call in range(2):
            gi, gs = lists_of(pm._topk(aq, ac, k, "cosine", subset=sel), m)
            assert gi.max() > ids.size, "indices number the filtered rows, not the corpus"
            assert np.array_equal(gi, wi) and same_bits(gs, ws, np.float64), f"{kind} call {call}"
    assert len(made) == 2, "a second call with the same selection derived a second handle"
    derived = [v[1] for key, v in pm._cache.items() if "subset" in key]
    assert len(derived) == 2 and len(pm._cache) == 3
    assert all(np.array_equal(x.index_map(), ids) for x in derived)
    # nulls count as false; k clips to the number of selected rows
    few = np.array([3, 64, 4000])
    sel = pa.array([True if i in few else (None if i % 3 else False) for i in range(n)])
    gi, gs = lists_of(pm._topk(aq, ac, k, "cosine", subset=sel), m)
    assert gi.shape == (m, 3)
    wi, ws = truth(q, c, few, k, COS)
    assert np.array_equal(gi, wi) and same_bits(gs, ws, np.float64)
    pm.clear_corpus_cache()
    assert all(x.closed for x in derived) and not pm._cache


# ---- 10. the fallbacks give the same lists ----
def test_fallbacks_give_the_same_lists(monkeypatch, clean_cache):
    m, n, d, k = 9, 4111, 64, 10
    rs = np.random.RandomState(100)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    mask = half_mask(n, 101)
    ids = np.flatnonzero(mask)
    aq, ac, sel = arrow_rows(q, "fixed"), arrow_rows(c, "fixed"), pa.array(mask)
    wi, ws = truth(q, c, ids, k, EUC)

    def no_handle(self, sel):
        raise AssertionError("the fallback derived a handle")

    with monkeypatch.context() as mp:
        mp.setattr(pm, "_CACHE_ON", False)  # PMM_CORPUS_CACHE=0
        mp.setattr(_native.DeviceCorpus, "subset", no_handle)
        gi, gs = lists_of(pm._topk(aq, ac, k, "euclidean", subset=sel), m)
        assert np.array_equal(gi, wi) and same_bits(gs, ws, np.float64), "cache off"
        gi, gs = lists_of(pm._topk(q, c, k, "euclidean", subset=mask), m)  # numpy inputs: never cached
        assert np.array_equal(gi, wi) and same_bits(gs, ws, np.float64), "numpy inputs"
    import polars_matmul

    gi, gs = polars_matmul.topk(q, c, k, "euclidean", subset=ids[::-1])
    assert np.array_equal(gi, wi) and same_bits(gs, ws, np.float64), "numpy-level topk"
    pm.set_devices([0, 0])
    try:
        with monkeypatch.context() as mp:
            mp.setattr(_native.DeviceCorpus, "subset", no_handle)
            gi, gs = lists_of(pm._topk(aq, ac, k, "euclidean", subset=sel), m)
            assert np.array_equal(gi, wi) and same_bits(gs, ws, np.float64), "device list of two"
        dc = _native.DeviceCorpus(c)
        try:
            assert dc.shards == 2
            for bad in (mask, ids.astype(np.uint32)):
                with pytest.raises(_native.PmmError) as ei:
                    dc.subset(bad)
                assert ei.value.code == _native.PMM_ERR_UNSUPPORTED and "sharded" in str(ei.value)
        finally:
            dc.close()
    finally:
        pm.set_devices([])


# ---- 11. refusals ----
def test_refusals():
    n, d = 1037, 37
    c = f32(np.random.RandomState(110).randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        sub = dc.subset(np.arange(0, n, 2, dtype=np.uint32))
        try:
            for sel in (np.ones(sub.n, bool), np.array([0, 1], dtype=np.uint32)):
                with pytest.raises(_native.PmmError) as ei:
                    sub.subset(sel)
                assert ei.value.code == _native.PMM_ERR_ARG and "derived" in str(ei.value)
        finally:
            sub.close()
        for ids, where in (([3, 9, 9, 20], "ids[2]"), ([3, 9, 8, 20], "ids[2]"), ([3, 9, n], "ids[2]"),
                           ([5, 4], "ids[1]")):
            with pytest.raises(_native.PmmError) as ei:
                dc.subset(np.array(ids, dtype=np.uint32))
            assert ei.value.code == _native.PMM_ERR_ARG and where in str(ei.value), (ids, str(ei.value))
        with pytest.raises(_native.PmmError) as ei:
            dc.subset(np.zeros(0, dtype=np.uint32))
        assert ei.value.code == _native.PMM_ERR_ARG
    finally:
        dc.close()


# ---- 12. concurrency, bounded ----
def test_four_threads_derive_search_and_destroy():
    m, n, d, k = 33, 1037, 37, 10
    rs = np.random.RandomState(120)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    masks = [half_mask(n, 121 + t) for t in range(4)]
    wants = [truth(q, c, np.flatnonzero(mk), k, COS) for mk in masks]
    dc = _native.DeviceCorpus(c)
    errors = []

    def work(t):
        try:
            for _ in range(2):
                sub = dc.subset(masks[t])
                try:
                    assert np.array_equal(sub.index_map(), np.flatnonzero(masks[t]))
                    assert_exact(sub.topk(q, k, COS), wants[t], f"thread {t}")
                finally:
                    sub.close()
        except BaseException as e:  # noqa: BLE001 - reported on the main thread
            errors.append((t, repr(e)))

    try:
        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
    finally:
        dc.close()
