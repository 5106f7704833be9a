"""Grouped search on partitioned corpus handles (``DeviceCorpus.partition`` /
``topk_grouped``, pmm_corpus_partition / pmm_topk_f32_grouped /
pmm_topk_f64_grouped) and ``groups=`` on ``_topk``.

The truth is ``oracle.topk(q[ql == g], c[cl == g])`` per group with its indices
mapped through the group's row numbers; "exact" is equality of every index and
of every score's bits.  There are no tolerances in this file.
"""
from __future__ import annotations

import numpy as np
import pyarrow as pa
import pytest

import oracle
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
NONE = _native.NO_GROUP


def same_bits(a, b, dtype):
    a, b = np.ascontiguousarray(a, dtype), np.ascontiguousarray(b, dtype)
    u = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def truth(q, c, ql, cl, k, metric):
    """Per query row: (indices in c's numbering, scores) of the oracle on the row's group."""
    lists = [(np.zeros(0, np.uint32), np.zeros(0, c.dtype))] * q.shape[0]
    for g in np.unique(ql[ql != NONE]):
        ids = np.flatnonzero(cl == g)
        rows = np.flatnonzero(ql == g)
        if ids.size == 0:
            continue
        kg = min(k, ids.size)
        oi, osc = oracle.topk(np.ascontiguousarray(q[rows]), np.ascontiguousarray(c[ids]), kg, ORACLE_METRIC[metric])
        oi, osc = np.asarray(oi).astype(np.int64), np.asarray(osc)
        for j, r in enumerate(rows):
            lists[r] = (ids[oi[j]].astype(np.uint32), osc[j])
    return lists


def assert_exact(got, want, k, label, dtype=np.float32):
    idx, sc, lens = got
    assert idx.shape == sc.shape == (len(want), k) and lens.shape == (len(want),), label
    for r, (wi, ws) in enumerate(want):
        n = wi.size
        assert lens[r] == n, f"{label}: row {r} length {lens[r]} != {n}"
        assert np.array_equal(idx[r, :n], wi), f"{label}: row {r} indices {idx[r, :n]} != {wi}"
        assert same_bits(sc[r, :n], ws, dtype), f"{label}: row {r} score bits differ"
        assert np.all(idx[r, n:] == 0xFFFFFFFF) and not np.any(sc[r, n:].view(np.uint8)), f"{label}: row {r} padding"


def main_shape(dtype, d, seed):
    """m = 37, n = 1237: eight labels with segments of 1, 7, 255, 256, 257, 300
    rows and the rest (151), label 7 without corpus rows, ten corpus rows and
    two queries in no group, 17 queries in one group (two work units).
    (Segments of 1 + 7 + 255 + 256 + 257 + 300 rows do not fit in a corpus of
    1037 rows, the odd size the other suites use; every segment size is kept
    and the corpus is 200 rows longer, still no multiple of any tile.)"""
    m, n = 37, 1237
    rs = np.random.RandomState(seed)
    q, c = rs.randn(m, d).astype(dtype), rs.randn(n, d).astype(dtype)
    sizes = [1, 7, 255, 256, 257, 300]
    cl = np.concatenate([np.full(s, g) for g, s in enumerate(sizes)] + [np.full(10, NONE)]
                        + [np.full(n - sum(sizes) - 10, 6)]).astype(np.uint32)
    rs.shuffle(cl)
    ql = np.array([5] * 17 + [0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 6, 6, 6, 7, 7, 7, NONE, NONE], dtype=np.uint32)
    rs.shuffle(ql)
    assert ql.size == m and cl.size == n
    return q, c, ql, cl


# ---- 1. the main shape, three metrics, both paths ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_f32_grouped_kernel_and_loop(monkeypatch, metric):
    d, k = 37, 10
    q, c, ql, cl = main_shape(np.float32, d, 21 + metric)
    want = truth(q, c, ql, cl, k, metric)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            perm, off = _native.partition_plan(cl, 8)
            assert part.n == perm.size == 1227 and part.d == d and part.shards == 1
            assert np.array_equal(part.index_map(), perm) and np.array_equal(part.group_offsets(), off)
            assert part.nbytes == _native.partitioned_device_bytes(1227, d, 8)
            assert dc.group_offsets() is None
            for path in ("kernel", "loop"):
                monkeypatch.setenv("PMM_GROUPED", path)
                _native.timing_enable(True)
                _native.timing_reset()
                got = part.topk_grouped(q, ql, k, metric)
                launches = _native.timing_read("grouped_topk_f32")[1]
                _native.timing_enable(False)
                assert launches == (1 if path == "kernel" else 0), (path, launches)
                assert_exact(got, want, k, f"{NAME[metric]} {path}")
        finally:
            part.close()
    finally:
        dc.close()


# ---- 2. ties, NaN and zero rows, the kernel's largest k and the first k past it ----
def test_ties_nan_zero_rows_and_k_at_the_kernel_limit(monkeypatch):
    n, d = 700, 40
    rs = np.random.RandomState(31)
    c = rs.randn(n, d).astype(np.float32)
    cl = (np.arange(n) % 2).astype(np.uint32)  # group 0: even rows, group 1: odd rows (350 each)
    c[400] = c[620] = c[6]  # duplicates inside group 0
    c[401] = c[7]           # and inside group 1
    c[100] = np.nan         # a NaN row and a zero-norm row in group 0
    c[200] = 0.0
    q = np.ascontiguousarray(np.stack([c[6], c[7], rs.randn(d).astype(np.float32), c[6]]))
    ql = np.array([0, 1, 0, 1], dtype=np.uint32)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 2)
        try:
            monkeypatch.setenv("PMM_GROUPED", "kernel")
            for k, kernel_launches in ((10, 1), (128, 1), (129, 0), (350, 0)):
                for metric in (COS, DOT, EUC):
                    _native.timing_enable(True)
                    _native.timing_reset()
                    got = part.topk_grouped(q, ql, k, metric)
                    launches = _native.timing_read("grouped_topk_f32")[1]
                    _native.timing_enable(False)
                    assert launches == kernel_launches, (k, launches)
                    assert_exact(got, truth(q, c, ql, cl, k, metric), k, f"k={k} {NAME[metric]}")
                    if metric == COS:
                        assert got[0][0, :3].tolist() == [6, 400, 620], got[0][0, :4]  # the lower parent row first
                        assert got[0][1, :2].tolist() == [7, 401], got[0][1, :3]
                    # (only a dot product stays NaN: the reference's cosine of a NaN norm is 0
                    # and its max clamps a NaN distance to 0)
                    if k == 350 and metric == DOT:
                        assert got[0][0, -1] == 100, "the NaN row ranks last"
        finally:
            part.close()
    finally:
        dc.close()


# ---- 3. one call, both paths: dispatch by segment size ----
def test_one_call_uses_both_paths(monkeypatch):
    d, k = 37, 10
    q, c, ql, cl = main_shape(np.float32, d, 41)
    monkeypatch.delenv("PMM_GROUPED", raising=False)
    monkeypatch.setenv("PMM_GROUPED_SEG_MAX", "256")
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            _native.timing_enable(True)
            _native.timing_reset()
            got = part.topk_grouped(q, ql, k, COS)
            grouped = _native.timing_read("grouped_topk_f32")[1]
            fused = _native.timing_read("gemm_f32_topk")[1]
            _native.timing_enable(False)
            # segments of 1, 7, 151, 255, 256 rows: one launch; 257, 300: one fused pass each
            assert grouped == 1 and fused == 2, (grouped, fused)
            assert_exact(got, truth(q, c, ql, cl, k, COS), k, "mixed")
        finally:
            part.close()
    finally:
        dc.close()


# ---- 4. an f64 parent ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_f64_grouped(metric):
    d, k = 20, 10
    q, c, ql, cl = main_shape(np.float64, d, 51 + metric)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            assert part.device_dtype == _native.DTYPE_F64
            assert part.nbytes == _native.partitioned_device_bytes(1227, d, 8, np.float64)
            got = part.topk_grouped(q, ql, k, metric)
            assert got[1].dtype == np.float64
            assert_exact(got, truth(q, c, ql, cl, k, metric), k, f"f64 {NAME[metric]}", np.float64)
        finally:
            part.close()
    finally:
        dc.close()


# ---- 5. through _topk(groups=) on Arrow arrays (a corpus past the cache's 1 MiB floor) ----
def arrow_rows(a):
    return pa.FixedSizeListArray.from_arrays(pa.array(a.reshape(-1)), a.shape[1])


def ragged(out):
    off = out.offsets.to_numpy()
    idx = out.values.field("index").to_numpy(zero_copy_only=False)
    sc = out.values.field("score").to_numpy(zero_copy_only=False)
    return [(idx[off[i]:off[i + 1]], sc[off[i]:off[i + 1]]) for i in range(len(out))]


@pytest.fixture
def clean_cache():
    pm.clear_corpus_cache()
    yield
    pm.clear_corpus_cache()


def grouped_inputs(seed):
    m, n, d = 23, 4111, 64
    rs = np.random.RandomState(seed)
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    names = np.array(["de", "en", "fr", "it", "xx"])
    cl = names[rs.randint(0, 4, size=n)].astype(object)  # ("xx": no corpus row)
    cl[::97] = None
    ql = names[rs.randint(0, 5, size=m)].astype(object)
    ql[3] = None
    return q, c, pa.array(ql, type=pa.string()), pa.array(cl, type=pa.string())


def per_label_subset(aq_rows, q, ac, ql, cl, k, metric, **kw):
    """Per query row the lists of _topk(..., subset=cl == g) on the label's queries."""
    want = [None] * q.shape[0]
    qn, cn = np.array(ql.to_pylist(), dtype=object), np.array(cl.to_pylist(), dtype=object)
    for r in range(q.shape[0]):
        if qn[r] is None or not np.any(cn == qn[r]):
            want[r] = (np.zeros(0, np.uint32), np.zeros(0))
    for g in sorted({x for x in qn if x is not None}):
        rows = np.flatnonzero(qn == g)
        mask = cn == g
        if not mask.any():
            continue
        out = pm._topk(aq_rows(rows), ac, k, metric, subset=pa.array(mask.astype(bool)), **kw)
        for j, (i, s) in enumerate(ragged(out)):
            want[rows[j]] = (i, s)
    return want


def assert_lists(got, want, label):
    assert len(got) == len(want)
    for r, ((gi, gs), (wi, ws)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), f"{label}: row {r} indices {gi} != {wi}"
        assert same_bits(gs, ws, np.float64), f"{label}: row {r} score bits differ"


def test_topk_groups_on_arrow_arrays(clean_cache):
    k = 10
    q, c, ql, cl = grouped_inputs(61)
    aq, ac = arrow_rows(q), arrow_rows(c)
    _native.timing_enable(True)
    _native.timing_reset()
    out = pm._topk(aq, ac, k, "cosine", groups=(ql, cl))
    first = _native.timing_read("subset_gather")[1]
    _native.timing_reset()
    out2 = pm._topk(aq, ac, k, "cosine", groups=(ql, cl))
    second = _native.timing_read("subset_gather")[1]
    _native.timing_enable(False)
    assert first == 1 and second == 0, "the second call on the same label array partitioned again"
    assert out.type == pa.large_list(pm._TOPK_STRUCT) and out.equals(out2)
    parts = [v[1] for key, v in pm._cache.items() if "groups" in key]
    assert len(parts) == 1 and len(pm._cache) == 2
    # ragged offsets: min(k, rows of the label) entries, none for a null or unseen label
    qn, cn = ql.to_pylist(), np.array(cl.to_pylist(), dtype=object)
    lens = [0 if g is None else min(k, int((cn == g).sum())) for g in qn]
    assert np.array_equal(np.diff(out.offsets.to_numpy()), lens) and 0 in lens and k in lens
    # every label's lists equal subset= on the matching queries: the path that predates this one
    want = per_label_subset(lambda rows: arrow_rows(np.ascontiguousarray(q[rows])), q, ac, ql, cl, k, "cosine")
    assert_lists(ragged(out), want, "groups= vs subset=")
    pm.clear_corpus_cache()
    assert all(x.closed for x in parts)


# ---- 6. refusals and fallbacks ----
def test_a_partitioned_handle_serves_grouped_calls_only():
    q, c, ql, cl = main_shape(np.float32, 37, 71)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            with pytest.raises(_native.PmmError) as ei:
                part.topk(q, 5, COS)
            assert ei.value.code == _native.PMM_ERR_ARG and "partitioned" in str(ei.value)
            for sel in (np.ones(part.n, bool), np.array([0, 1], dtype=np.uint32)):
                with pytest.raises(_native.PmmError) as ei:
                    part.subset(sel)
                assert ei.value.code == _native.PMM_ERR_ARG and "partitioned" in str(ei.value)
            with pytest.raises(_native.PmmError) as ei:
                part.partition(np.zeros(part.n, dtype=np.uint32), 1)
            assert ei.value.code == _native.PMM_ERR_ARG and "partitioned" in str(ei.value)
            with pytest.raises(_native.PmmError) as ei:
                part.topk_grouped(q, np.full(q.shape[0], 8, dtype=np.uint32), 5, COS)
            assert ei.value.code == _native.PMM_ERR_ARG and "qlabels[0]" in str(ei.value)
        finally:
            part.close()
        with pytest.raises(_native.PmmError) as ei:
            dc.partition(np.full(c.shape[0], NONE, dtype=np.uint32), 3)
        assert ei.value.code == _native.PMM_ERR_ARG
        with pytest.raises(_native.PmmError) as ei:
            dc.topk_grouped(q, ql, 5, COS)
        assert ei.value.code == _native.PMM_ERR_ARG and "not partitioned" in str(ei.value)
        sub = dc.subset(np.arange(0, c.shape[0], 2, dtype=np.uint32))
        try:
            with pytest.raises(_native.PmmError) as ei:
                sub.partition(np.zeros(sub.n, dtype=np.uint32), 1)
            assert ei.value.code == _native.PMM_ERR_ARG and "derived" in str(ei.value)
        finally:
            sub.close()
    finally:
        dc.close()


def test_fallbacks_give_the_same_lists(monkeypatch, clean_cache):
    k = 10
    q, c, ql, cl = grouped_inputs(81)
    aq, ac = arrow_rows(q), arrow_rows(c)
    want = ragged(pm._topk(aq, ac, k, "euclidean", groups=(ql, cl)))

    def no_handle(self, labels, G):
        raise AssertionError("the fallback partitioned a handle")

    with monkeypatch.context() as mp:
        mp.setattr(_native.DeviceCorpus, "partition", no_handle)
        pm.set_devices([0, 0])
        try:
            got = ragged(pm._topk(aq, ac, k, "euclidean", groups=(ql, cl)))
        finally:
            pm.set_devices([])
        assert_lists(got, want, "device 0 listed twice")
        got = ragged(pm._topk(q, c, k, "euclidean", groups=(ql, cl)))  # numpy inputs: never cached
        assert_lists(got, want, "numpy inputs")
        import polars_matmul

        gi, gs = polars_matmul.topk(q, c, k, "euclidean", groups=(ql, cl))
        assert gi.shape == gs.shape == (q.shape[0], k)
        for r, (wi, ws) in enumerate(want):
            assert np.array_equal(gi[r, :wi.size], wi) and same_bits(gs[r, :wi.size], ws, np.float64)
            assert np.all(gi[r, wi.size:] == 0xFFFFFFFF) and np.all(np.isnan(gs[r, wi.size:]))
        # compute="bf16": per label on the host rows, bit for bit what subset= gives per label
        got = ragged(pm._topk(aq, ac, k, "cosine", compute="bf16", groups=(ql, cl)))
        ref = per_label_subset(lambda rows: arrow_rows(np.ascontiguousarray(q[rows])), q, ac, ql, cl, k, "cosine",
                               compute="bf16")
        assert_lists(got, ref, "bf16 fallback vs subset=")
