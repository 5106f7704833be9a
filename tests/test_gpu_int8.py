"""Int8 rows on the int8 MFMA (pmm_topk_i8*, DESIGN.md §4d "Int8 rows"): the f64 route's
answer, bit for bit.

The bar of every case: indices and f64 score bits equal the oracle's f64 path
on the int8 values cast to f64 (oracle_similarity_f64 + oracle_select_topk_f64
under the fixed total order) AND pmm_topk_f64 on the same cast.  No tolerance
anywhere in this file.  One oracle score matrix per (inputs, metric) serves
every k and both m.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import pyarrow as pa
import pytest

import oracle
from polars_matmul import _native
from polars_matmul._polars_matmul import _topk, clear_corpus_cache

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
METRICS = (COS, DOT, EUC)
M = 70
DIMS = (1, 37, 64, 255, 256, 257, 768, 1000, 1536,
        2000,   # pads to 2048, the int8 scan's limit
        2049)   # just past it: both sides widened, the f64 path


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ks_of(n):
    return sorted({min(k, n) for k in (1, 10, 100, min(n, 1000))})


def same(got, want, label):
    assert got[0].shape == want[0].shape and got[1].dtype == np.float64, label
    assert np.array_equal(got[0], want[0]), f"{label}: indices differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{label}: score bits differ"


def check_all(q, c, label, ks=None, ms=(1, M), metrics=METRICS, search=_native.topk_i8_host):
    """Every (metric, k, m) of these inputs against the oracle and pmm_topk_f64."""
    qd, cd = q.astype(np.float64), c.astype(np.float64)
    for metric in metrics:
        S = oracle.similarity(qd, cd, metric)
        for k in (ks or ks_of(c.shape[0])):
            want = oracle.select_topk(S, k, metric != EUC)
            for m in ms:
                tag = f"{label} metric={metric} k={k} m={m}"
                got = search(q[:m], c, k, metric)
                same(got, (want[0][:m], want[1][:m]), tag + " vs oracle")
                same(got, _native.topk_host(qd[:m], cd, k, metric), tag + " vs pmm_topk_f64")


def uniform(n, d, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(-128, 128, size=(M, d)).astype(np.int8),
            rs.randint(-128, 128, size=(n, d)).astype(np.int8))


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", (5, 1000, 3001))
def test_uniform_rows_equal_the_f64_route(n, d):
    q, c = uniform(n, d, 1000 * n + d)
    check_all(q, c, f"uniform n={n} d={d}")


@pytest.mark.parametrize("d", (37, 256))
def test_ternary_rows_tie_massively(d):
    rs = np.random.RandomState(d)
    q = rs.randint(-1, 2, size=(M, d)).astype(np.int8)
    c = rs.randint(-1, 2, size=(3001, d)).astype(np.int8)
    check_all(q, c, f"ternary d={d}")


def test_extreme_rows_largest_dot():
    d = 1536
    rs = np.random.RandomState(7)
    q = rs.randint(-128, 128, size=(M, d)).astype(np.int8)
    c = rs.randint(-128, 128, size=(1000, d)).astype(np.int8)
    q[0::3] = -128
    q[1::3] = 127
    c[0::4] = -128
    c[1::4] = 127
    check_all(q, c, "extremes")


def test_zero_rows_score_plus_zero():
    q, c = uniform(1000, 64, 11)
    q[::5] = 0
    c[::3] = 0
    check_all(q, c, "zero rows")
    idx, sc = _native.topk_i8_host(q[:1], c, 1000, COS)  # a zero query row: every score is +0.0, in index order
    assert np.array_equal(idx[0], np.arange(1000, dtype=np.uint32))
    assert np.array_equal(bits(sc), np.zeros((1, 1000), np.uint64))


def test_identical_rows_overflow_the_band_and_rerun(monkeypatch):
    """600 equal corpus rows tie at every place of a k = 10 list.  With the
    candidate buffers lowered to 64 entries the rows overflow, are listed and
    searched again on the widened rows: the same bits."""
    q, c = uniform(3001, 64, 5)
    c[100:700] = q[3]  # equal to a query row: they lead its cosine list, tie in dot and euclidean
    check_all(q, c, "identical rows", ks=(10,))
    monkeypatch.setenv("PMM_I8_CAP", "64")
    _native.timing_enable(True)
    _native.timing_reset()
    try:
        check_all(q, c, "identical rows, 64-entry buffers", ks=(10,))
        assert _native.timing_read("widen_i8_f64")[1] > 0, "no row was re-run"
    finally:
        _native.timing_enable(False)


def test_duplicates_straddle_the_kth_place():
    rs = np.random.RandomState(9)
    base = rs.randint(-128, 128, size=(40, 255)).astype(np.int8)
    c = base[rs.randint(0, 40, size=3001)]
    q = rs.randint(-128, 128, size=(M, 255)).astype(np.int8)
    check_all(q, c, "duplicates")


def _device_search(q, c, k, metric, workspace=True):
    import torch

    def dev_rows(a):
        dp = -(-a.shape[1] // 64) * 64
        t = torch.zeros((a.shape[0], dp), dtype=torch.int8, device="cuda")
        t[:, :a.shape[1]] = torch.from_numpy(a).cuda()
        return t, dp

    (tq, dp), (tc, _) = dev_rows(q), dev_rows(c)
    m, n, d = q.shape[0], c.shape[0], q.shape[1]
    oi = torch.empty((m, k), dtype=torch.int32, device="cuda")
    os_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
    nbytes = _native.i8_workspace_bytes(m, n, d, k, metric) if workspace else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _native.topk_i8_device(tq.data_ptr(), dp, m, tc.data_ptr(), dp, n, d, k, metric, oi.data_ptr(), os_.data_ptr(),
                           workspace=ws.data_ptr() if workspace else 0, workspace_bytes=nbytes,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy().view(np.uint32), os_.cpu().numpy()


@pytest.mark.parametrize("d,k", [(257, 10), (2049, 10), (64, 1000)])
def test_handle_host_and_device_entries_agree(d, k):
    q, c = uniform(1000, d, 3 * d + k)
    dc = _native.DeviceCorpus.int8(c)
    try:
        assert dc.device_dtype == _native.DTYPE_I8 and dc.shards == 1
        assert dc.nbytes == _native.corpus_device_bytes(1000, d, np.int8) == 1000 * (-(-d // 64) * 64) + 8000
        for metric in METRICS:
            want = _native.topk_i8_host(q, c, k, metric)
            same(dc.topk(q, k, metric), want, f"handle d={d} metric={metric}")
            same(_device_search(q, c, k, metric), want, f"device d={d} metric={metric}")
            same(_device_search(q, c, k, metric, workspace=False), want, f"device, arena d={d} metric={metric}")
    finally:
        dc.close()
    check_all(q, c, f"entries d={d}", ks=(k,), ms=(M,))


def test_two_threads_on_one_handle():
    q, c = uniform(3001, 256, 21)
    dc = _native.DeviceCorpus.int8(c)
    want = {metric: _native.topk_i8_host(q, c, 100, metric) for metric in METRICS}
    out, errs = {}, []

    def run(t):
        try:
            for rep in range(3):
                for metric in METRICS:
                    out[(t, rep, metric)] = dc.topk(q, 100, metric)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    ts = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dc.close()
    assert not errs, errs
    for key, got in out.items():
        same(got, want[key[2]], f"thread {key}")


@pytest.mark.parametrize("fixed", (False, True))
def test_topk_on_arrow_int8_columns_equals_the_float64_columns(fixed):
    rs = np.random.RandomState(31)
    d, n = 48, 400
    qv = rs.randint(-128, 128, size=(9, d)).tolist()
    cv = rs.randint(-128, 128, size=(n, d)).tolist()
    cv[7][5] = None  # a null element reads as 0
    qv[2][0] = None
    t8 = pa.list_(pa.int8(), d) if fixed else pa.list_(pa.int8())
    t64 = pa.list_(pa.float64(), d) if fixed else pa.list_(pa.float64())
    clear_corpus_cache()
    for metric in ("cosine", "dot", "euclidean"):
        got = _topk(pa.array(qv, type=t8), pa.array(cv, type=t8), 10, metric)
        want = _topk(pa.array(qv, type=t64), pa.array(cv, type=t64), 10, metric)
        assert got.type == want.type
        assert got.equals(want), metric


def test_numpy_topk_takes_the_int8_route():
    import polars_matmul

    q, c = uniform(1000, 64, 41)
    got = polars_matmul.topk(q, c, 10, "cosine")
    same(got, polars_matmul.topk(q.astype(np.float64), c.astype(np.float64), 10, "cosine"), "numpy topk")


def _raw(fn, *args):
    rc = fn(*args)
    return rc, _native.last_error()


def test_refusals():
    L = _native.lib()
    q, c = uniform(100, 16, 51)
    idx, sc64, sc32 = np.empty((M, 5), np.uint32), np.empty((M, 5), np.float64), np.empty((M, 5), np.float32)
    i8 = _native.DeviceCorpus.int8(c)
    f32 = _native.DeviceCorpus(c.astype(np.float32))
    try:
        # an int8 handle at the other rows' entries, and the other way round: PMM_ERR_ARG naming the entry
        for name, qq, ss in (("pmm_topk_f32_corpus", q.astype(np.float32), sc32),
                             ("pmm_topk_f64_corpus", q.astype(np.float64), sc64),
                             ("pmm_topk_bf16_corpus", q.astype(np.float32), sc32)):
            rc, msg = _raw(getattr(L, name), i8._h, _native.ptr(qq), M, 5, COS, _native.ptr(idx), _native.ptr(ss))
            assert rc == _native.PMM_ERR_ARG and "int8 rows: use pmm_topk_i8_corpus" in msg, (name, rc, msg)
        rc, msg = _raw(L.pmm_topk_i8_corpus, f32._h, _native.ptr(q), M, 5, COS, _native.ptr(idx), _native.ptr(sc64))
        assert rc == _native.PMM_ERR_ARG and "f32 rows: use pmm_topk_f32_corpus" in msg, (rc, msg)
        # out of scope on an int8 handle: PMM_ERR_UNSUPPORTED
        out = ctypes.c_void_p()
        ids = np.array([0, 1], np.uint32)
        rc, msg = _raw(L.pmm_corpus_subset_ids, i8._h, _native.ptr(ids), 2, ctypes.byref(out))
        assert rc == _native.PMM_ERR_UNSUPPORTED and "int8" in msg and not out.value, (rc, msg)
        mask = np.full(16, 0xFF, np.uint8)
        rc, msg = _raw(L.pmm_corpus_subset_mask, i8._h, _native.ptr(mask), 0, ctypes.byref(out))
        assert rc == _native.PMM_ERR_UNSUPPORTED and "int8" in msg and not out.value, (rc, msg)
        labels = np.zeros(100, np.uint32)
        rc, msg = _raw(L.pmm_corpus_partition, i8._h, _native.ptr(labels), 1, ctypes.byref(out))
        assert rc == _native.PMM_ERR_UNSUPPORTED and "int8" in msg and not out.value, (rc, msg)
        total = ctypes.c_int64(0)
        offs = np.zeros(M + 1, np.int64)
        rc, msg = _raw(L.pmm_range_f32_corpus, i8._h, _native.ptr(q.astype(np.float32)), M, 0.5, COS, 0,
                       _native.ptr(offs), None, None, ctypes.byref(total))
        assert rc == _native.PMM_ERR_UNSUPPORTED and "int8" in msg, (rc, msg)
        # sizes: k > n is refused as pmm_topk_f64 refuses it; k = 0 and m = 0 return at once
        rc, msg = _raw(L.pmm_topk_i8, _native.ptr(q), M, _native.ptr(c), 100, 16, 101, COS, _native.ptr(idx),
                       _native.ptr(sc64))
        assert rc == _native.PMM_ERR_ARG and "must be <= n" in msg, (rc, msg)
        rc, msg = _raw(L.pmm_topk_i8_corpus, i8._h, _native.ptr(q), M, 101, COS, _native.ptr(idx), _native.ptr(sc64))
        assert rc == _native.PMM_ERR_ARG and "must be <= n" in msg, (rc, msg)
        assert L.pmm_topk_i8(_native.ptr(q), M, _native.ptr(c), 100, 16, 0, COS, None, None) == _native.PMM_OK
        assert L.pmm_topk_i8(None, 0, _native.ptr(c), 100, 16, 5, COS, None, None) == _native.PMM_OK
        assert L.pmm_topk_i8_corpus(i8._h, None, 0, 5, COS, None, None) == _native.PMM_OK
        rc, msg = _raw(L.pmm_topk_i8, _native.ptr(q), M, _native.ptr(c), 100, 16, 5, 7, _native.ptr(idx),
                       _native.ptr(sc64))
        assert rc == _native.PMM_ERR_ARG, (rc, msg)
        # d >= 2^16: PMM_ERR_UNSUPPORTED from the host entry and the creator
        wide = np.zeros((1, 65536), np.int8)
        rc, msg = _raw(L.pmm_topk_i8, _native.ptr(wide), 1, _native.ptr(wide), 1, 65536, 1, DOT, _native.ptr(idx),
                       _native.ptr(sc64))
        assert rc == _native.PMM_ERR_UNSUPPORTED and "d < 65536" in msg, (rc, msg)
        rc, msg = _raw(L.pmm_corpus_create_i8, _native.ptr(wide), 1, 65536, ctypes.byref(out))
        assert rc == _native.PMM_ERR_UNSUPPORTED and "d < 65536" in msg and not out.value, (rc, msg)
        # a misaligned device stride is refused before any launch
        rc, msg = _raw(L.pmm_topk_i8_device, 256, 16, M, 512, 16, 100, 16, 5, COS, 0, 1024, 2048, None, 0, None)
        assert rc == _native.PMM_ERR_ARG and "roundup(d, 64)" in msg, (rc, msg)
    finally:
        i8.close()
        f32.close()


def test_a_device_list_does_not_shard_int8_rows():
    q, c = uniform(1000, 64, 61)
    want = _native.topk_i8_host(q, c, 10, COS)
    _native.set_devices([0, 0])
    try:
        dc = _native.DeviceCorpus.int8(c)
        try:
            assert dc.shards == 1
            same(dc.topk(q, 10, COS), want, "handle under a device list")
        finally:
            dc.close()
        same(_native.topk_i8_host(q, c, 10, COS), want, "host entry under a device list")
    finally:
        _native.set_devices([])
