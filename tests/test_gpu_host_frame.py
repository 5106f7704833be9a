"""The host layer's shared paths on the GPU: the one sharded driver for f32,
bf16 and f64 rows (topk_sharded) and the one host-call frame (host_topk) that
every host entry and handle entry goes through.  A repeated device id drives
the multi-shard code on one GPU.  No tolerance in this file: indices and score
bits are equal."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import oracle
from polars_matmul import _native

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
METRICS = (COS, DOT, EUC)
BF16 = _native.COMPUTE_BF16


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want, label):
    assert got[0].shape == want[0].shape and got[1].dtype == want[1].dtype, label
    assert np.array_equal(got[0], want[0]), f"{label}: indices differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{label}: score bits differ"


@pytest.fixture
def device_list():
    yield
    _native.set_devices([])


# ---------------------------------------------------------------------------
# A shard shorter than k beside one that is not: n = 129 over [0, 0] gives
# shards of 64 and 65 rows, k = 65.  f32 and bf16 shards pad the short list with
# empty slots in the kernel; the f64 shard is searched for 64 entries into a
# compact list that is laid behind empty slots.
# ---------------------------------------------------------------------------
SHORT_M, SHORT_N, SHORT_D, SHORT_K = 33, 129, 40, 65


@pytest.mark.parametrize("kind", ["f32", "bf16", "f64 fused", "f64 materialised"])
def test_short_shard_beside_a_full_one(kind, device_list, monkeypatch):
    rs = np.random.RandomState(129)
    f64 = kind.startswith("f64")
    dt = np.float64 if f64 else np.float32
    q, c = rs.randn(SHORT_M, SHORT_D).astype(dt), rs.randn(SHORT_N, SHORT_D).astype(dt)
    c[70] = c[3]  # an exact tie across the shard boundary
    if f64:
        monkeypatch.setenv("PMM_F64_FUSED", "1" if kind == "f64 fused" else "0")
    compute = BF16 if kind == "bf16" else _native.COMPUTE_F32
    handle = (lambda: _native.DeviceCorpus(c, compute="bf16")) if kind == "bf16" else (lambda: _native.DeviceCorpus(c))
    one = handle()
    two = None
    try:
        for metric in METRICS:
            _native.set_devices([])
            want = _native.topk_host(q, c, SHORT_K, metric, compute)
            same(one.topk(q, SHORT_K, metric), want, f"{kind} one-shard handle metric={metric}")
            if kind != "bf16":
                oi, osc = oracle.topk(q, c, SHORT_K, metric)
                same(want, (np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(dt)), f"{kind} oracle metric={metric}")
            _native.set_devices([0, 0])
            same(_native.topk_host(q, c, SHORT_K, metric, compute), want, f"{kind} host entry, 2 shards metric={metric}")
            if two is None:
                two = handle()
                assert two.shards == 2 and one.shards == 1
            same(two.topk(q, SHORT_K, metric), want, f"{kind} sharded handle metric={metric}")
    finally:
        _native.set_devices([])
        one.close()
        if two is not None:
            two.close()


# ---------------------------------------------------------------------------
# The f64 deferred re-run under sharding: test_f64_fused_overflow_falls_back's
# construction (every corpus row beats every earlier one).  k = 10 has a
# 1024-entry buffer; a shard's first chunk is 512 columns and its second would
# be 15 times that, every one a survivor, so a shard of 2000 rows overflows.
# The flags are read once both shards have run; both re-run materialised.
# ---------------------------------------------------------------------------
def test_f64_overflowed_shards_rerun_after_every_device(device_list, monkeypatch):
    monkeypatch.setenv("PMM_F64_FUSED", "1")
    n, d, k = 4000, 16, 10
    q = np.ones((4, d))
    c = np.repeat(np.arange(n, dtype=np.float64)[:, None], d, axis=1) / n
    want = _native.topk_host(q, c, k, DOT)
    assert want[0].tolist() == [list(range(n - 1, n - 1 - k, -1))] * 4
    _native.set_devices([0, 0])
    _native.timing_reset()
    _native.timing_enable(True)
    try:
        got = _native.topk_host(q, c, k, DOT)
        fused, rerun = _native.timing_read("gemm_f64_topk")[1], _native.timing_read("gemm_f64_scores")[1]
        merges = _native.timing_read("merge_devices_f64")[1]
    finally:
        _native.timing_enable(False)
        _native.timing_reset()
    assert fused >= 4 and rerun == 2 and merges == 1, (fused, rerun, merges)
    same(got, want, "sharded f64 overflow re-run")


# ---------------------------------------------------------------------------
# An int8 handle through the shared handle path.  H2D / D2H: launch counts of
# the call on the build before the shared path (the queries, padded, in one
# timed upload; both lists in one timed download).
# ---------------------------------------------------------------------------
I8_HANDLE_H2D, I8_HANDLE_D2H = 1, 1


@pytest.mark.parametrize("metric", METRICS)
def test_int8_handle_through_the_shared_path(metric):
    rs = np.random.RandomState(300 + metric)
    m, n, d, k = 17, 300, 70, 10
    q = rs.randint(-128, 128, size=(m, d)).astype(np.int8)
    c = rs.randint(-128, 128, size=(n, d)).astype(np.int8)
    dc = _native.DeviceCorpus.int8(c)
    _native.timing_reset()
    _native.timing_enable(True)
    try:
        got = dc.topk(q, k, metric)
        h2d, d2h = _native.timing_read("h2d")[1], _native.timing_read("d2h")[1]
    finally:
        _native.timing_enable(False)
        _native.timing_reset()
        dc.close()
    assert (h2d, d2h) == (I8_HANDLE_H2D, I8_HANDLE_D2H)
    same(got, _native.topk_i8_host(q, c, k, metric), f"int8 handle vs host entry metric={metric}")
    same(got, _native.topk_host(q.astype(np.float64), c.astype(np.float64), k, metric), f"int8 handle vs f64 metric={metric}")


def test_int8_entry_refuses_partitioned_and_other_handles():
    L = _native.lib()
    rs = np.random.RandomState(7)
    c = rs.randn(100, 16).astype(np.float32)
    q = rs.randint(-128, 128, size=(5, 16)).astype(np.int8)
    idx, sc = np.empty((5, 3), np.uint32), np.empty((5, 3), np.float64)
    f32 = _native.DeviceCorpus(c)
    part = f32.partition(np.arange(100, dtype=np.uint32) % 4, 4)
    try:
        call = lambda h: (L.pmm_topk_i8_corpus(h._h, _native.ptr(q), 5, 3, COS, _native.ptr(idx), _native.ptr(sc)),
                          _native.last_error())
        rc, msg = call(part)
        assert rc == _native.PMM_ERR_ARG and msg.startswith("the corpus handle is partitioned (pmm_corpus_partition)"), msg
        assert msg.endswith("use pmm_topk_f32_grouped"), msg
        rc, msg = call(f32)
        assert rc == _native.PMM_ERR_ARG and msg == "the corpus handle holds f32 rows: use pmm_topk_f32_corpus", msg
    finally:
        part.close()
        f32.close()
