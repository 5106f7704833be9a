"""What a corpus handle (pmm_corpus_*) does per call, pinned at the C ABI for
the three row types: the bytes it reports, its lists against the host entry's
on the same arrays, the refusal of a handle of another row type, and the copies
and launches a creation and a call record.

The shapes pad under every rule (d = 33 -> 64 floats, 48 doubles, 128 bf16) and
are ragged against every tile.  "Equal" is np.array_equal on the indices and on
the scores' bits; there are no tolerances in this file.  The launch counts are
literals: what the library recorded before the handle code was folded into one
creator and one call path.
"""
from __future__ import annotations

import numpy as np
import pytest

from polars_matmul import _native

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
METRICS = (COS, DOT, EUC)
KINDS = ("f32", "f64", "bf16")
N, D, M, K = 130, 33, 3, 5
IDS = np.array([0, 3, 64, 65, 100, 128, 129], np.uint32)  # 7 ascending rows, both ends among them
TIMED = ("h2d", "round_norms_bf16", "remap_index", "d2h")

ENTRY = {"f32": "pmm_topk_f32_corpus", "f64": "pmm_topk_f64_corpus", "bf16": "pmm_topk_bf16_corpus"}


def arrays(kind, n, seed):
    """(q, c) in the dtype the kind's entries take."""
    rs = np.random.RandomState(seed)
    dt = np.float64 if kind == "f64" else np.float32
    return np.ascontiguousarray(rs.randn(M, D), dt), np.ascontiguousarray(rs.randn(n, D), dt)


def corpus(kind, c):
    return _native.DeviceCorpus(c, compute="bf16" if kind == "bf16" else "f32")


def host(kind, q, c, k, metric):
    return _native.topk_host(q, c, k, metric, _native.COMPUTE_BF16 if kind == "bf16" else _native.COMPUTE_F32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_lists(got, want, label):
    assert got[0].shape == want[0].shape and got[1].dtype == want[1].dtype, label
    assert np.array_equal(got[0], want[0]), f"{label}: indices differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{label}: score bits differ"


@pytest.fixture(scope="module")
def host_lists():
    """The host entry's lists with no device list, per (kind, metric): computed once."""
    assert _native.get_devices() == []
    out = {}
    for kind in KINDS:
        q, c = arrays(kind, N, 7)
        for metric in METRICS:
            out[kind, metric] = host(kind, q, c, K, metric)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_bytes_plain_sharded_subset(kind):
    _, c = arrays(kind, N, 7)
    want = _native.corpus_device_bytes(N, D, c.dtype, "bf16" if kind == "bf16" else "f32")
    one = corpus(kind, c)
    try:
        assert one.shards == 1 and one.nbytes == want
        sub = one.subset(IDS)
        try:
            assert sub.n == IDS.size
            assert sub.nbytes == _native.subset_device_bytes(IDS.size, D, c.dtype, "bf16" if kind == "bf16" else "f32")
        finally:
            sub.close()
    finally:
        one.close()
    try:
        _native.set_devices([0, 0, 0])
        three = corpus(kind, c)
        try:
            assert three.shards == 3 and three.nbytes == want
        finally:
            three.close()
    finally:
        _native.set_devices([])


@pytest.mark.parametrize("kind", KINDS)
def test_lists_equal_host_entry(kind, host_lists):
    q, c = arrays(kind, N, 7)
    one = corpus(kind, c)
    try:
        for metric in METRICS:
            assert_same_lists(one.topk(q, K, metric), host_lists[kind, metric], f"{kind} metric {metric}")
    finally:
        one.close()


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_lists_equal_host_entry(kind, host_lists):
    q, c = arrays(kind, N, 7)
    try:
        _native.set_devices([0, 0, 0])
        three = corpus(kind, c)
        try:
            assert three.shards == 3
            for metric in METRICS:
                assert_same_lists(three.topk(q, K, metric), host_lists[kind, metric], f"{kind} x3 metric {metric}")
        finally:
            three.close()
    finally:
        _native.set_devices([])


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_shards_shorter_than_k(kind):
    # 7 rows over [0, 0, 0]: shards of 2, 2 and 3 rows, two of them shorter than
    # k = 3 (f64: the padded short-list path)
    n, k = 7, 3
    q, c = arrays(kind, n, 9)
    want = {metric: host(kind, q, c, k, metric) for metric in METRICS}
    try:
        _native.set_devices([0, 0, 0])
        three = corpus(kind, c)
        try:
            assert three.shards == 3
            for metric in METRICS:
                assert_same_lists(three.topk(q, k, metric), want[metric], f"{kind} short shards metric {metric}")
        finally:
            three.close()
    finally:
        _native.set_devices([])


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_handle_names_its_entry(kind):
    q, c = arrays(kind, N, 7)
    lib = _native.lib()
    h = corpus(kind, c)
    try:
        for other in KINDS:
            if other == kind:
                continue
            qo = np.zeros((M, D), np.float64 if other == "f64" else np.float32)
            idx = np.empty((M, K), np.uint32)
            sc = np.empty((M, K), qo.dtype)
            rc = getattr(lib, ENTRY[other])(h._h, _native.ptr(qo), M, K, COS, _native.ptr(idx), _native.ptr(sc))
            assert rc == _native.PMM_ERR_ARG, (kind, other, rc)
            assert _native.last_error() == f"the corpus handle holds {kind} rows: use {ENTRY[kind]}", (kind, other)
    finally:
        h.close()


def counts(fn):
    """fn()'s result and the launches it recorded under each TIMED name."""
    _native.timing_enable(True)
    _native.timing_reset()
    try:
        out = fn()
        got = {name: _native.timing_read(name)[1] for name in TIMED}
    finally:
        _native.timing_reset()
        _native.timing_enable(False)
    return out, got


def timed(h2d=0, round_norms_bf16=0, remap_index=0, d2h=0):
    return {"h2d": h2d, "round_norms_bf16": round_norms_bf16, "remap_index": remap_index, "d2h": d2h}


# (creation, call on the handle, derivation by ids, call on the derived handle)
LAUNCHES = {
    "f32": (timed(h2d=1), timed(h2d=1, d2h=1), timed(h2d=1), timed(h2d=1, remap_index=1, d2h=1)),
    "f64": (timed(h2d=1), timed(h2d=1, d2h=1), timed(h2d=1), timed(h2d=1, remap_index=1, d2h=1)),
    "bf16": (timed(h2d=1, round_norms_bf16=1), timed(h2d=1, round_norms_bf16=1, d2h=1), timed(h2d=1),
             timed(h2d=1, round_norms_bf16=1, remap_index=1, d2h=1)),
}


@pytest.mark.parametrize("kind", KINDS)
def test_launch_counts(kind):
    q, c = arrays(kind, N, 7)
    create, call, derive, subcall = LAUNCHES[kind]
    one, got = counts(lambda: corpus(kind, c))
    try:
        print(kind, "create", got)
        assert got == create, ("create", got)
        _, got = counts(lambda: one.topk(q, K, COS))
        print(kind, "call", got)
        assert got == call, ("call", got)
        sub, got = counts(lambda: one.subset(IDS))
        try:
            print(kind, "derive", got)
            assert got == derive, ("derive", got)
            _, got = counts(lambda: sub.topk(q, K, COS))
            print(kind, "derived call", got)
            assert got == subcall, ("derived call", got)
        finally:
            sub.close()
    finally:
        one.close()
