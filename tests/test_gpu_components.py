"""Duplicate groups on resident corpus handles (pmm_components_f32_self,
``DeviceCorpus.components_self``, ``duplicate_groups``): the connected
components of the self range search's pairs, every row labelled with the
smallest row of its component.

The truth everywhere is the oracle's ranked list of the column against itself,
cut at the threshold above the diagonal (tests/self_cases.py), joined by a
plain union-find (tests/components_cases.py).  Labels and counts must be equal;
there are no tolerances in this file.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import pytest

from components_cases import CHAIN_THRESHOLD, chain_column, components_truth
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm
from self_cases import COS, DOT, EUC, NAME, f32, ragged_column, range_self_truth, ranked_self

pytestmark = pytest.mark.gpu

INF = float("inf")
METRICS = [COS, DOT, EUC]


def everything(metric):
    """The threshold every finite score passes."""
    return INF if metric == EUC else -INF


def edge_threshold(full, metric, edges):
    """The threshold that the ``edges`` best pairs (i, j > i) pass -- more on ties."""
    s = np.sort(range_self_truth(full, everything(metric), metric)[2])
    return float(s[edges - 1] if metric == EUC else s[s.size - edges])


def assert_same(got, want, label):
    labels, components, pairs = got
    assert labels.dtype == np.uint32 and labels.shape == want[0].shape, label
    assert np.array_equal(labels, want[0]), f"{label}: labels differ at {np.flatnonzero(labels != want[0])[:10]}"
    assert (components, pairs) == (want[1], want[2]), f"{label}: (components, pairs) {(components, pairs)}, " \
                                                      f"wanted {want[1:]}"


def ccomponents(dc, threshold, metric, labels, components=True, pairs=True):
    """The C entry as it is: (rc, components, pairs)."""
    nc, npairs = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _native.lib().pmm_components_f32_self(dc._h, threshold, metric, None if labels is None else _native.ptr(labels),
                                               ctypes.byref(nc) if components else None,
                                               ctypes.byref(npairs) if pairs else None)
    return rc, nc.value, npairs.value


@pytest.fixture(scope="module")
def ragged():
    """Case 1 (n = 300, d = 37): per metric the column, a threshold that about
    120 pairs pass and the truth at it."""
    out = {}
    for metric in METRICS:
        c = ragged_column(metric)
        full = ranked_self(c, metric)
        t = edge_threshold(full, metric, 120)
        out[metric] = (c, full, t, components_truth(full, t, metric))
    return out


# ---- 1. ragged in every dimension, a sparse graph of small components ----
@pytest.mark.parametrize("metric", METRICS)
def test_ragged_shape(ragged, metric):
    c, full, t, want = ragged[metric]
    sizes = np.bincount(want[0], minlength=c.shape[0])
    assert sizes.max() >= 3 and (sizes > 1).sum() >= 2 and (sizes == 1).sum() >= 20, sizes[sizes > 0]
    assert want[1] == (sizes > 0).sum() and want[2] >= 120
    dc = _native.DeviceCorpus(c)
    try:
        got = dc.components_self(t, metric)
        assert_same(got, want, NAME[metric])
        assert got[2] == int(dc.range_self(t, metric)[0][-1])  # the range entry's own total
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
        out[metric] = (t, components_truth(full, t, metric))
    return c, out


def test_diagonal_tiles_under_every_variant(diagonal_case, monkeypatch):
    c, cases = diagonal_case
    got = {}
    for variant in (0, 3):
        monkeypatch.setenv("PMM_GEMM_VARIANT", str(variant))
        dc = _native.DeviceCorpus(c)
        try:
            for metric in METRICS:
                t, want = cases[metric]
                assert want[2] > 0
                got[variant, metric] = dc.components_self(t, metric)
                assert_same(got[variant, metric], want, f"variant {variant} {NAME[metric]}")
        finally:
            dc.close()
    for metric in METRICS:
        assert np.array_equal(got[0, metric][0], got[3, metric][0]) and got[0, metric][1:] == got[3, metric][1:]


# ---- 3. chains: a component held together only by all of its links ----
def test_chains():
    n, d = 600, 16
    c, chains, isolated = chain_column(n, d, 1)
    dc = _native.DeviceCorpus(c)
    try:
        labels, components, pairs = dc.components_self(CHAIN_THRESHOLD, EUC)
    finally:
        dc.close()
    for r in chains:
        assert (labels[r] == r.min()).all(), (len(r), np.unique(labels[r]))  # one label, the smallest row
    assert len({int(labels[r[0]]) for r in chains}) == len(chains)  # no two chains merged
    assert np.array_equal(labels[isolated], isolated)
    assert components == len(chains) + isolated.size and pairs == sum(len(r) - 1 for r in chains)
    assert_same((labels, components, pairs), components_truth(ranked_self(c, EUC), CHAIN_THRESHOLD, EUC), "truth")


# ---- 4. everything hits, nothing hits ----
@pytest.mark.parametrize("n", [1, 2, 130])
def test_extremes(n):
    c = f32(np.random.RandomState(30 + n).randn(n, 8))
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            labels, components, pairs = dc.components_self(everything(metric), metric)
            assert labels.dtype == np.uint32 and not labels.any() and labels.shape == (n,), NAME[metric]
            assert (components, pairs) == (1, n * (n - 1) // 2), NAME[metric]
        labels, components, pairs = dc.components_self(2.0, COS)  # no cosine reaches 2
        assert np.array_equal(labels, np.arange(n, dtype=np.uint32)) and (components, pairs) == (n, 0)
    finally:
        dc.close()


# ---- 5. one heavy group: every hit contends for one root ----
def test_one_heavy_group():
    n, d, copies = 2048, 8, 1500
    rs = np.random.RandomState(12)
    c = f32(rs.randn(n, d))
    rows = np.sort(rs.permutation(n)[:copies])
    c[rows] = 6.0  # the copied row: (6, .., 6), its dot product with itself 288
    dc = _native.DeviceCorpus(c)
    try:
        for metric, t in ((COS, 0.99), (DOT, 250.0)):
            want = components_truth(ranked_self(c, metric), t, metric)
            got = dc.components_self(t, metric)
            again = dc.components_self(t, metric)
            assert (got[0][rows] == rows[0]).all(), NAME[metric]  # the first copy's number
            assert got[2] >= copies * (copies - 1) // 2
            if metric == DOT:  # only the copies pass
                assert got[2] == copies * (copies - 1) // 2 and got[1] == n - copies + 1
            assert_same(got, want, NAME[metric])
            assert_same(again, want, NAME[metric] + " again")
    finally:
        dc.close()


# ---- 6. a derived handle reports the parent's row numbers ----
@pytest.mark.parametrize("metric", METRICS)
def test_derived_handle(metric):
    n, d, s = 700, 37, 300
    rs = np.random.RandomState(81 + metric)
    c = f32(rs.randn(n, d))
    sel = np.sort(rs.permutation(n)[:s]).astype(np.uint32)
    assert (np.diff(sel.astype(np.int64)) > 1).sum() > 50  # scattered: not the parent's own numbering
    full = ranked_self(f32(c[sel]), metric)
    t = edge_threshold(full, metric, 150)
    want = components_truth(full, t, metric, ids=sel)
    assert (np.bincount(components_truth(full, t, metric)[0]) > 1).any()
    dc = _native.DeviceCorpus(c)
    try:
        sub = dc.subset(sel)
        try:
            assert_same(sub.components_self(t, metric), want, NAME[metric])
        finally:
            sub.close()
        one = dc.subset(sel[5:6])  # n = 1: the row's parent number
        try:
            labels, components, pairs = one.components_self(t, metric)
            assert labels.tolist() == [int(sel[5])] and (components, pairs) == (1, 0)
        finally:
            one.close()
    finally:
        dc.close()


# ---- 7. NaN, infinite and zero-norm rows ----
@pytest.mark.parametrize("metric", [COS, EUC])
def test_special_rows(metric):
    n, d = 200, 24
    rs = np.random.RandomState(44)
    c = f32(rs.randn(n, d))
    c[[7, 90, 150]] = 0.0                 # zero norm (and copies of each other)
    c[20, 3] = c[131, 0] = np.nan
    c[33, 1] = c[34, 1] = np.inf
    c[60, 2] = -np.inf
    c[[101, 102]] = c[100]                # exact copies
    c[140] = -c[100]
    c[199] = 1e-30 * c[198]               # a subnormal-scale row
    full = ranked_self(c, metric)
    # (the oracle's scores decide what a special row is to the others: cosine has
    # NaN scores here, the infinite rows'; euclidean has infinite distances)
    above = full[0].astype(np.int64) > np.arange(n)[:, None]
    nan_pairs = int((np.isnan(full[1]) & above).sum())
    assert nan_pairs > 0 if metric == COS else np.isinf(full[1]).any()
    dc = _native.DeviceCorpus(c)
    try:
        finite = range_self_truth(full, everything(metric), metric)[2]
        for t in (edge_threshold(full, metric, 100), 0.0, -0.0, everything(metric)):
            want = components_truth(full, t, metric)
            got = dc.components_self(t, metric)
            assert_same(got, want, f"{NAME[metric]} threshold {t}")
        # a NaN score joins nothing: at the threshold every other score passes,
        # the pairs are all but the NaN ones
        assert got[2] == n * (n - 1) // 2 - nan_pairs == finite.size
    finally:
        dc.close()


# ---- 8. dirty scratch: parent[] is initialised by the call itself ----
@pytest.mark.parametrize("poison", ["0x00", "0xFF"])
def test_poisoned_scratch(ragged, poison, monkeypatch):
    for metric in METRICS:
        c, _, t, want = ragged[metric]
        dc = _native.DeviceCorpus(c)
        try:
            monkeypatch.delenv("PMM_ARENA_POISON", raising=False)
            plain = dc.components_self(t, metric)
            monkeypatch.setenv("PMM_ARENA_POISON", poison)
            assert_same(dc.components_self(t, metric), plain, f"poison {poison} {NAME[metric]}")
            assert_same(plain, want, NAME[metric])
        finally:
            dc.close()


# ---- 9. the C entry as it is ----
def test_refused_handles_and_arguments():
    n, d = 300, 37
    c = f32(np.random.RandomState(9).randn(n, d))
    dc = _native.DeviceCorpus(c)
    part = dc.partition(np.arange(n, dtype=np.uint32) % 3, 3)
    d64 = _native.DeviceCorpus(c.astype(np.float64))
    b16 = _native.DeviceCorpus(c, compute="bf16")
    i8 = _native.DeviceCorpus.int8(np.clip(c * 40, -127, 127).astype(np.int8))
    one = _native.DeviceCorpus(c[:1])
    labels = np.full(n, 0xDEADBEEF, np.uint32)
    try:
        for h, code, word in ((part, _native.PMM_ERR_ARG, "partitioned"), (d64, _native.PMM_ERR_ARG, "f32 handle"),
                              (b16, _native.PMM_ERR_ARG, "f32 handle"),
                              (i8, _native.PMM_ERR_UNSUPPORTED, "f32 handle")):
            rc, _, _ = ccomponents(h, 0.5, COS, labels)
            assert rc == code and word in _native.last_error(), _native.last_error()
            assert "self search" in _native.last_error() or word == "partitioned"
        with pytest.raises(_native.PmmError) as ei:
            part.components_self(0.5, COS)
        assert ei.value.code == _native.PMM_ERR_ARG
        rc, _, _ = ccomponents(dc, float("nan"), COS, labels)
        assert rc == _native.PMM_ERR_ARG and "NaN" in _native.last_error()
        assert ccomponents(dc, 0.5, 3, labels)[0] == _native.PMM_ERR_ARG
        assert ccomponents(dc, 0.5, COS, None) == (_native.PMM_ERR_ARG, -7, -7)  # (the counts untouched too)
        assert ccomponents(dc, 0.5, COS, labels, components=False)[0] == _native.PMM_ERR_ARG
        assert ccomponents(dc, 0.5, COS, labels, pairs=False)[0] == _native.PMM_ERR_ARG
        assert (labels == 0xDEADBEEF).all()  # a refused call writes nothing
        rc, components, pairs = ccomponents(one, 0.5, COS, labels)
        assert rc == _native.PMM_OK and labels[0] == 0 and (components, pairs) == (1, 0)
        assert (labels[1:] == 0xDEADBEEF).all()
    finally:
        for h in (part, d64, b16, i8, one, dc):
            h.close()
    _native.set_devices([0, 0])
    try:
        sharded = _native.DeviceCorpus(c)
        try:
            assert sharded.shards == 2
            rc, _, _ = ccomponents(sharded, 0.5, COS, labels)
            assert rc == _native.PMM_ERR_UNSUPPORTED and "self search" in _native.last_error()
        finally:
            sharded.close()
    finally:
        _native.set_devices([])


# ---- 10. the public entries ----
def test_public_entries_equal_the_handle(ragged, monkeypatch):
    import pyarrow as pa

    import polars_matmul

    c, _, t, want = ragged[COS]
    dc = _native.DeviceCorpus(c)
    try:
        hl = dc.components_self(t, COS)[0]
    finally:
        dc.close()
    assert np.array_equal(hl, want[0])
    created = []

    class Counting(_native.DeviceCorpus):
        def __init__(self, *a, **k):
            created.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(_native, "DeviceCorpus", Counting)
    monkeypatch.setattr(pm, "_CACHE_ON", True)
    monkeypatch.setattr(pm, "_CACHE_MIN_BYTES", 0)  # (the column is small: cache it all the same)
    pm.clear_corpus_cache()
    try:
        col = pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1)), c.shape[1])
        arr = pm._duplicate_groups(col, t, "cosine")
        assert arr.type == pa.uint32() and len(arr) == c.shape[0] and arr.null_count == 0
        assert np.array_equal(arr.to_numpy(), hl)
        again = pm._duplicate_groups(col, t, "cosine")
        assert np.array_equal(again.to_numpy(), hl)
        assert len(created) == 1, "the second call made a second handle"
        labels = polars_matmul.duplicate_groups(c, t)
        assert labels.dtype == np.uint32 and np.array_equal(labels, hl)
        assert np.array_equal(polars_matmul.duplicate_groups(c, t, "cosine", compute="f32"), hl)
    finally:
        pm.clear_corpus_cache()


# ---- 11. two threads on one handle ----
def test_two_threads_one_handle(ragged):
    c = ragged[COS][0]
    full = {m: ranked_self(c, m) for m in (COS, EUC)}
    jobs = [(COS, ragged[COS][2]), (EUC, edge_threshold(full[EUC], EUC, 200))]
    dc = _native.DeviceCorpus(c)
    try:
        serial = [dc.components_self(t, m) for m, t in jobs]
        assert serial[0][2] != serial[1][2]
        results, errors = [[], []], []

        def work(i):
            try:
                for _ in range(3):
                    results[i].append(dc.components_self(jobs[i][1], jobs[i][0]))
            except BaseException as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for i in range(2):
            assert len(results[i]) == 3
            for r in results[i]:
                assert_same(r, serial[i], f"thread {i}")
            assert_same(serial[i], components_truth(full[jobs[i][0]], jobs[i][1], jobs[i][0]), f"serial {i}")
    finally:
        dc.close()
