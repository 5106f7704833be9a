"""Probed search on partitioned corpus handles (``DeviceCorpus.topk_probed``,
pmm_topk_f32_probed) and ``groups=`` with a list of labels per query row.

The truth for query row i is ``oracle.topk(q[i], c[ids_i])`` with ``ids_i``
the ascending corpus rows of every group the row probes, its indices mapped
through ``ids_i``; "exact" is equality of every index and of every score's
bits (the sign of a zero included).  There are no tolerances in this file.
"""
from __future__ import annotations

import numpy as np
import pyarrow as pa
import pytest

import oracle
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm
from value_cases import value_case

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
NONE = _native.NO_GROUP


def same_bits(a, b, dtype=np.float32):
    a, b = np.ascontiguousarray(a, dtype), np.ascontiguousarray(b, dtype)
    u = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def flat(probes):
    """(offsets int64, labels uint32) of a list of per-row label lists."""
    po = np.concatenate([[0], np.cumsum([len(p) for p in probes])]).astype(np.int64)
    return po, np.array([x for p in probes for x in p], dtype=np.uint32)


def truth(q, c, probes, cl, k, metric):
    """Per query row: (indices in c's numbering, scores) of the oracle on the union of the row's groups."""
    lists = []
    for i, p in enumerate(probes):
        ids = np.flatnonzero(np.isin(cl, [x for x in p if x != NONE]) & (cl != NONE))
        if ids.size == 0:
            lists.append((np.zeros(0, np.uint32), np.zeros(0, c.dtype)))
            continue
        oi, osc = oracle.topk(np.ascontiguousarray(q[i:i + 1]), np.ascontiguousarray(c[ids]), min(k, ids.size),
                              ORACLE_METRIC[metric])
        lists.append((ids[np.asarray(oi).astype(np.int64)[0]].astype(np.uint32), np.asarray(osc)[0]))
    return lists


def assert_exact(got, want, k, label):
    idx, sc, lens = got
    assert idx.shape == sc.shape == (len(want), k) and lens.shape == (len(want),), label
    for r, (wi, ws) in enumerate(want):
        n = wi.size
        assert lens[r] == n, f"{label}: row {r} length {lens[r]} != {n}"
        assert np.array_equal(idx[r, :n], wi), f"{label}: row {r} indices {idx[r, :n]} != {wi}"
        assert same_bits(sc[r, :n], ws), f"{label}: row {r} score bits differ"
        assert np.all(idx[r, n:] == 0xFFFFFFFF) and not np.any(sc[r, n:].view(np.uint8)), f"{label}: row {r} padding"


def timed(call):
    """(result, probed_topk_f32 launches, probe_merge launches) of call()."""
    _native.timing_enable(True)
    _native.timing_reset()
    try:
        got = call()
        return got, _native.timing_read("probed_topk_f32")[1], _native.timing_read("probe_merge")[1]
    finally:
        _native.timing_enable(False)


def main_shape(d, seed):
    """tests/test_gpu_grouped.py's corpus, restated: n = 1237, eight labels
    with segments of 1, 7, 255, 256, 257, 300 and 151 rows, label 7 without
    corpus rows, ten rows in no group.  m = 37 queries with probe lists of
    0, 1, 2, 3 and 8 labels: 19 rows probe group 5 (two work units), one list
    repeats a label, two hold the none label, three name the empty label 7
    and the union of [0, 1] (8 rows) is shorter than k = 10."""
    m, n = 37, 1237
    rs = np.random.RandomState(seed)
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    sizes = [1, 7, 255, 256, 257, 300]
    cl = np.concatenate([np.full(s, g) for g, s in enumerate(sizes)] + [np.full(10, NONE)]
                        + [np.full(n - sum(sizes) - 10, 6)]).astype(np.uint32)
    rs.shuffle(cl)
    probes = [[5] for _ in range(5)] + [[5, r % 5] for r in range(5, 11)] + [[r % 4, 5, 6] for r in range(11, 17)]
    probes += [[], [0, 1], [3, 3, 2], [NONE, 4], [7], [7, 2], list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [NONE]]
    probes += [rs.randint(0, 8, size=rs.randint(1, 4)).tolist() for _ in range(m - len(probes))]
    assert len(probes) == m and sum(5 in p for p in probes) >= 17
    return q, c, probes, cl


@pytest.fixture(scope="module")
def main_case():
    q, c, probes, cl = main_shape(37, 7)
    want = {(metric, k): truth(q, c, probes, cl, k, metric) for metric in (COS, DOT, EUC) for k in (1, 10, 128)}
    return q, c, probes, cl, want


# ---- 1. the main shape: three metrics, three k, both paths ----
@pytest.mark.parametrize("metric", [COS, DOT, EUC])
def test_main_shape_kernel_and_loop(monkeypatch, main_case, metric):
    q, c, probes, cl, want = main_case
    po, pl = flat(probes)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            for path in ("kernel", "loop"):
                monkeypatch.setenv("PMM_GROUPED", path)
                for k in (1, 10, 128):
                    got, kernel, merge = timed(lambda: part.topk_probed(q, po, pl, k, metric))
                    assert kernel == (1 if path == "kernel" else 0) and merge == 1, (path, k, kernel, merge)
                    assert_exact(got, want[(metric, k)], k, f"{NAME[metric]} {path} k={k}")
                    if k == 10:
                        assert got[2][17] == 0 and got[2][18] == 8 and got[2][21] == 0 and got[2][25] == 0
        finally:
            part.close()
    finally:
        dc.close()


# ---- 2. PMM_ARENA_POISON: the workspace may hold anything ----
def test_main_shape_on_a_poisoned_arena(monkeypatch, main_case):
    q, c, probes, cl, want = main_case
    po, pl = flat(probes)
    monkeypatch.delenv("PMM_GROUPED", raising=False)
    monkeypatch.setenv("PMM_GROUPED_SEG_MAX", "256")  # segments of 257 and 300 rows take the loop in the same call
    monkeypatch.setenv("PMM_ARENA_POISON", "0xFF")
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            got, kernel, merge = timed(lambda: part.topk_probed(q, po, pl, 10, COS))
            assert kernel == 1 and merge == 1
            assert_exact(got, want[(COS, 10)], 10, "poisoned arena, both paths in one call")
        finally:
            part.close()
    finally:
        dc.close()


# ---- 3. ties across groups go to the lower PARENT row ----
@pytest.mark.parametrize("path", ["kernel", "loop"])
def test_ties_across_groups_break_by_parent_row(monkeypatch, path):
    n, d = 700, 40
    rs = np.random.RandomState(31)
    c = rs.randn(n, d).astype(np.float32)
    cl = np.where(np.arange(n) < 100, 1, 0).astype(np.uint32)  # rows 0..99 in group 1: partition order reverses
    c[500] = c[10]            # parent 10 (group 1) ties with parent 500 (group 0, the lower partition row)
    c[300] = c[600] = c[20]   # parent 20 (group 1) with 300 and 600 (group 0)
    q = np.ascontiguousarray(np.stack([c[10], c[20], rs.randn(d).astype(np.float32)]))
    probes = [[0, 1], [1, 0], [0, 1]]
    po, pl = flat(probes)
    monkeypatch.setenv("PMM_GROUPED", path)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 2)
        try:
            for metric in (COS, DOT, EUC):
                for k in (1, 2, 3, 4):
                    got = part.topk_probed(q, po, pl, k, metric)
                    assert_exact(got, truth(q, c, probes, cl, k, metric), k, f"{NAME[metric]} k={k}")
                    if metric in (COS, EUC):
                        assert got[0][0, :2].tolist() == [10, 500][:k], got[0][0]
                        assert got[0][1, :3].tolist() == [20, 300, 600][:k], got[0][1]
        finally:
            part.close()
    finally:
        dc.close()


# ---- 4. equivalences, bit for bit ----
def test_one_probe_per_row_equals_topk_grouped(monkeypatch):
    q, c, _, cl = main_shape(37, 11)
    rs = np.random.RandomState(12)
    ql = rs.randint(0, 8, size=q.shape[0]).astype(np.uint32)
    ql[::9] = NONE
    po, pl = flat([[x] for x in ql])
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            for path in ("kernel", "loop"):
                monkeypatch.setenv("PMM_GROUPED", path)
                for metric in (COS, DOT, EUC):
                    gi, gs, gl = part.topk_grouped(q, ql, 10, metric)
                    pi, ps, plen = part.topk_probed(q, po, pl, 10, metric)
                    assert np.array_equal(gi, pi) and np.array_equal(gl, plen), (path, metric)
                    assert np.array_equal(gs.view(np.uint32), ps.view(np.uint32)), (path, metric)
        finally:
            part.close()
    finally:
        dc.close()


def test_probing_every_group_equals_the_ungrouped_search(monkeypatch):
    m, n, d = 19, 1237, 37
    rs = np.random.RandomState(13)
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    c[700] = c[3]
    q[0] = c[3]
    cl = rs.randint(0, 8, size=n).astype(np.uint32)  # no row dropped
    po, pl = flat([list(range(8))] * m)
    monkeypatch.delenv("PMM_GROUPED", raising=False)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            for metric in (COS, DOT, EUC):
                for k in (10, 128):
                    wi, ws = dc.topk(q, k, metric)
                    pi, ps, plen = part.topk_probed(q, po, pl, k, metric)
                    assert np.all(plen == k) and np.array_equal(wi, pi), (metric, k)
                    assert np.array_equal(ws.view(np.uint32), ps.view(np.uint32)), (metric, k)
        finally:
            part.close()
    finally:
        dc.close()


# ---- 5. signed zeros, zero rows, NaN and infinite rows, spread over the groups ----
@pytest.mark.parametrize("case", ["signed_zero", "nonfinite"])
@pytest.mark.parametrize("path", ["kernel", "loop"])
def test_zero_and_nan_scores(monkeypatch, case, path):
    m, n, d, k = 5, 300, 37, 128
    q, c = value_case(case, np.float32, m, n, d)
    cl = (np.arange(n) % 3).astype(np.uint32)  # the planted rows fall in all three groups
    probes = [[0, 1], [1, 2], [0, 1, 2], [2], [2, 0]]
    po, pl = flat(probes)
    monkeypatch.setenv("PMM_GROUPED", path)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 3)
        try:
            for metric in (COS, DOT):
                want = truth(q, c, probes, cl, k, metric)
                if case == "signed_zero":  # (the case is in the lists: zeros of both signs)
                    z = np.concatenate([ws[ws == 0] for _, ws in want])
                    assert np.signbit(z).any() and not np.signbit(z).all(), "no zero of each sign in the truth"
                assert_exact(part.topk_probed(q, po, pl, k, metric), want, k, f"{case} {NAME[metric]} {path}")
        finally:
            part.close()
    finally:
        dc.close()


# ---- 6. the kernel's widest row, and the first width past it ----
@pytest.mark.parametrize("d,launches", [(1024, 1), (1025, 0)])
def test_width_at_and_past_the_kernel_limit(monkeypatch, d, launches):
    m, n, k = 5, 300, 10
    rs = np.random.RandomState(d)
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    cl = (np.arange(n) % 3).astype(np.uint32)
    probes = [[0, 1], [1, 2], [0, 1, 2], [2], []]
    po, pl = flat(probes)
    monkeypatch.delenv("PMM_GROUPED", raising=False)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 3)
        try:
            got, kernel, merge = timed(lambda: part.topk_probed(q, po, pl, k, COS))
            assert kernel == launches and merge == 1
            assert_exact(got, truth(q, c, probes, cl, k, COS), k, f"d={d}")
        finally:
            part.close()
    finally:
        dc.close()


# ---- 7. k = 129 and the other refusals ----
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


def assert_lists(got, want, label):
    assert len(got) == len(want)
    for r, ((gi, gs), (wi, ws)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), f"{label}: row {r} indices {gi} != {wi}"
        assert same_bits(gs, ws.astype(np.float64), np.float64), f"{label}: row {r} score bits differ"


def test_k_129_is_refused_by_the_entry_and_served_by_the_fallback(clean_cache):
    q, c, probes, cl = main_shape(37, 17)
    po, pl = flat(probes)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 8)
        try:
            with pytest.raises(_native.PmmError) as ei:
                part.topk_probed(q, po, pl, 129, COS)
            assert ei.value.code == _native.PMM_ERR_UNSUPPORTED and "128" in str(ei.value)
            with pytest.raises(_native.PmmError) as ei:
                part.topk_probed(q, po, np.where(pl == 6, 8, pl).astype(np.uint32), 10, COS)
            assert ei.value.code == _native.PMM_ERR_ARG and "query row" in str(ei.value)
        finally:
            part.close()
        with pytest.raises(_native.PmmError) as ei:
            dc.topk_probed(q, po, pl, 10, COS)
        assert ei.value.code == _native.PMM_ERR_ARG and "not partitioned" in str(ei.value)
    finally:
        dc.close()
    c64 = _native.DeviceCorpus(c.astype(np.float64))
    try:
        part = c64.partition(cl, 8)
        try:
            with pytest.raises(_native.PmmError) as ei:
                part.topk_probed(q, po, pl, 10, COS)
            assert ei.value.code == _native.PMM_ERR_UNSUPPORTED
        finally:
            part.close()
    finally:
        c64.close()
    lists = pa.array([[None if x == NONE else int(x) for x in p] for p in probes], type=pa.list_(pa.int64()))
    labels = pa.array([None if x == NONE else int(x) for x in cl], type=pa.int64())
    out = pm._topk(arrow_rows(q), arrow_rows(c), 129, "cosine", groups=(lists, labels))
    assert_lists(ragged(out), truth(q, c, probes, cl, 129, COS), "k = 129 through groups=")


# ---- 8. the Arrow and NumPy forms ----
def test_groups_with_lists_on_arrow_and_numpy_inputs(clean_cache):
    m, n, d, k = 23, 4111, 64, 10
    rs = np.random.RandomState(61)
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    names = np.array(["de", "en", "fr", "it", "xx"])  # ("xx": no corpus row)
    code = rs.randint(0, 4, size=n)
    cl = names[code].astype(object)
    cl[::97] = None
    lists = [names[rs.randint(0, 5, size=rs.randint(0, 4))].tolist() for _ in range(m)]
    lists[3], lists[4], lists[5] = None, ["en", None, "de"], ["xx"]
    al = pa.array(lists, type=pa.list_(pa.string()))
    acl = pa.array(cl, type=pa.string())
    aq, ac = arrow_rows(q), arrow_rows(c)
    # the truth on integer codes: None and "xx" name no group
    ncl = np.where(np.array([x is None for x in cl]), NONE, code).astype(np.uint32)
    where = {"de": 0, "en": 1, "fr": 2, "it": 3}
    probes = [[] if p is None else [where[x] for x in p if x in where] for p in lists]
    want = truth(q, c, probes, ncl, k, COS)
    _native.timing_enable(True)
    _native.timing_reset()
    out = pm._topk(aq, ac, k, "cosine", groups=(al, acl))
    first = (_native.timing_read("subset_gather")[1], _native.timing_read("probe_merge")[1])
    _native.timing_reset()
    out2 = pm._topk(aq, ac, k, "cosine", groups=(al.cast(pa.large_list(pa.string())), acl))
    second = (_native.timing_read("subset_gather")[1], _native.timing_read("probe_merge")[1])
    _native.timing_enable(False)
    assert first == (1, 1) and second == (0, 1), "the second call on the same label array partitioned again"
    assert out.type == pa.large_list(pm._TOPK_STRUCT) and out.equals(out2)
    assert len([key for key in pm._cache if "groups" in key]) == 1 and len(pm._cache) == 2
    assert_lists(ragged(out), want, "groups= with lists")
    lens = np.diff(out.offsets.to_numpy())
    assert lens[3] == 0 and lens[5] == 0 and lens[4] == k
    # the NumPy form: a label matrix, one row of probes per query (never cached: the host fallback)
    import polars_matmul

    mat = rs.randint(0, 6, size=(m, 3))
    gi, gs = polars_matmul.topk(q, c, k, "cosine", groups=(mat, np.where(ncl == NONE, 9, ncl).astype(mat.dtype)))
    mprobes = [[x for x in row if x < 4] for row in mat.tolist()]
    for r, (wi, ws) in enumerate(truth(q, c, mprobes, ncl, k, COS)):
        assert np.array_equal(gi[r, :wi.size], wi) and same_bits(gs[r, :wi.size], ws.astype(np.float64), np.float64)
        assert np.all(gi[r, wi.size:] == 0xFFFFFFFF) and np.all(np.isnan(gs[r, wi.size:]))
