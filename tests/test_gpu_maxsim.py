"""Late-interaction search on multi-vector handles (pmm_topk_f32_maxsim,
``DeviceCorpus.multivector`` / ``topk_maxsim``, ``_topk_maxsim``,
``polars_matmul.topk_maxsim``): exact MaxSim top-k over per-row document lists.

The truth of a (query, document) pair: ``oracle.similarity(Q_i, D_c, metric)``,
``np.fmax.reduce(axis=1, initial=-inf)`` over the document's tokens, then a
Python loop of ``np.float32`` adds from +0.0 in token order.  A row's list is
its documents by (score descending, id ascending, NaN last).  Indices, score
bits, lengths and padding must be equal; there are no tolerances in this file
(a NaN score is the engine's one quiet NaN, as in every key-decoded list).
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

COS, DOT = _native.METRIC_COSINE, _native.METRIC_DOT
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT}
NAME = {COS: "cosine", DOT: "dot"}
EMPTY = 0xFFFFFFFF
LQ = (1, 31, 32, 33, 64, 70, 0)
LD = (1, 2, 31, 32, 33, 63, 64, 65, 130)
NDOCS = 67
DUPES = (5, 14, 23, 32)  # one document four times (the same place of the length cycle)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def offsets_of(lens):
    o = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=o[1:])
    return o


def pair_scores(qt, qo, dt, do, metric):
    """[m][n_docs] f32 MaxSim scores by the definition."""
    m, nd = qo.size - 1, do.size - 1
    out = np.zeros((m, nd), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(m):
            Q = f32(qt[qo[i]:qo[i + 1]])
            if Q.shape[0] == 0:
                continue
            for c in range(nd):
                s = np.asarray(oracle.similarity(Q, f32(dt[do[c]:do[c + 1]]), ORACLE_METRIC[metric]), dtype=np.float32)
                mx = np.fmax.reduce(s, axis=1, initial=-np.inf).astype(np.float32)
                acc = np.float32(0.0)
                for t in range(mx.size):
                    acc = np.float32(acc + mx[t])
                out[i, c] = acc
    return out


def truth(scores, qo, co, ci, k):
    """(idx [m, k], scores f32 [m, k], lens [m]) from the pair scores, padded
    as the entry pads (index 0xFFFFFFFF, score +0.0)."""
    m = qo.size - 1
    idx = np.full((m, k), EMPTY, dtype=np.uint32)
    sc = np.zeros((m, k), dtype=np.float32)
    lens = np.zeros(m, dtype=np.uint32)
    for i in range(m):
        S = ci[co[i]:co[i + 1]].astype(np.int64)
        if qo[i + 1] == qo[i] or S.size == 0:
            continue
        v = scores[i, S]
        nan = np.isnan(v)
        order = np.lexsort((S, -np.where(nan, 0, v).astype(np.float64), nan))  # NaN last, score descending, id ascending
        kk = min(k, S.size)
        lens[i] = kk
        idx[i, :kk] = S[order[:kk]]
        sc[i, :kk] = v[order[:kk]]
    # (a NaN leaves the engine's ordered keys as the one quiet NaN 0x7FC00000, whatever
    # sign or payload the host's inf - inf has)
    sc.view(np.uint32)[np.isnan(sc)] = 0x7FC00000
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
    assert bad.size == 0, f"{label}: score bits differ in rows {bad[:8]}: {gs[bad[0]][:6]} vs {ws[bad[0]][:6]}"


def lists(counts, n, seed):
    rs = np.random.RandomState(seed)
    ids = np.concatenate([np.sort(rs.choice(n, size=int(c), replace=False)) for c in counts] + [np.zeros(0, np.int64)])
    return offsets_of(counts), np.ascontiguousarray(ids, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def data(d):
    """(query tokens, query offsets, document tokens, document offsets)."""
    rs = np.random.RandomState(300 + d)
    qo = offsets_of(LQ)
    do = offsets_of([LD[c % len(LD)] for c in range(NDOCS)])
    qt, dt = f32(rs.randn(qo[-1], d)), f32(rs.randn(do[-1], d))
    for c in DUPES[1:]:
        dt[do[c]:do[c + 1]] = dt[do[DUPES[0]]:do[DUPES[0] + 1]]
    return qt, qo, dt, do


@functools.lru_cache(maxsize=None)
def scores(d, metric):
    return pair_scores(*data(d), metric)


@pytest.fixture(scope="module")
def corpora():
    made = {}

    def get(d):
        if d not in made:
            _, _, dt, do = data(d)
            made[d] = _native.DeviceCorpus.multivector(dt, do)
        return made[d]

    yield get
    for dc in made.values():
        dc.close()


def list_lengths(k, start):
    base = [min(max(x, 0), NDOCS) for x in (0, 1, k - 1, k, k + 1, 63, 64, 65, 67)]
    return [base[(start + i) % len(base)] for i in range(len(LQ))]


# ---- 1. every shape, both metrics, the cut at k ----
@pytest.mark.parametrize("k", [1, 10, 67, 100])
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("d", [1, 2, 3, 31, 32, 33, 128, 130, 256])
def test_lists_equal_the_definition(corpora, d, metric, k):
    qt, qo, dt, do = data(d)
    for start in (0, 4):  # all nine list lengths over the seven rows
        co, ci = lists(list_lengths(k, start + d + k), NDOCS, 11 * d + k + start)
        want = truth(scores(d, metric), qo, co, ci, k)
        got = corpora(d).topk_maxsim(qt, qo, co, ci, k, metric)
        assert_same(got, want, f"d={d} {NAME[metric]} k={k} start={start}")
        unused = np.arange(k)[None, :] >= want[2][:, None].astype(np.int64)
        assert (got[0][unused] == EMPTY).all() and (f32(got[1]).view(np.uint32)[unused] == 0).all()
    assert want[2][len(LQ) - 1] == 0  # the query without tokens


# ---- 2. ties ----
@pytest.mark.parametrize("metric", [COS, DOT])
def test_duplicate_documents_tie_to_the_lower_id(corpora, metric):
    d = 33
    qt, qo, _, _ = data(d)
    sc = scores(d, metric)
    every = np.arange(NDOCS, dtype=np.uint32)
    co = np.arange(len(LQ) + 1, dtype=np.int64) * NDOCS
    ci = np.tile(every, len(LQ))
    full = truth(sc, qo, co, ci, NDOCS)
    row = 3
    assert len({sc[row, c].tobytes() for c in DUPES}) == 1
    first = full[0][row].tolist().index(DUPES[0])
    assert full[0][row, first:first + 4].tolist() == list(DUPES)
    for k in range(first + 1, first + 5):  # the cut at k inside the tied group
        got = corpora(d).topk_maxsim(qt, qo, co, ci, k, metric)
        assert_same(got, truth(sc, qo, co, ci, k), f"ties {NAME[metric]} k={k}")
        assert got[0][row, first:k].tolist() == list(DUPES)[:k - first]


# ---- 3. values ----
def run_case(qt, qo, dt, do, metric, ks, label):
    sc = pair_scores(qt, qo, dt, do, metric)
    nd, m = do.size - 1, qo.size - 1
    co = np.arange(m + 1, dtype=np.int64) * nd
    ci = np.tile(np.arange(nd, dtype=np.uint32), m)
    dc = _native.DeviceCorpus.multivector(dt, do)
    try:
        for k in ks:
            assert_same(dc.topk_maxsim(qt, qo, co, ci, k, metric), truth(sc, qo, co, ci, k), f"{label} k={k}")
    finally:
        dc.close()
    return sc


@pytest.mark.parametrize("metric", [COS, DOT])
def test_nan_token_rows_are_ignored(metric):
    d = 20
    rs = np.random.RandomState(5)
    do = offsets_of([3, 1, 40, 2])
    dt = f32(rs.randn(do[-1], d))
    dt[1] = np.nan          # document 0: one NaN token among three
    dt[3] = np.nan          # document 1: its only token
    dt[4 + 35, 2] = np.nan  # document 2: one NaN element in its second block
    qo = offsets_of([2, 33])
    qt = f32(rs.randn(qo[-1], d))
    sc = run_case(qt, qo, dt, do, metric, (1, 2, 4), f"NaN tokens {NAME[metric]}")
    if metric == DOT:
        assert np.isneginf(sc[:, 1]).all() and np.isfinite(sc[:, 0]).all()


def test_inf_and_minus_inf_maxima_make_a_nan_score_that_sorts_last():
    d = 8
    e = np.eye(d, dtype=np.float32)
    do = offsets_of([1, 2, 1])
    dt = f32(np.stack([e[1], e[2], e[3], e[4]]))
    dt[0, 0] = np.inf
    qt = f32(np.stack([e[0], -e[0], e[0], e[0], -e[0], e[2]]))
    qo = offsets_of([2, 1, 3])
    with np.errstate(all="ignore"):
        sc = run_case(qt, qo, dt, do, DOT, (1, 2, 3), "inf - inf")
    assert np.isnan(sc[0, 0]) and np.isnan(sc[2, 0]) and np.isposinf(sc[1, 0])
    dc = _native.DeviceCorpus.multivector(dt, do)
    try:
        co = np.arange(4, dtype=np.int64) * 3
        gi, gs, _ = dc.topk_maxsim(qt, qo, co, np.tile(np.arange(3, dtype=np.uint32), 3), 3, DOT)
    finally:
        dc.close()
    assert gi[0, 2] == 0 and np.isnan(gs[0, 2]) and gi[1, 0] == 0


@pytest.mark.parametrize("metric", [COS, DOT])
def test_zero_maxima_sum_to_plus_zero(metric):
    d = 33
    rs = np.random.RandomState(6)
    do = offsets_of([2, 35, 1])
    dt = f32(rs.randn(do[-1], d))
    dt[-1] = -0.0
    qo = offsets_of([3, 40])
    qt = np.zeros((qo[-1], d), dtype=np.float32)
    qt[1] = -0.0
    qt[3:, :] = 0.0
    sc = run_case(qt, qo, dt, do, metric, (1, 3), f"zero maxima {NAME[metric]}")
    assert (sc.view(np.uint32) == 0).all()


@pytest.mark.parametrize("metric", [COS, DOT])
def test_signed_zero_rows_with_padded_columns(metric):
    q, c = value_case("signed_zero", np.float32, 5, 320, 33)
    rows = sorted(SIGNED_ZERO_ROWS)
    # the planted rows as one-token documents, all of them as one document, and two mixed ones
    dt = f32(np.concatenate([c[rows], c[rows], c[rows[:3]], c[[rows[1], 7, rows[3]]]]))
    do = offsets_of([1] * len(rows) + [len(rows), 3, 3])
    qt = f32(np.concatenate([q[0:1], q[1:2], q[2:3], q[0:3], q]))
    qo = offsets_of([1, 1, 1, 3, 5])
    sc = run_case(qt, qo, dt, do, metric, (1, 5, 11), f"signed zero {NAME[metric]}")
    assert (sc.view(np.uint32) != 0x80000000).all() and (sc.view(np.uint32) == 0).any()


# ---- 4. the sort routes and dirty scratch ----
@functools.lru_cache(maxsize=None)
def flat():
    """200 one-token documents, d = 33 (with one duplicate pair)."""
    rs = np.random.RandomState(77)
    do = np.arange(201, dtype=np.int64)
    dt = f32(rs.randn(200, 33))
    dt[150] = dt[20]
    qo = offsets_of([3, 33, 1, 2])
    qt = f32(rs.randn(qo[-1], 33))
    co, ci = lists([5, 128, 129, 200], 200, 3)
    return qt, qo, dt, do, co, ci


@functools.lru_cache(maxsize=None)
def flat_scores(metric):
    qt, qo, dt, do, _, _ = flat()
    return pair_scores(qt, qo, dt, do, metric)


@pytest.fixture(scope="module")
def flat_corpus():
    dc = _native.DeviceCorpus.multivector(flat()[2], flat()[3])
    yield dc
    dc.close()


@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("k", [10, 129, 300])
def test_lowered_sort_max_takes_the_cut_and_merge_route(flat_corpus, monkeypatch, metric, k):
    qt, qo, _, _, co, ci = flat()
    assert (np.diff(co) >= 130).sum() >= 1 and (np.diff(co) > 128).sum() >= 2
    want = truth(flat_scores(metric), qo, co, ci, k)
    assert_same(flat_corpus.topk_maxsim(qt, qo, co, ci, k, metric), want, f"block sort k={k}")
    monkeypatch.setenv("PMM_RANGE_SORT_MAX", "128")
    assert_same(flat_corpus.topk_maxsim(qt, qo, co, ci, k, metric), want, f"sort max 128, k={k}")


@pytest.mark.parametrize("poison", ["0xFF", "0x7F", "0x01"])
def test_poisoned_arena_gives_the_same_bits(flat_corpus, corpora, monkeypatch, poison):
    qt, qo, _, _, co, ci = flat()
    for metric in (COS, DOT):
        # wave sort (5, 128), block sort (129, 200), and with the lowered limit cut-and-merge
        for k, smax in ((10, None), (150, None), (150, "128")):
            want = truth(flat_scores(metric), qo, co, ci, k)
            if smax:
                monkeypatch.setenv("PMM_RANGE_SORT_MAX", smax)
            clean = flat_corpus.topk_maxsim(qt, qo, co, ci, k, metric)
            monkeypatch.setenv("PMM_ARENA_POISON", poison)
            got = flat_corpus.topk_maxsim(qt, qo, co, ci, k, metric)
            monkeypatch.delenv("PMM_ARENA_POISON")
            monkeypatch.delenv("PMM_RANGE_SORT_MAX", raising=False)
            assert_same(got, clean, f"poison {poison} {NAME[metric]} k={k} smax={smax}")
            assert_same(got, want, f"poison {poison} {NAME[metric]} k={k} smax={smax} vs the definition")
        # several token blocks and padded columns (d = 130) on dirty scratch
        d, k = 130, 10
        q2, qo2, _, _ = data(d)
        co2, ci2 = lists(list_lengths(k, 3), NDOCS, 9)
        monkeypatch.setenv("PMM_ARENA_POISON", poison)
        got = corpora(d).topk_maxsim(q2, qo2, co2, ci2, k, metric)
        monkeypatch.delenv("PMM_ARENA_POISON")
        assert_same(got, truth(scores(d, metric), qo2, co2, ci2, k), f"poison {poison} {NAME[metric]} d=130")


# ---- 5. the raw entry: flagged errors, refusals, guard bands ----
def raw(dc, qt, qo, co, ci, k, metric, planes=None):
    qt, qo = f32(qt), np.ascontiguousarray(qo, np.int64)
    m = qo.size - 1
    co, ci = np.ascontiguousarray(co, np.int64), np.ascontiguousarray(ci, np.uint32)
    oi, os_, ol = planes or (np.zeros((m, k), np.uint32), np.zeros((m, k), np.float32), np.zeros(m, np.uint32))
    rc = _native.lib().pmm_topk_f32_maxsim(dc._h, _native.ptr(qt), _native.ptr(qo), m, _native.ptr(co), _native.ptr(ci),
                                           k, metric, _native.ptr(oi), _native.ptr(os_), _native.ptr(ol))
    return rc, _native.last_error()


def test_bad_lists_are_reported_and_the_handle_serves_on(corpora):
    d = 33
    qt, qo, _, _ = data(d)
    dc = corpora(d)
    q2, qo2 = qt[:qo[2]], qo[:3]
    co = np.array([0, 3, 5], dtype=np.int64)
    for ids, text in (([5, 9, 7, 1, 2], "strictly ascending"), ([5, 9, 9, 1, 2], "strictly ascending"),
                      ([5, 9, 10, 1, NDOCS], "not a document"), ([5, 9, 10, 1, 0xFFFFFFFF], "not a document")):
        rc, msg = raw(dc, q2, qo2, co, ids, 2, COS)
        assert rc == _native.PMM_ERR_ARG and text in msg, (ids, rc, msg)
        good_co, good_ci = lists([3, 2], NDOCS, 1)
        assert_same(dc.topk_maxsim(q2, qo2, good_co, good_ci, 2, COS), truth(scores(d, COS), qo2, good_co, good_ci, 2),
                    "after a refusal")
    for off, text in (([1, 3, 5], "start at 0"), ([0, 4, 3], "descend")):
        rc, msg = raw(dc, q2, qo2, off, [1, 2, 3, 4, 5], 2, COS)
        assert rc == _native.PMM_ERR_ARG and text in msg, msg
    rc, msg = raw(dc, q2, [0, 2, 1], co, [1, 2, 3, 4, 5], 2, COS)
    assert rc == _native.PMM_ERR_ARG and "q_offsets must not descend" in msg
    rc, msg = raw(dc, q2, qo2, [0, NDOCS + 1, NDOCS + 1], np.zeros(NDOCS + 1), 2, COS)
    assert rc == _native.PMM_ERR_ARG and "lists 68 documents" in msg
    rc, msg = raw(dc, q2, qo2, co, [1, 2, 3, 4, 5], 2, _native.METRIC_EUCLIDEAN)
    assert rc == _native.PMM_ERR_ARG and "not a similarity" in msg
    assert raw(dc, q2, qo2, co, [1, 2, 3, 4, 5], 2, 7)[0] == _native.PMM_ERR_ARG
    rc, msg = raw(dc, q2, qo2, co, [1, 2, 3, 4, 5], 0, COS)
    assert rc == _native.PMM_ERR_ARG and "k must be >= 1" in msg
    L = _native.lib()
    assert L.pmm_topk_f32_maxsim(dc._h, None, None, 0, None, None, 1, COS, None, None, None) == _native.PMM_OK
    assert L.pmm_topk_f32_maxsim(dc._h, None, None, 2, None, None, 1, COS, None, None, None) == _native.PMM_ERR_ARG
    assert L.pmm_topk_f32_maxsim(dc._h, None, None, -1, None, None, 1, COS, None, None, None) == _native.PMM_ERR_ARG


def test_other_handles_are_refused_and_bad_offsets_make_no_handle():
    d = 33
    qt, qo, dt, do = data(d)
    co, ci = lists([3, 2], 20, 1)
    made = []
    try:
        f = _native.DeviceCorpus.multivector(dt, do)
        made.append(f)
        labels = (np.arange(dt.shape[0]) % 3).astype(np.uint32)
        others = [("no documents", _native.DeviceCorpus(dt)), ("f64", _native.DeviceCorpus(dt.astype(np.float64))),
                  ("bf16", _native.DeviceCorpus(dt, compute="bf16")),
                  ("int8", _native.DeviceCorpus.int8((dt * 10).astype(np.int8))),
                  ("derived", f.subset(np.arange(0, dt.shape[0], 2, dtype=np.uint32))),
                  ("partitioned", f.partition(labels, 3)), ("bit", f.sign_bits())]
        made += [dc for _, dc in others]
        for what, dc in others:
            rc, msg = raw(dc, qt[:qo[2]], qo[:3], co, ci, 2, COS)
            assert rc == _native.PMM_ERR_ARG and what in msg, (what, rc, msg)
            assert dc.doc_offsets().tolist() == [0]  # derived handles carry no documents
        assert np.array_equal(f.doc_offsets(), do) and f.n_docs == NDOCS and f.n == dt.shape[0]
        plain = made[1]
        assert f.nbytes == plain.nbytes + 8 * do.size
    finally:
        for dc in made:
            dc.close()
    for bad, text in (([1, 5, dt.shape[0]], "start at 0"), ([0, 5, 5, dt.shape[0]], "ascend strictly"),
                      ([0, 5, 4, dt.shape[0]], "ascend strictly"), ([0, 5, dt.shape[0] - 1], "end at n_tokens")):
        with pytest.raises(_native.PmmError) as ei:
            _native.DeviceCorpus.multivector(dt, np.array(bad, dtype=np.int64))
        assert ei.value.code == _native.PMM_ERR_ARG and text in str(ei.value)


def test_output_planes_between_guard_bands(corpora):
    d, k = 33, 10
    qt, qo, _, _ = data(d)
    co, ci = lists(list_lengths(k, 2), NDOCS, 4)
    m = qo.size - 1
    G = 1024
    bufs = [np.full(n + 2 * G, 0xA5A5A5A5, dtype=np.uint32) for n in (m * k, m * k, m)]
    oi = bufs[0][G:G + m * k].reshape(m, k)
    os_ = bufs[1][G:G + m * k].view(np.float32).reshape(m, k)
    ol = bufs[2][G:G + m]
    rc, msg = raw(corpora(d), qt, qo, co, ci, k, COS, planes=(oi, os_, ol))
    assert rc == _native.PMM_OK, msg
    assert_same((oi, os_, ol), truth(scores(d, COS), qo, co, ci, k), "guarded planes")
    for b, n in zip(bufs, (m * k, m * k, m)):
        assert (b[:G] == 0xA5A5A5A5).all() and (b[G + n:] == 0xA5A5A5A5).all()


# ---- 6. existing entries on a multi-vector handle ----
def test_existing_entries_see_the_plain_token_handle(corpora):
    d = 33
    qt, _, dt, _ = data(d)
    mv, plain = corpora(d), _native.DeviceCorpus(dt)
    bits_mv = bits_plain = None
    try:
        q = qt[:9]
        for metric in (COS, DOT, _native.METRIC_EUCLIDEAN):
            a, b = mv.topk(q, 10, metric), plain.topk(q, 10, metric)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        a, b = mv.range(q, 0.2, COS), plain.range(q, 0.2, COS)
        assert a[0][-1] > 0 and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        co, ci = lists([0, 1, 64, 300, 5, 129, 2, 70, 33], dt.shape[0], 2)
        a, b = mv.topk_candidates(q, co, ci, 20, COS), plain.topk_candidates(q, co, ci, 20, COS)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        bits_mv, bits_plain = mv.sign_bits(), plain.sign_bits()
        assert np.array_equal(bits_mv.bit_rows(), bits_plain.bit_rows())
        assert np.array_equal(bits_mv.bit_rows(), pm.pack_sign(dt))
    finally:
        for dc in (plain, bits_mv, bits_plain):
            if dc is not None:
                dc.close()


# ---- 7. the Python surface ----
def ragged(want):
    idx, sc, lens = want
    return [[(int(idx[i, j]), float(sc[i, j])) for j in range(int(lens[i]))] for i in range(idx.shape[0])]


def same_ragged(out, want):
    got, exp = [[(e["index"], e["score"]) for e in row] for row in out.to_pylist()], ragged(want)
    assert [[p[0] for p in r] for r in got] == [[p[0] for p in r] for r in exp]
    a = np.array([p[1] for r in got for p in r], dtype=np.float64)
    b = np.array([p[1] for r in exp for p in r], dtype=np.float64)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def token_column(tokens, offsets, d, ragged_inner=False):
    flat_values = pa.array(tokens.reshape(-1))
    if ragged_inner:
        inner = pa.ListArray.from_arrays(pa.array(np.arange(tokens.shape[0] + 1, dtype=np.int32) * d), flat_values)
    else:
        inner = pa.FixedSizeListArray.from_arrays(flat_values, d)
    return pa.LargeListArray.from_arrays(pa.array(offsets, type=pa.int64()), inner)


@pytest.mark.parametrize("metric", [COS, DOT])
def test_every_entry_returns_the_same_lists(corpora, monkeypatch, metric):
    d, k = 256, 10
    qt, qo, dt, do = data(d)
    assert dt.nbytes >= pm._CACHE_MIN_BYTES  # cacheable
    co, ci = lists(list_lengths(k, 1), NDOCS, 21)
    sc = scores(d, metric)
    want = truth(sc, qo, co, ci, k)
    assert_same(corpora(d).topk_maxsim(qt, qo, co, ci, k, metric), want, "DeviceCorpus.topk_maxsim")
    # the caller's lists: unsorted, with duplicates
    rs = np.random.RandomState(2)
    rows = [rs.permutation(np.concatenate([ci[co[i]:co[i + 1]], ci[co[i]:co[i + 1]][:2]]).astype(np.int64)).tolist()
            for i in range(len(LQ))]
    cand = pa.array(rows, type=pa.large_list(pa.int64()))
    queries, docs = token_column(qt, qo, d), token_column(dt, do, d)
    pm.clear_corpus_cache()
    try:
        monkeypatch.setattr(pm, "_CACHE_ON", True)
        same_ragged(pm._topk_maxsim(queries, docs, k, NAME[metric], candidates=cand), want)
        assert len(pm._cache) == 1  # searched on the cached multi-vector handle
        same_ragged(pm._topk_maxsim(token_column(qt, qo, d, True), docs, k, NAME[metric], candidates=(co, ci)), want)
        assert len(pm._cache) == 1
        pm.clear_corpus_cache()
        monkeypatch.setattr(pm, "_CACHE_ON", False)  # the forced fallback: the union's documents, renumbered lists
        same_ragged(pm._topk_maxsim(queries, docs, k, NAME[metric], candidates=cand), want)
        assert len(pm._cache) == 0
        gi, gs = polars_matmul.topk_maxsim((qt, qo), (dt, do), k, NAME[metric], candidates=(co, ci))
        unused = np.arange(k)[None, :] >= want[2][:, None].astype(np.int64)
        assert np.array_equal(gi, want[0]) and np.isnan(gs[unused]).all()
        assert np.array_equal(gs[~unused].view(np.uint64), want[1].astype(np.float64)[~unused].view(np.uint64))
        # candidates=None: every document for every row; k clips to their number
        every = np.tile(np.arange(NDOCS, dtype=np.uint32), len(LQ))
        full = truth(sc, qo, np.arange(len(LQ) + 1, dtype=np.int64) * NDOCS, every, NDOCS)
        same_ragged(pm._topk_maxsim(queries, docs, 1000, NAME[metric]), full)
        gi, gs = polars_matmul.topk_maxsim((qt, qo), (dt, do), 1000, NAME[metric])
        assert gi.shape == (len(LQ), NDOCS) and np.array_equal(gi, full[0])
    finally:
        pm.clear_corpus_cache()
