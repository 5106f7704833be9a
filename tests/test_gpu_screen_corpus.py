"""The bf16 screen of the f32 cosine top-k on cached corpus handles: an f32
``DeviceCorpus`` builds its screen image on the first call whose shape asks for
the screen and every such call then screens against it.

"Exact" below: indices and f32 score bits equal a fresh handle's call under
PMM_F32_SCREEN=0 (the f32 kernel on the cached norms) and ``oracle.topk``.
"""
from __future__ import annotations

import threading

import numpy as np
import pytest

import oracle
from polars_matmul import _native

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
BUILD = "corpus_image_build"  # the image build's timing label (no "/screen" in it)


def same_bits(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def screen_reports(capfd):
    """The screened calls' own reports (PMM_SCREEN_DEBUG), one dict per call."""
    reps = []
    for ln in capfd.readouterr().err.splitlines():
        if ln.startswith("[pmm screen]"):
            rep = {}
            for tok in ln.split()[2:]:
                key, val = tok.split("=")
                rep[key] = float(val) if "." in val or "e" in val else int(val)
            reps.append(rep)
    return reps


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def image_bytes(n, d):
    return _native.corpus_device_bytes(n, d, np.float32, screen=True) - _native.corpus_device_bytes(n, d, np.float32)


def timed_topk(dc, q, k, metric=COS):
    """(lists, "/screen" launches, image-build launches) of one call, timed on this thread."""
    _native.timing_enable(True)
    _native.timing_reset()
    try:
        got = dc.topk(q, k, metric)
        _, screened = _native.timing_read("/screen")
        _, built = _native.timing_read(BUILD)
    finally:
        _native.timing_reset()
        _native.timing_enable(False)
    return got, screened, built


def assert_exact(monkeypatch, got, q, c, k, label, metric=COS, screen="1"):
    """got == a fresh handle under PMM_F32_SCREEN=0 == the oracle; leaves the knob at ``screen``."""
    monkeypatch.setenv("PMM_F32_SCREEN", "0")
    plain = _native.DeviceCorpus(c)
    try:
        i0, s0 = plain.topk(q, k, metric)
        assert plain.nbytes == _native.corpus_device_bytes(*c.shape, np.float32), f"{label}: knob off built an image"
    finally:
        plain.close()
        if screen is None:
            monkeypatch.delenv("PMM_F32_SCREEN")
        else:
            monkeypatch.setenv("PMM_F32_SCREEN", screen)
    assert np.array_equal(got[0], i0), f"{label}: indices differ from the unscreened handle"
    assert same_bits(got[1], s0), f"{label}: scores differ from the unscreened handle"
    oi, osc = oracle.topk(q, c, k, ORACLE_METRIC[metric])
    assert np.array_equal(got[0].astype(np.int64), np.asarray(oi).astype(np.int64)), f"{label}: indices differ from the oracle"
    assert same_bits(got[1], np.asarray(osc).astype(np.float32)), f"{label}: scores differ from the oracle"


@pytest.fixture
def screen_on(monkeypatch):
    assert _native.device_count() > 0, "no HIP device visible"
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    monkeypatch.setenv("PMM_SCREEN_DEBUG", "1")
    return monkeypatch


# m not a multiple of the 32-row wave, n from the smallest allowed to sizes that
# are no multiple of the 64-column tile, d padded to 128, k = 1, 10, 100, k = n
SHAPES = [(1, 1, 1, 1), (1, 38, 37, 1), (33, 47, 700, 10), (70, 100, 768, 100), (70, 137, 1, 100),
          (33, 1037, 700, 100), (70, 3037, 768, 10), (1, 3000, 128, 1)]


@pytest.mark.parametrize("m,n,d,k", SHAPES)
def test_handle_screens_and_is_exact_on_ragged_shapes(screen_on, m, n, d, k):
    rs = np.random.RandomState(1000 * m + n + d + k)
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        got, screened, built = timed_topk(dc, q, k)
        assert screened >= 1, "the handle's call did not screen"
        assert built == 1 and dc.nbytes == base + image_bytes(n, d)
        assert_exact(screen_on, got, q, c, k, f"{m}x{n}x{d} k={k}")
    finally:
        dc.close()


def test_image_is_built_once_and_reused(screen_on, capfd):
    rs = np.random.RandomState(21)
    n, d, k = 1037, 700, 10
    c = f32(rs.randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        assert base == _native.corpus_device_bytes(n, d, np.float32)
        builds = 0
        for call, m in enumerate((33, 70, 1)):
            q = f32(rs.randn(m, d))
            capfd.readouterr()
            got, screened, built = timed_topk(dc, q, k)
            reps = screen_reports(capfd)
            builds += built
            assert screened >= 1 and built == (1 if call == 0 else 0)
            assert dc.nbytes == base + image_bytes(n, d)  # grown by the first call, not after it
            assert len(reps) == 1 and reps[0]["handle"] == 1 and reps[0]["m"] == m
            assert reps[0]["corpus_unsafe"] == 0 and 0 < reps[0]["corpus_residual"] <= 2.0 ** -8
            assert_exact(screen_on, got, q, c, k, f"call {call} m={m}")
        assert builds == 1
    finally:
        dc.close()


UNSAFE = {"zero-row": None, "nan": np.nan, "inf": np.inf, "subnormal": 1e-40, "above-window": 2.0 ** 49}


def plant(a, what):
    if what == "zero-row":
        a[5, :] = 0.0
    else:
        a[5, 17] = UNSAFE[what]


@pytest.mark.parametrize("what", list(UNSAFE))
def test_unsafe_corpus_never_screens(screen_on, what):
    rs = np.random.RandomState(13)
    m, n, d, k = 33, 300, 96, 10
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    plant(c, what)
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        for call in range(2):
            got, screened, built = timed_topk(dc, q, k)
            # the flag is read once, at the build: no screen pass in the first call or after it
            assert screened == 0 and built == (1 if call == 0 else 0), f"call {call}"
            assert dc.nbytes == base
            assert_exact(screen_on, got, q, c, k, f"{what} in a corpus row, call {call}")
    finally:
        dc.close()


@pytest.mark.parametrize("what", list(UNSAFE))
def test_unsafe_query_row_is_rerun(screen_on, capfd, what):
    rs = np.random.RandomState(13)
    q, c = f32(rs.randn(33, 100)), f32(rs.randn(1037, 100))
    plant(q, what)
    dc = _native.DeviceCorpus(c)
    try:
        capfd.readouterr()
        got, screened, _ = timed_topk(dc, q, 10)
        rep = screen_reports(capfd)[0]
        assert screened >= 1 and rep["handle"] == 1
        assert rep["rerun_rows"] >= 1 and rep["whole_call_f32"] == 0 and rep["corpus_unsafe"] == 0
        assert_exact(screen_on, got, q, c, 10, f"{what} in a query row")
    finally:
        dc.close()


def test_crowded_band_overflows_and_reruns(screen_on, capfd):
    # ~2000 near-copies of one vector at relative spacing 1e-4 .. 1e-6 and a query aligned with it: far more
    # than a segment holds within 2 eps of the k-th, so the row overflows and the f32 kernel finishes it.
    # Planned for one workgroup: the row's single segment (capg 256) sees the whole crowd.
    screen_on.setenv("PMM_CUS", "1")
    rs = np.random.RandomState(3)
    d, k = 128, 10
    v = rs.randn(d).astype(np.float32)
    near = v[None, :] * (1.0 + rs.randn(2000, d).astype(np.float32) * 10.0 ** rs.uniform(-6, -4, (2000, 1)).astype(np.float32))
    c = np.concatenate([rs.randn(1500, d).astype(np.float32), near.astype(np.float32)])
    c = f32(c[rs.permutation(len(c))])
    q = f32(np.concatenate([v[None, :] * np.float32(0.5), rs.randn(34, d).astype(np.float32)]))
    dc = _native.DeviceCorpus(c)
    try:
        capfd.readouterr()
        got, screened, _ = timed_topk(dc, q, k)
        rep = screen_reports(capfd)[0]
        assert screened >= 1 and rep["handle"] == 1
        assert rep["overflowed"] >= 1 and rep["rerun_rows"] >= rep["overflowed"] and rep["whole_call_f32"] == 0
        assert_exact(screen_on, got, q, c, k, "crowded band")
    finally:
        dc.close()


def test_exact_duplicates_go_to_the_lower_index(screen_on):
    rs = np.random.RandomState(5)
    base = rs.randn(40, 64).astype(np.float32)
    c = f32(np.concatenate([base] * 30))  # every corpus row 30 times
    q = f32(rs.randn(33, 64))
    dc = _native.DeviceCorpus(c)
    try:
        got, screened, _ = timed_topk(dc, q, 100)
        assert screened >= 1
        assert_exact(screen_on, got, q, c, 100, "duplicates")
        i1, s1 = got
        for r in range(i1.shape[0]):  # equal scores are listed in ascending index order
            tie = s1[r, 1:] == s1[r, :-1]
            assert np.all(i1[r, 1:][tie].astype(np.int64) > i1[r, :-1][tie].astype(np.int64))
    finally:
        dc.close()


@pytest.mark.parametrize("metric,k,d", [(DOT, 10, 96), (EUC, 10, 96), (COS, 200, 96), (COS, 10, 800)],
                         ids=["dot", "euclidean", "k=200", "d=800"])
def test_outside_the_screens_limits_nothing_is_built(screen_on, metric, k, d):
    rs = np.random.RandomState(31)
    m, n = 33, 1037
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        got, screened, built = timed_topk(dc, q, k, metric)
        assert screened == 0 and built == 0 and dc.nbytes == base
        assert_exact(screen_on, got, q, c, k, "outside the limits", metric)
    finally:
        dc.close()


def test_sharded_handle_stays_unscreened(screen_on):
    rs = np.random.RandomState(37)
    m, n, d, k = 33, 1037, 96, 10
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    one = _native.DeviceCorpus(c)
    dc = None
    try:
        _native.set_devices([0, 0])
        dc = _native.DeviceCorpus(c)
        assert dc.shards == 2 and one.shards == 1
        base = dc.nbytes
        assert base == _native.corpus_device_bytes(n, d, np.float32)
        got, screened, built = timed_topk(dc, q, k)
        assert screened == 0 and built == 0 and dc.nbytes == base
        ref, ref_screened, _ = timed_topk(one, q, k)
        assert ref_screened >= 1
        assert np.array_equal(got[0], ref[0]) and same_bits(got[1], ref[1])
    finally:
        _native.set_devices([])
        one.close()
        if dc is not None:
            dc.close()


def test_knob_off_never_builds(screen_on):
    screen_on.setenv("PMM_F32_SCREEN", "0")
    rs = np.random.RandomState(41)
    m, n, d, k = 33, 1037, 700, 10
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        for _ in range(2):
            got, screened, built = timed_topk(dc, q, k)
            assert screened == 0 and built == 0 and dc.nbytes == base
        oi, osc = oracle.topk(q, c, k, oracle.COSINE)
        assert np.array_equal(got[0].astype(np.int64), np.asarray(oi).astype(np.int64))
        assert same_bits(got[1], np.asarray(osc).astype(np.float32))
    finally:
        dc.close()


def test_default_thresholds_are_the_device_entrys(screen_on):
    screen_on.delenv("PMM_F32_SCREEN")
    rs = np.random.RandomState(7)
    m, n, d, k = 33, 2037, 96, 10
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        got, screened, built = timed_topk(dc, q, k)
        assert screened == 0 and built == 0 and dc.nbytes == base
        assert_exact(screen_on, got, q, c, k, "default thresholds", screen=None)
    finally:
        dc.close()


def test_two_threads_make_the_first_screened_call(screen_on):
    rs = np.random.RandomState(43)
    m, n, d, k = 33, 1037, 700, 10
    c = f32(rs.randn(n, d))
    qs = [f32(rs.randn(m, d)) for _ in range(2)]
    dc = _native.DeviceCorpus(c)
    try:
        base = dc.nbytes
        start = threading.Barrier(2)
        res = [None, None]

        def first_call(i):
            start.wait()
            try:
                res[i] = timed_topk(dc, qs[i], k)  # (timing is recorded per thread)
            except BaseException as e:  # noqa: BLE001 - reported by the assertion below
                res[i] = e

        ts = [threading.Thread(target=first_call, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for r in res:
            assert not isinstance(r, BaseException), r
        assert res[0][2] + res[1][2] == 1, "the image was not built exactly once"
        assert dc.nbytes == base + image_bytes(n, d)
        for i in range(2):
            assert res[i][1] >= 1
            assert_exact(screen_on, res[i][0], qs[i], c, k, f"thread {i}")
    finally:
        dc.close()


def lists_of(out, m, k):
    vals = out.values
    return (vals.field("index").to_numpy().reshape(m, k), vals.field("score").to_numpy().reshape(m, k))


def test_through_topk_and_the_corpus_cache(screen_on):
    import pyarrow as pa

    from polars_matmul import _polars_matmul as pm

    rs = np.random.RandomState(47)
    m, n, d, k = 33, 2100, 128, 10  # 1.05 MiB of f32 rows: above the cache's floor
    q, c = f32(rs.randn(m, d)), f32(rs.randn(n, d))
    arr = pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1), type=pa.float32()), d)
    qarr = pa.FixedSizeListArray.from_arrays(pa.array(q.reshape(-1), type=pa.float32()), d)
    pm.clear_corpus_cache()
    try:
        screen_on.setenv("PMM_F32_SCREEN", "0")
        want = lists_of(pm._topk(qarr, arr, k, "cosine"), m, k)
        assert sum(v[1].nbytes for v in pm._cache.values()) == _native.corpus_device_bytes(n, d, np.float32)
        pm.clear_corpus_cache()
        screen_on.setenv("PMM_F32_SCREEN", "1")
        pm._topk(qarr, arr, k, "cosine")
        assert len(pm._cache) == 1
        _native.timing_enable(True)
        _native.timing_reset()
        got = lists_of(pm._topk(qarr, arr, k, "cosine"), m, k)  # the cached handle, its image built by the call before
        _, screened = _native.timing_read("/screen")
        _, built = _native.timing_read(BUILD)
        assert len(pm._cache) == 1 and screened >= 1 and built == 0
        assert got[1].dtype == np.float64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # the cache's byte total includes the image
        assert sum(v[1].nbytes for v in pm._cache.values()) == _native.corpus_device_bytes(n, d, np.float32, screen=True)
    finally:
        _native.timing_reset()
        _native.timing_enable(False)
        pm.clear_corpus_cache()
