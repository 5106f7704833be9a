"""The thread-safety contract of the handle entries (include/pmm.h: "every entry
point may be called concurrently from different threads (each thread owns its
HIP stream and scratch)", "a handle may be used from several threads
concurrently", and "Thread-safe like the other handle entries" on the range,
self, candidate, MaxSim and k-means entries) and of the Python corpus cache.

Every comparison is of raw bytes, with no tolerance: indices, score bits, CSR
offsets, lens, labels, centroids, update counts.  A result is first computed
serially and compared ONCE with the definition its feature test already has
(``oracle.topk``, tests/kmeans_cases.py, tests/self_cases.py, the ``truth``
functions of the feature tests), so that threaded and serial cannot agree on a
wrong answer; the threaded result is then compared with the serial one.

The frame (``run_threads``): every thread has inputs and an expected result of
its own, all threads leave one barrier together, each does exactly ROUNDS = 2
rounds, exceptions are re-raised on the main thread and no thread may be alive
after the join.  Nothing here provokes a device fault: the only failing calls
are argument errors.

What the serial pass leaves warm: it runs in this process before the threads
start, so process-wide first-call state (the launchers' opt-in to large LDS, a
thread-independent debug buffer) is already set when the threads race.  Only
per-handle state is raced cold: the screen image in 1b, the first
``sign_bits()`` of a handle in the bits case, the cache entries in part 2.

Shapes are the feature tests' own small ones, enlarged until a call runs
several kernels with a read-back in between; each is named where it is used.
"""
from __future__ import annotations

import os
import threading

import numpy as np
import pyarrow as pa
import pytest

import kmeans_cases as kc
import oracle
import self_cases as sc_
import test_bits_cpu as bits_cpu
import test_gpu_candidates as cand_
import test_gpu_grouped as grouped_
import test_gpu_maxsim as maxsim_
import test_gpu_probed as probed_
import test_gpu_range as range_
from concurrency_cases import JOIN, arrow_parts, assert_bits, frozen, run_threads
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
NONE = _native.NO_GROUP
T = 4
ROUNDS = 2
INF = float("inf")


@pytest.fixture
def env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    assert _native.device_count() > 0, "no HIP device visible"
    return monkeypatch


@pytest.fixture
def device_list():
    yield
    _native.set_devices([])


@pytest.fixture
def clean_cache():
    pm.clear_corpus_cache()
    yield
    pm.clear_corpus_cache()


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def randn(seed, rows, d):
    return f32(np.random.RandomState(seed).randn(rows, d))


def threaded_equals_serial(calls, serial, label, rounds=ROUNDS):
    """calls[t]() on T threads; every round of every thread has the bytes of serial[t]."""
    got = run_threads([lambda r, c=c: c() for c in calls], rounds)
    for t, per_round in enumerate(got):
        for r, res in enumerate(per_round):
            assert_bits(res, serial[t], f"{label}: thread {t} round {r}")


# ---------------------------------------------------------------------------
# The cases of 1a, one builder per entry: (handles to close, [call per thread],
# check(t, serial result) against the definition, [the call per thread that
# gives the serial result]: the same calls unless the threads must find a
# handle untouched).  1c and 1d take single threads' calls.
# ---------------------------------------------------------------------------
def range_case(env):
    """tests/test_gpu_range.py's long-segment shape (n = 2000, d = 37) with PMM_RANGE_SORT_MAX=1024
    as there: rows of up to 1024 hits are sorted in LDS, rows of 2000 go to the handle's top-k with
    k = 2000 (the any-k route: a second entry, with its own arena acquisition, inside the call)."""
    env.setenv("PMM_RANGE_SORT_MAX", "1024")
    c = randn(12, 2000, 37)
    dc = _native.DeviceCorpus(c)
    spec = []  # (q, threshold, metric, cap, any-k?)
    for t, (m, metric, how, cap) in enumerate([(33, COS, 0.9, None), (17, DOT, "all", None), (9, EUC, 0.1, 10),
                                                (5, COS, "all", 7)]):
        q = randn(100 + t, m, 37)
        full = range_.ranked(q, c, metric)
        if how == "all":
            thr = INF if metric == EUC else -INF
        else:
            thr = float(np.quantile(full[1][np.isfinite(full[1])], how))
        spec.append((q, thr, metric, cap, how == "all", full))

    def check(t, got):
        q, thr, metric, cap, anyk, full = spec[t]
        want = range_.cut(full, thr, metric)
        longest = int(np.diff(want[0]).max())
        assert (longest > 1024) == anyk and want[0][-1] > 0, (t, longest)
        if cap is not None:  # the first call has no room: the repeat with the exact total
            assert want[0][-1] > cap
        range_.assert_same(got, want, f"range thread {t} {NAME[metric]}")

    calls = [lambda s=s: dc.range(s[0], s[1], s[2], cap=s[3]) for s in spec]
    return [dc], calls, check, calls


def self_case(env, derived=False):
    """tests/test_gpu_self.py's ragged column, n = 700 instead of 300 (three 256-row tiles, so the
    triangular schedule has inner and diagonal tiles), d = 37; derived: the subset handle of its
    test_derived_handle, ties across the selection included."""
    n, d = 700, 37
    c = randn(81, n, d)
    c[200] = c[100] = c[3]
    dc = _native.DeviceCorpus(c)
    handles, h, ids = [dc], dc, np.arange(n, dtype=np.uint32)
    if derived:
        mask = np.random.RandomState(82).rand(n) < 0.5
        mask[[0, n - 1, 100, 200]] = True
        mask[3] = False
        ids = np.flatnonzero(mask).astype(np.uint32)
        h = dc.subset(mask)
        handles.insert(0, h)
    rows = f32(c[ids])
    fulls = {metric: sc_.ranked_self(rows, metric) for metric in (COS, DOT, EUC)}
    # (entry, metric, k or quantile, cap)
    spec = [("range", COS, None, None), ("topk", DOT, 10, None), ("range", EUC, None, 5), ("topk", COS, 33, None)]
    thr = {metric: sc_.median_threshold(fulls[metric]) for metric in (COS, EUC)}

    def call(entry, metric, k, cap):
        if entry == "range":
            return h.range_self(thr[metric], metric, cap=cap)
        return h.topk_self(k, metric)

    def check(t, got):
        entry, metric, k, cap = spec[t]
        if entry == "range":
            wo, wi, ws = sc_.range_self_truth(fulls[metric], thr[metric], metric)
            assert cap is None or wo[-1] > cap
            sc_.assert_same_csr(got, (wo, ids[wi], ws), f"range_self thread {t}")
        else:
            ti, ts = sc_.topk_self_truth(fulls[metric], k)
            sc_.assert_same_lists(got, (ids[ti], ts), f"topk_self thread {t}")

    calls = [lambda s=s: call(*s) for s in spec]
    return handles, calls, check, calls


def candidates_case(env):
    """tests/test_gpu_candidates.py's corpus (N = 1237, d = 33) with PMM_RANGE_SORT_MAX=256: lists
    of up to 128 ids sort in a wave, up to 256 in a workgroup, longer ones are cut into pieces and
    merged (the long-row path, with its second key array)."""
    env.setenv("PMM_RANGE_SORT_MAX", "256")
    N, d = cand_.N, 33
    c = randn(133, N, d)
    dc = _native.DeviceCorpus(c)
    spec = []
    for t, (counts, k, metric) in enumerate([([1, 5, 63, 64, 65, 128, 100], 10, COS),        # short lists
                                             ([300, N, 257, 700, 1000], 100, DOT),           # long rows
                                             ([0, 7, 129, 256, 0, 40], 5, EUC),              # empty lists
                                             (cand_.boundary_counts(400, N, 15), 400, COS)]):  # every tier, cut at k
        q = randn(140 + t, len(counts), d)
        offsets, ids = cand_.lists(counts, N, 150 + t)
        spec.append((q, offsets, ids, k, metric))

    def check(t, got):
        q, offsets, ids, k, metric = spec[t]
        cand_.assert_same(got, cand_.truth(q, c, offsets, ids, k, metric), f"candidates thread {t}")

    calls = [lambda s=s: dc.topk_candidates(*s) for s in spec]
    return [dc], calls, check, calls


def maxsim_case(env, d=37):
    """150 documents of 1 .. 33 tokens (tests/test_gpu_maxsim.py's lengths, more documents than its
    67 so that a list can pass 128) with PMM_RANGE_SORT_MAX=128 as its sort-route test: lists of up
    to 128 documents are sorted in a wave, longer ones cut and merged -- the two sort classes."""
    env.setenv("PMM_RANGE_SORT_MAX", "128")
    nd = 150
    lens = [(1, 2, 5, 31, 33, 7)[j % 6] for j in range(nd)]
    do = maxsim_.offsets_of(lens)
    dt = randn(300 + d, int(do[-1]), d)
    dc = _native.DeviceCorpus.multivector(dt, do)
    spec = []
    for t, (counts, k, metric) in enumerate([([5, 64, 128], 10, COS), ([129, 150, 140], 150, DOT),
                                             ([150, 0, 130], 129, COS), ([1, 128, 129], 10, DOT)]):
        qo = maxsim_.offsets_of([(1, 33, 7)[(t + j) % 3] for j in range(len(counts))])
        qt = randn(310 + t, int(qo[-1]), d)
        co, ci = maxsim_.lists(counts, nd, 320 + t)
        spec.append((qt, qo, co, ci, k, metric))

    def check(t, got):
        qt, qo, co, ci, k, metric = spec[t]
        scores = maxsim_.pair_scores(qt, qo, dt, do, metric)
        maxsim_.assert_same(got, maxsim_.truth(scores, qo, co, ci, k), f"maxsim d={d} thread {t}")

    calls = [lambda s=s: dc.topk_maxsim(*s) for s in spec]
    return [dc], calls, check, calls


def kmeans_case(env):
    """tests/test_gpu_kmeans.py's planted rows (16 centres, noise 2.0), n = 3000, d = 33: several
    updates with label changes, so every call reads its changed flag back several times while the
    other threads' kernels run."""
    x, _, _ = kc.planted(3000, 33, 16, 7, noise=2.0)
    dc = _native.DeviceCorpus(x)
    spec = [(kc.default_init(x, K, seed), metric, it) for K, seed, metric, it in
            [(5, 0, EUC, 5), (16, 1, COS, 5), (64, 2, EUC, 3), (3, 3, COS, 6)]]

    def check(t, got):
        init, metric, it = spec[t]
        want = kc.kmeans_ref(x, init, metric, it)
        assert want[3] >= 2, f"a degenerate case: {want[3]} updates"
        assert got[3] == want[3] and bool(got[4]) == want[4], (got[3:], want[3:5])
        for j in range(3):
            assert_bits(got[j], want[j], f"kmeans thread {t} output {j} vs the restatement")

    calls = [lambda s=s: dc.kmeans(*s) for s in spec]
    return [dc], calls, check, calls


def partitioned_case(env):
    """tests/test_gpu_probed.py's main shape (n = 1237, d = 37, eight labels, segments of 1 .. 300
    rows) on ONE partitioned handle: two threads search it grouped, one probed with one label per
    row (nprobe = 1) and one with the main shape's lists (nprobe up to 8, repeats, empty labels)."""
    _, c, probes, cl = probed_.main_shape(37, 7)
    dc = _native.DeviceCorpus(c)
    part = dc.partition(cl, 8)
    m = len(probes)
    rs = np.random.RandomState(9)
    ql = [rs.randint(0, 8, size=m).astype(np.uint32) for _ in range(2)]
    ql[0][::9] = NONE
    one = [[int(g)] for g in rs.randint(0, 8, size=m)]
    qs = [randn(200 + t, m, 37) for t in range(T)]
    spec = [("grouped", ql[0], 10, COS), ("probed", one, 5, DOT), ("probed", probes, 10, EUC), ("grouped", ql[1], 20, EUC)]

    def call(t):
        kind, labels, k, metric = spec[t]
        if kind == "grouped":
            return part.topk_grouped(qs[t], labels, k, metric)
        po, pl = probed_.flat(labels)
        return part.topk_probed(qs[t], po, pl, k, metric)

    def check(t, got):
        kind, labels, k, metric = spec[t]
        if kind == "grouped":
            grouped_.assert_exact(got, grouped_.truth(qs[t], c, labels, cl, k, metric), k, f"grouped thread {t}")
        else:
            probed_.assert_exact(got, probed_.truth(qs[t], c, labels, cl, k, metric), k, f"probed thread {t}")

    calls = [lambda t=t: call(t) for t in range(T)]
    return [part, dc], calls, check, calls


def bits_corpus():
    """tests/test_gpu_bits.py's forced-overflow corpus: 3000 rows of 12 bytes drawn from 40 patterns,
    ordered farthest first from the first pattern -- every later chunk beats that query's buffer."""
    rs = np.random.RandomState(64)
    patterns = np.ascontiguousarray(rs.randint(0, 256, size=(40, 12)).astype(np.uint8))
    cb = np.ascontiguousarray(patterns[rs.randint(0, 40, size=3000)])
    far = bits_cpu.hamming_truth(patterns[:1], cb, 3000)[0][0][::-1]
    return np.ascontiguousarray(cb[far]), patterns, rs


def bits_case(env):
    """PMM_BITS_CAP=64 as tests/test_gpu_bits.py's overflow test: the first pattern's queries overflow
    their 64-entry buffers and are re-run (a read-back of the overflow count, a gather, a second
    search); their complements see the nearest rows first and stay on the native route.  Threads 0
    and 1 search one bit handle; threads 2 and 3 derive the sign bits of one f32 handle whose rows
    have exactly those bits, together, and search their own."""
    env.setenv("PMM_BITS_CAP", "64")
    cb, patterns, rs = bits_corpus()
    x = f32(np.unpackbits(cb, axis=1, bitorder="little").astype(np.float32) * 2 - 1)
    hb, dc, ref = _native.DeviceCorpus.bits(cb), _native.DeviceCorpus(x), _native.DeviceCorpus(x)
    near = np.ascontiguousarray(np.repeat(patterns[:1], 20, axis=0))
    qs = [near, np.ascontiguousarray(~near[:7]), np.ascontiguousarray(np.concatenate([near[:3], patterns[5:30]])),
          np.ascontiguousarray(~patterns[:33])]
    ks = [10, 10, 7, 3]

    def derive_and_search(parent, t):
        sb = parent.sign_bits()
        try:
            return (sb.bit_rows(),) + sb.topk(qs[t], ks[t])
        finally:
            sb.close()

    # the route of the two searches of the shared bit handle (the timing records are per thread)
    reruns = []
    _native.timing_enable(True)
    try:
        for t in range(2):
            _native.timing_reset()
            hb.topk(qs[t], ks[t])
            reruns.append(_native.timing_read("bits_gather")[1])
    finally:
        _native.timing_enable(False)
        _native.timing_reset()
    assert reruns[0] >= 1 and reruns[1] == 0, f"re-run launches of threads 0 and 1: {reruns}"

    def check(t, got):
        if t >= 2:
            assert np.array_equal(got[0], cb), f"thread {t}: sign_bits() rows are not pack_sign's"
            got = got[1:]
        want = bits_cpu.hamming_truth(qs[t], cb, ks[t])
        assert got[0].dtype == np.uint32 and got[1].dtype == np.float64
        assert_bits(got, want, f"bits thread {t} vs the restatement")

    # the serial results of threads 2 and 3 come from a second, identical f32 handle: on ``dc`` the
    # two threads' sign_bits() are the first ever, made together
    both = [lambda: hb.topk(qs[0], ks[0]), lambda: hb.topk(qs[1], ks[1])]
    calls = both + [lambda: derive_and_search(dc, 2), lambda: derive_and_search(dc, 3)]
    serial_calls = both + [lambda: derive_and_search(ref, 2), lambda: derive_and_search(ref, 3)]
    return [hb, dc, ref], calls, check, serial_calls


CASES = {"range": range_case, "self_plain": self_case, "self_derived": lambda env: self_case(env, True),
         "candidates": candidates_case, "maxsim_d37": maxsim_case, "maxsim_d130": lambda env: maxsim_case(env, 130),
         "kmeans": kmeans_case, "grouped_probed": partitioned_case, "bits": bits_case}


def close_all(handles):
    for h in handles:
        h.close()


# ---------------------------------------------------------------------------
# 1a. One entry, one shared handle, different arguments per thread
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_one_entry_four_threads_different_arguments(env, name):
    handles, calls, check, serial_calls = CASES[name](env)
    try:
        serial = [c() for c in serial_calls]
        for t, res in enumerate(serial):
            check(t, res)
        assert len({frozen(s) for s in serial}) == T, "two threads expect the same bytes: a swap would not show"
        threaded_equals_serial(calls, serial, name)
    finally:
        close_all(handles)


# ---------------------------------------------------------------------------
# 1b. Different entries at once on one parent
# ---------------------------------------------------------------------------
def test_six_entries_at_once_on_one_parent(env):
    """tests/test_gpu_dirty_scratch.py's screened handle shape (70 x 3037 x 256, k = 10 under
    PMM_F32_SCREEN=1): the first cosine top-k builds the handle's bf16 image and publishes it while
    five other entries read the same rows; the image is built and accounted once."""
    env.setenv("PMM_F32_SCREEN", "1")
    n, d, k = 3037, 256, 10
    c = randn(77, n, d)
    q = randn(78, 70, d)
    rs = np.random.RandomState(79)
    mask = rs.rand(n) < 0.4
    mask[[0, n - 1]] = True
    sel = np.flatnonzero(mask).astype(np.uint32)
    labels = rs.randint(0, 8, size=n).astype(np.uint32)
    labels[::50] = NONE
    probes = [rs.randint(0, 8, size=rs.randint(1, 4)).tolist() for _ in range(33)]
    po, pl = probed_.flat(probes)
    co, ci = cand_.lists([0, 1, 64, 129, 300, n, 40], n, 80)
    init = kc.default_init(c, 8, 1)
    full = sc_.ranked_self(c, COS)
    thr = float(np.sort(full[1][np.isfinite(full[1])])[-(n + 4000)])  # about 2000 pairs besides the diagonal

    def entries(dc):
        def subset_search():
            sub = dc.subset(mask)
            try:
                return sub.topk(q[:33], k, EUC)
            finally:
                sub.close()

        def partition_search():
            part = dc.partition(labels, 8)
            try:
                return part.topk_probed(q[:33], po, pl, k, DOT)
            finally:
                part.close()

        return [lambda: dc.topk(q, k, COS), lambda: dc.range_self(thr, COS), lambda: dc.kmeans(init, EUC, 3),
                subset_search, partition_search, lambda: dc.topk_candidates(q[:7], co, ci, k, DOT)]

    ref, shared = _native.DeviceCorpus(c), _native.DeviceCorpus(c)
    try:
        before = ref.nbytes
        serial = [call() for call in entries(ref)]
        assert ref.nbytes > before, "the handle built no screen image: the top-k did not screen"
        # the serial results against the definitions
        oi, osc = oracle.topk(q, c, k, oracle.COSINE)
        assert_bits(serial[0], (np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(np.float32)), "screened top-k vs oracle")
        sc_.assert_same_csr(serial[1], sc_.range_self_truth(full, thr, COS), "range_self")
        want = kc.kmeans_ref(c, init, EUC, 3)
        assert serial[2][3] == want[3] and bool(serial[2][4]) == want[4]
        for j in range(3):
            assert_bits(serial[2][j], want[j], f"kmeans output {j} vs the restatement")
        oi, osc = oracle.topk(q[:33], f32(c[sel]), k, oracle.EUCLIDEAN)
        assert_bits(serial[3], (sel[np.asarray(oi).astype(np.int64)], np.asarray(osc).astype(np.float32)), "subset top-k vs oracle")
        probed_.assert_exact(serial[4], probed_.truth(q[:33], c, probes, labels, k, DOT), k, "partition + probed")
        cand_.assert_same(serial[5], cand_.truth(q[:7], c, co, ci, k, DOT), "candidates")
        # the same six calls at once on a fresh handle: the image is built during the run
        assert shared.nbytes == before
        threaded_equals_serial(entries(shared), serial, "six entries")
        assert shared.nbytes == ref.nbytes, "the shared handle's image was not built and accounted exactly once"
    finally:
        ref.close()
        shared.close()


# ---------------------------------------------------------------------------
# 1c. close() while a call is in flight
# ---------------------------------------------------------------------------
def search_while(call, act):
    """tests/test_gpu_bf16_corpus.py's pattern, bounded: one thread repeats ``call`` (at most 20
    times, until it is refused); once its first call has returned, ``act()`` runs here.  Returns
    (the completed results, the refusals' texts)."""
    started = threading.Event()
    done, errors, other = [], [], []

    def searcher():
        try:
            for _ in range(20):
                try:
                    done.append(call())
                except RuntimeError as e:
                    if isinstance(e, _native.PmmError):
                        raise
                    errors.append(str(e))
                    break
                finally:
                    started.set()
        except BaseException as e:  # noqa: BLE001 - reported on the main thread
            other.append(repr(e))
            started.set()

    th = threading.Thread(target=searcher)
    th.start()
    assert started.wait(timeout=JOIN)
    act()
    th.join(timeout=JOIN)
    assert not th.is_alive(), "the searching thread is still running"
    assert not other, other
    return done, errors


@pytest.mark.parametrize("name,thread", [("range", 0), ("self_plain", 0), ("self_plain", 1), ("kmeans", 0), ("candidates", 1),
                                         ("maxsim_d37", 1), ("grouped_probed", 0), ("grouped_probed", 2), ("bits", 0)],
                         ids=["range", "range_self", "topk_self", "kmeans", "topk_candidates", "topk_maxsim",
                              "topk_grouped", "topk_probed", "bits_topk"])
def test_close_while_the_call_is_in_flight(env, name, thread):
    """The searched handle is closed from another thread: every call that had acquired it completes
    with the serial bytes (compared with the definition in 1a), the next one is refused as a closed
    handle is today (RuntimeError "DeviceCorpus is closed"), and ``closed`` is true afterwards."""
    handles, calls, _, _ = CASES[name](env)
    try:
        call, target = calls[thread], handles[0]
        serial = call()
        done, errors = search_while(call, target.close)
        assert target.closed
        assert done and all(e == "DeviceCorpus is closed" for e in errors), errors
        for j, got in enumerate(done):
            assert_bits(got, serial, f"{name}: call {j}, closed while searching")
        with pytest.raises(RuntimeError, match="DeviceCorpus is closed"):
            call()
        target.close()  # idempotent
    finally:
        close_all(handles)


@pytest.mark.parametrize("kind", ["subset", "partition"])
def test_parent_closed_while_a_derived_handle_is_searched(env, kind):
    """include/pmm.h: a subset and a partition are "independent of the parent (pmm_corpus_destroy
    frees it)".  The parent is closed -- nobody holds it, so it is destroyed at once -- while
    another thread searches the derived handle, which goes on serving the same bytes."""
    q, c, ql, cl = grouped_.main_shape(np.float32, 37, 5)
    mask = cl != NONE
    ids = np.flatnonzero(mask).astype(np.uint32)
    dc = _native.DeviceCorpus(c)
    der = dc.subset(mask) if kind == "subset" else dc.partition(cl, 8)
    try:
        call = (lambda: der.topk(q, 10, COS)) if kind == "subset" else (lambda: der.topk_grouped(q, ql, 10, COS))
        serial = call()
        if kind == "subset":
            oi, osc = oracle.topk(q, f32(c[ids]), 10, oracle.COSINE)
            assert_bits(serial, (ids[np.asarray(oi).astype(np.int64)], np.asarray(osc).astype(np.float32)), "subset vs oracle")
        else:
            grouped_.assert_exact(serial, grouped_.truth(q, c, ql, cl, 10, COS), 10, "grouped")
        done, errors = search_while(call, dc.close)
        assert dc.closed and not der.closed
        assert len(done) == 20 and not errors, (len(done), errors)
        for j, got in enumerate(done):
            assert_bits(got, serial, f"{kind}: call {j}, parent closed while searching")
        assert_bits(call(), serial, f"{kind}: after the parent is gone")
    finally:
        der.close()
        dc.close()


# ---------------------------------------------------------------------------
# 1d. Errors stay on their thread
# ---------------------------------------------------------------------------
def test_argument_errors_stay_on_their_thread(env):
    """Two threads make calls the library refuses for their arguments, two search.  Every refusal
    carries its own code and text; the searches return the serial bytes and their threads' own
    pmm_last_error() is still empty (the message is thread-local in the library)."""
    handles, calls, _, _ = CASES["grouped_probed"](env)
    part, dc = handles
    mv_handles = maxsim_case(env)[0]
    try:
        q = randn(1, 5, 37)
        offsets, down = np.array([0, 2, 2, 2, 2, 2], dtype=np.int64), np.array([5, 4], dtype=np.uint32)
        qt = randn(2, 3, 37)
        qo, co, ci = np.array([0, 3], np.int64), np.array([0, 2], np.int64), np.array([0, 1], np.uint32)
        po = np.arange(6, dtype=np.int64)
        failing = [
            [(lambda: dc.range(q, float("nan"), COS), "the range threshold is NaN"),
             (lambda: part.topk_probed(q, po, np.array([0, 1, 8, 2, 3], np.uint32), 3, COS), "query row 2")],
            [(lambda: dc.topk_candidates(q, offsets, down, 2, DOT), "strictly ascending within a row"),
             (lambda: mv_handles[0].topk_maxsim(qt, qo, co, ci, 1, EUC), "MaxSim takes cosine or dot")],
        ]
        searching = [calls[0], calls[2]]
        serial = [c() for c in searching]

        def fail(t):
            def work(r):
                call, text = failing[t][r]
                with pytest.raises(_native.PmmError) as ei:
                    call()
                assert ei.value.code == _native.PMM_ERR_ARG and text in str(ei.value), (t, r, str(ei.value))
                assert text in _native.last_error()
                return None
            return work

        def search(t):
            def work(r):
                got = searching[t]()
                return got, _native.last_error()
            return work

        got = run_threads([fail(0), fail(1), search(0), search(1)], ROUNDS)
        for t in (0, 1):
            for r in range(ROUNDS):
                res, last = got[2 + t][r]
                assert_bits(res, serial[t], f"searching thread {t} round {r}")
                assert last == "", f"searching thread {t} reads another thread's error: {last!r}"
    finally:
        close_all(handles + mv_handles)


# ---------------------------------------------------------------------------
# 1e. Three shards on one device, under threads
# ---------------------------------------------------------------------------
def test_three_shards_on_one_device_under_threads(env, device_list):
    """set_devices([0, 0, 0]) as tests/test_gpu_dirty_scratch.py: two threads search one sharded f32
    handle -- ``topk`` with different k and metric, and the sharded host entry -- and get the bytes
    of one device.  ``topk`` is the entry a sharded handle serves: range, self and candidate search
    take a handle of one shard (include/pmm.h) and the third thread gets PMM_ERR_UNSUPPORTED from
    each of them, every time, with the shard count in the text."""
    n, d = 3001, 40
    c, qs = randn(130, n, d), [randn(131 + t, 33 + t, d) for t in range(2)]
    c[2100] = c[3]  # a tie across shards
    args = [(10, COS), (44, EUC)]
    _native.set_devices([])
    one = [_native.topk_host(qs[t], c, *args[t]) for t in range(2)]
    for t in range(2):
        oi, osc = oracle.topk(qs[t], c, args[t][0], {COS: oracle.COSINE, EUC: oracle.EUCLIDEAN}[args[t][1]])
        assert_bits(one[t], (np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(np.float32)), f"one device {t} vs oracle")
    _native.set_devices([0, 0, 0])
    dc = _native.DeviceCorpus(c)
    try:
        assert dc.shards == 3
        offsets, ids = np.array([0, 2], np.int64), np.array([1, 2], np.uint32)
        refused = [lambda: dc.range(qs[0][:1], 0.5, COS), lambda: dc.range_self(0.5, COS), lambda: dc.topk_self(3, COS),
                   lambda: dc.topk_candidates(qs[0][:1], offsets, ids, 1, COS)]

        def search(t):
            return lambda r: dc.topk(qs[t], *args[t]) + _native.topk_host(qs[t], c, *args[t])

        def unsupported(r):
            for call in refused:
                with pytest.raises(_native.PmmError) as ei:
                    call()
                assert ei.value.code == _native.PMM_ERR_UNSUPPORTED and "3 shards" in str(ei.value), str(ei.value)

        got = run_threads([search(0), search(1), unsupported], ROUNDS)
        for t in range(2):
            for r in range(ROUNDS):
                assert_bits(got[t][r][:2], one[t], f"sharded handle, thread {t} round {r}")
                assert_bits(got[t][r][2:], one[t], f"sharded host entry, thread {t} round {r}")
    finally:
        _native.set_devices([])
        dc.close()


# ---------------------------------------------------------------------------
# 2. The Python corpus cache under threads (pyarrow inputs, as the feature tests)
# ---------------------------------------------------------------------------
def arrow_rows(a):
    return pa.FixedSizeListArray.from_arrays(pa.array(a.reshape(-1)), a.shape[1])


def cache_corpus(seed, n=4111, d=64):
    """tests/test_gpu_probed.py's cached shape: 4111 x 64 f32 is just past _CACHE_MIN_BYTES (1 MiB)."""
    c = randn(seed, n, d)
    assert c.nbytes >= pm._CACHE_MIN_BYTES
    return c, arrow_rows(c)


def topk_lists(out, m, k):
    """(idx (m, k), f32 score bits) of ``_topk``'s column."""
    off, idx, bits_ = arrow_parts(out)
    assert np.array_equal(off, np.arange(m + 1) * k)
    return idx.reshape(m, k), bits_.view(np.float64).astype(np.float32).reshape(m, k)


@pytest.mark.parametrize("form", ["plain", "subset", "groups", "maxsim"])
def test_cold_cache_four_threads_make_one_entry(env, clean_cache, form):
    m, k = 23, 10
    c, ac = cache_corpus(61)
    q = randn(62, m, 64)
    aq = arrow_rows(q)
    rs = np.random.RandomState(63)
    if form == "plain":
        call = lambda: pm._topk(aq, ac, k, "dot")  # noqa: E731
        oi, osc = oracle.topk(q, c, k, oracle.DOT)
        want, extra = (np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(np.float32)), None
    elif form == "subset":
        mask = rs.rand(c.shape[0]) < 0.5
        amask = pa.array(mask)
        call = lambda: pm._topk(aq, ac, k, "dot", subset=amask)  # noqa: E731
        ids = np.flatnonzero(mask).astype(np.uint32)
        oi, osc = oracle.topk(q, f32(c[ids]), k, oracle.DOT)
        want, extra = (ids[np.asarray(oi).astype(np.int64)], np.asarray(osc).astype(np.float32)), "subset"
    elif form == "groups":
        cl = rs.randint(0, 4, size=c.shape[0]).astype(np.uint32)
        probes = [rs.randint(0, 4, size=rs.randint(1, 4)).tolist() for _ in range(m)]
        al = pa.array([[int(x) for x in p] for p in probes], type=pa.list_(pa.int64()))
        acl = pa.array(cl.astype(np.int64))
        call = lambda: pm._topk(aq, ac, k, "dot", groups=(al, acl))  # noqa: E731
        want, extra = probed_.truth(q, c, probes, cl, k, DOT), "groups"
    else:
        nd = 300  # 300 documents of 7 tokens, d = 128: 2100 x 128 f32 token rows, past _CACHE_MIN_BYTES
        do = np.arange(nd + 1, dtype=np.int64) * 7
        dt = randn(64, nd * 7, 128)
        qo = maxsim_.offsets_of([3, 1, 9, 5])
        qt = randn(65, int(qo[-1]), 128)
        co, ci = maxsim_.lists([40, 0, 129, 7], nd, 66)
        docs = pa.LargeListArray.from_arrays(pa.array(do), arrow_rows(dt))
        queries = pa.LargeListArray.from_arrays(pa.array(qo), arrow_rows(qt))
        lists = pa.LargeListArray.from_arrays(pa.array(co), pa.array(ci.astype(np.int64)))
        call = lambda: pm._topk_maxsim(queries, docs, k, "cosine", candidates=lists)  # noqa: E731
        want, extra = maxsim_.truth(maxsim_.pair_scores(qt, qo, dt, do, COS), qo, co, ci, k), None
    serial = call()
    # the serial result against the definition
    if form in ("plain", "subset"):
        assert_bits(topk_lists(serial, m, k), want, f"{form} vs oracle")
    elif form == "groups":
        probed_.assert_lists(probed_.ragged(serial), want, "groups vs oracle")
    else:
        off, idx, bits_ = arrow_parts(serial)
        assert np.array_equal(np.diff(off), want[2])
        for i in range(4):
            assert np.array_equal(idx[off[i]:off[i + 1]], want[0][i, :want[2][i]])
            assert np.array_equal(bits_[off[i]:off[i + 1]].view(np.float64).astype(np.float32).view(np.uint32),
                                  want[1][i, :want[2][i]].view(np.uint32))
    assert len(pm._cache) == (2 if extra else 1)
    was_cached = [v[1] for v in pm._cache.values()]
    pm.clear_corpus_cache()  # cold again: the four threads race for the lock and for the first upload
    threaded_equals_serial([call] * T, [serial] * T, f"cold cache, {form}")
    assert len(pm._cache) == (2 if extra else 1), list(pm._cache)
    assert len([key for key in pm._cache if extra in key]) == 1 if extra else True
    # every caller has released what the cache handed it: clearing destroys each handle at once
    was_cached += [v[1] for v in pm._cache.values()]
    pm.clear_corpus_cache()
    assert all(dc.closed for dc in was_cached), [dc.closed for dc in was_cached]


def test_other_cached_paths_from_two_threads(env, clean_cache):
    """``_within``, ``_within_self``, ``_topk_self``, ``_kmeans_labels`` on one cached f32 column and
    ``_topk_hamming`` on one cached bit column, two threads each with arguments of their own."""
    x, _, _ = kc.planted(4111, 64, 16, 9, noise=2.0)
    ax = arrow_rows(x)
    q = [randn(91 + t, 9 + t, 64) for t in range(2)]
    handle = _native.DeviceCorpus(x)
    try:
        thr = [float(np.quantile(range_.ranked(q[t], x, metric)[1], 0.99 if metric == COS else 0.01))
               for t, metric in enumerate((COS, EUC))]
        full = sc_.ranked_self(x, COS)
        self_thr = float(np.sort(full[1][np.isfinite(full[1])])[-(4111 + 3000)])
        cb = np.ascontiguousarray(np.random.RandomState(93).randint(0, 256, size=(16411, 64)).astype(np.uint8))
        acb = arrow_rows(cb)
        qb = [np.ascontiguousarray(np.random.RandomState(94 + t).randint(0, 256, size=(5 + t, 64)).astype(np.uint8))
              for t in range(2)]
        assert cb.nbytes >= pm._CACHE_MIN_BYTES
        paths = {
            "within": [lambda t=t, metric=metric: pm._within(arrow_rows(q[t]), ax, thr[t], NAME[metric])
                       for t, metric in enumerate((COS, EUC))],
            "within_self": [lambda: pm._within_self(ax, self_thr, "cosine"), lambda: pm._within_self(ax, 1.0, "euclidean")],
            "topk_self": [lambda: pm._topk_self(ax, 5, "cosine"), lambda: pm._topk_self(ax, 12, "dot")],
            "kmeans_labels": [lambda: pm._kmeans_labels(ax, 5, "euclidean", max_iter=4, seed=1),
                              lambda: pm._kmeans_labels(ax, 16, "cosine", max_iter=3, seed=2)],
            "topk_hamming": [lambda t=t: pm._topk_hamming(arrow_rows(qb[t]), acb, 10 + t) for t in range(2)],
        }
        # every serial result equals the handle's (compared with the definitions in 1a) or the restatement
        handle_level = {
            "within": [lambda t=t, metric=metric: handle.range(q[t], thr[t], metric) for t, metric in enumerate((COS, EUC))],
            "within_self": [lambda: handle.range_self(self_thr, COS), lambda: handle.range_self(1.0, EUC)],
            "topk_self": [lambda: handle.topk_self(5, COS), lambda: handle.topk_self(12, DOT)],
        }
        for name, calls in paths.items():
            serial = [c() for c in calls]
            for t in range(2):
                if name in ("within", "within_self"):
                    o, i, s = handle_level[name][t]()
                    assert_bits(arrow_parts(serial[t]), (o, i, s.astype(np.float64).view(np.uint64)), f"{name} {t} vs the handle")
                elif name == "topk_self":
                    i, s = handle_level[name][t]()
                    assert_bits(arrow_parts(serial[t])[1:], (i.reshape(-1), s.astype(np.float64).reshape(-1).view(np.uint64)),
                                f"{name} {t} vs the handle")
                elif name == "kmeans_labels":
                    K, metric, it, seed = [(5, EUC, 4, 1), (16, COS, 3, 2)][t]
                    want = kc.kmeans_ref(x, kc.default_init(x, K, seed), metric, it)
                    assert np.array_equal(np.asarray(serial[t].to_numpy(zero_copy_only=False)), want[1]), f"{name} {t}"
                else:
                    wi, ws = bits_cpu.hamming_truth(qb[t], cb, 10 + t)
                    assert_bits(arrow_parts(serial[t])[1:], (wi.reshape(-1), ws.reshape(-1).view(np.uint64)), f"{name} {t}")
            assert frozen(serial[0]) != frozen(serial[1])
            got = run_threads([lambda r, c=c: c() for c in calls], ROUNDS)
            for t in range(2):
                for r in range(ROUNDS):
                    assert_bits(got[t][r], serial[t], f"{name}: thread {t} round {r}")
        assert len(pm._cache) == 2, list(pm._cache)  # the f32 column and the bit column, once each
    finally:
        handle.close()
