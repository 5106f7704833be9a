"""The host-only planners and validators under threads (include/pmm.h: "every
entry point may be called concurrently from different threads";
pmm_last_error() is "the last failing call on this thread").

Eight threads, each with arguments of its own, 200 calls each, released by one
barrier.  Every result is compared with the same call made serially before the
threads start -- and that serial result once with the restatement its feature
test already has -- and every failing call must carry the message of its OWN
arguments: the error text is thread-local in the library (``t_err``), so a
thread that read another's would name another's sizes.  No GPU.
"""
from __future__ import annotations

import numpy as np
import pytest

import test_probed_cpu as probed_cpu
import test_sort_plan as sort_plan_tests
from concurrency_cases import frozen, run_threads
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

T = 8
CALLS = 200
NONE = _native.NO_GROUP
COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN


def outcome(call):
    """("ok", result) or ("error", type, code, message) of call()."""
    try:
        return ("ok", frozen(call()))
    except (_native.PmmError, ValueError, TypeError, RuntimeError) as e:
        return ("error", type(e).__name__, getattr(e, "code", None), str(e))


def hammer(jobs):
    """jobs[t]: the calls of thread t (each a function without arguments, good
    and failing ones mixed).  Their serial outcomes are taken first; then T
    threads run their own calls round-robin, CALLS calls each, in the shared
    frame.  Returns the serial outcomes; asserts that every threaded one
    equals its own."""
    assert len(jobs) == T
    serial = [[outcome(c) for c in mine] for mine in jobs]

    def work(t):
        def call(j):
            i = j % len(jobs[t])
            got = outcome(jobs[t][i])
            assert got == serial[t][i], f"thread {t} call {j}: {got[:1] + got[1:][:3]} != {serial[t][i][:4]}"
        return call

    run_threads([work(t) for t in range(T)], CALLS)
    return serial


def failed_with(out, code, *texts):
    assert out[0] == "error" and out[2] == code, out
    for text in texts:
        assert text in out[3], (text, out[3])


def probe_case(t):
    rs = np.random.RandomState(400 + t)
    m, G = 20 + 7 * t, 4 + 3 * t
    sizes = rs.randint(0, 4, size=G) * rs.randint(1, 300, size=G)
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lens = rs.randint(0, 6, size=m)
    po = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pl = rs.randint(0, G, size=int(po[-1])).astype(np.uint32)
    pl[rs.rand(pl.size) < 0.1] = NONE
    return po, pl, goff, 3 + t


def test_probe_plan_from_eight_threads():
    cases = [probe_case(t) for t in range(T)]
    jobs = []
    for t, (po, pl, goff, k) in enumerate(cases):
        bad = pl.copy()
        at = t % bad.size
        bad[at] = 1000 + t  # no group: the message names this entry, this value and its row
        jobs.append([lambda a=(po, pl, goff, k): _native.probe_plan(*a),
                     lambda a=(po, bad, goff, k): _native.probe_plan(*a)])
    serial = hammer(jobs)
    for t, (po, pl, goff, k) in enumerate(cases):
        probed_cpu.assert_plan(po, pl, goff, k)  # the serial call against the restatement
        assert serial[t][0][0] == "ok"
        row = int(np.searchsorted(po, t % pl.size, side="right")) - 1
        failed_with(serial[t][1], _native.PMM_ERR_ARG, f"probe_labels[{t % pl.size}] = {1000 + t}", f"query row {row}")


def test_sort_plan_from_eight_threads():
    jobs, cases = [], []
    for t in range(T):
        smax = (128, 256, 8192, 1000)[t % 4]
        cap = (1, 100, 3 * 8192 + 1, sort_plan_tests.I64_MAX)[(t // 2) % 4]
        L = np.array(sort_plan_tests.lengths(smax), dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(np.roll(L, t))])
        cases.append((offsets, smax, cap))
        jobs.append([lambda a=(offsets, smax, cap): _native.sort_plan(*a),
                     lambda o=offsets, t=t: _native.sort_plan(o, 100 + t, 7 + t)])  # smax below the wave tier
    serial = hammer(jobs)
    for t, (offsets, smax, cap) in enumerate(cases):
        got = _native.sort_plan(offsets, smax, cap)
        want = sort_plan_tests.restated(offsets, smax, cap)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert all(np.array_equal(got[3][name], want[3][name]) for name in _native.SORT_PIECE.names)
        assert got[4] == want[4] and serial[t][0][0] == "ok"
        failed_with(serial[t][1], _native.PMM_ERR_ARG, f"smax={100 + t} cap={7 + t}")


def test_shard_and_self_plans_from_eight_threads():
    jobs = []
    for t in range(T):
        devs = [0, 1, 0, 2][:1 + t % 4]
        shape = (64 + t, 5000 + 97 * t, 37 + 8 * t, 10 + t, (COS, DOT, EUC)[t % 3])
        jobs.append([lambda d=devs, s=shape: _native.shard_plan(d, *s),
                     lambda d=devs, s=shape: _native.shard_plan(d, *s, compute=_native.COMPUTE_BF16, host_rows=False),
                     lambda t=t: _native.shard_plan([0, 1], 7 + t, 1, 300 + t, 10, COS),  # fewer rows than shards
                     lambda t=t: _native.range_self_plan(300 + 129 * t, 8 + 31 * t),
                     lambda t=t: _native.range_self_plan(1000 + t, 256, variant=(0, 3)[t % 2]),
                     lambda t=t: _native.range_self_plan(40 + t, 0)])  # no compute unit
    serial = hammer(jobs)
    for t in range(T):
        assert [o[0] for o in serial[t]] == ["ok", "ok", "error", "ok", "ok", "error"], serial[t]
        failed_with(serial[t][2], _native.PMM_ERR_ARG, f"m={7 + t} n=1 G=2 d={300 + t}")
        failed_with(serial[t][5], _native.PMM_ERR_ARG, f"n={40 + t} cus=0")
        # the self plan's own invariants (tests/test_self_plan.py): at least the triangle, at most the square
        variant, visits, full = _native.range_self_plan(300 + 129 * t, 8 + 31 * t)
        assert variant in (0, 3) and 0 < visits <= full
    # different device lists plan differently: the threads' results are not all one
    assert len({serial[t][0] for t in range(T)}) == T


def test_ascending_ids_and_validators_from_eight_threads():
    jobs, cases = [], []
    for t in range(T):
        rs = np.random.RandomState(500 + t)
        m, n = 5 + t, 200 + 13 * t
        ids = rs.randint(0, n, size=50 + t)
        mask = rs.rand(n) < 0.3
        mask[t] = True
        ql = rs.randint(0, 4, size=m).astype(np.int64)
        cl = rs.randint(0, 4, size=n).astype(np.int64)
        lens = rs.randint(0, 9, size=m)
        co = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ci = rs.randint(0, n, size=int(co[-1])).astype(np.int64)  # unsorted, with repeats: normalised
        bad_ci = ci.copy()
        if bad_ci.size == 0:
            co, ci, bad_ci = np.arange(m + 1, dtype=np.int64), np.arange(m, dtype=np.int64), np.arange(m, dtype=np.int64)
        bad_ci[-1] = n + t
        cases.append((m, n, ids, mask, co, ci))
        jobs.append([lambda a=(ids, n): _native.ascending_ids(*a),
                     lambda a=(np.append(ids, n + t), n): _native.ascending_ids(*a),
                     lambda a=(mask, n): pm._check_subset(*a),
                     lambda a=(ids, n): pm._check_subset(*a),
                     lambda a=(mask, n + 1 + t): pm._check_subset(*a),
                     lambda a=(np.append(ids, n + t), n): pm._check_subset(*a),
                     lambda a=((ql, cl), m, n): pm._check_groups(*a),
                     lambda a=((ql, cl), m + 1 + t, n): pm._check_groups(*a),
                     lambda a=((co, ci), m, n): pm._check_candidates(*a),
                     lambda a=((co, bad_ci), m, n): pm._check_candidates(*a)])
    serial = hammer(jobs)
    for t, (m, n, ids, mask, co, ci) in enumerate(cases):
        kinds = [o[0] for o in serial[t]]
        assert kinds == ["ok", "error", "ok", "ok", "error", "error", "ok", "error", "ok", "error"], kinds
        assert np.array_equal(_native.ascending_ids(ids, n), np.unique(ids).astype(np.uint32))
        assert pm._check_subset(mask, n).count == int(mask.sum())
        assert np.array_equal(pm._check_subset(ids, n).ids, np.unique(ids).astype(np.uint32))
        cand = pm._check_candidates((co, ci), m, n)
        for i in range(m):
            assert np.array_equal(cand.ids[cand.offsets[i]:cand.offsets[i + 1]], np.unique(ci[co[i]:co[i + 1]]))
        assert f"subset row id {n + t} is out of range for a corpus of {n} rows" in serial[t][1][3]
        assert f"subset mask has {n} rows, the corpus has {n + 1 + t}" in serial[t][4][3]
        assert f"subset row id {n + t} " in serial[t][5][3]
        assert f"left labels have {m} rows, the queries have {m + 1 + t}" in serial[t][7][3]
        assert f"hold the id {n + t}: not a row of the corpus ({n} rows)" in serial[t][9][3]


def test_a_failing_thread_leaves_the_others_last_error_alone():
    """pmm_last_error() is per thread: four threads fail over and over, four
    only succeed, and these still read "" -- their own last error -- at the end."""
    seen = {}

    def work(t):
        def call(j):
            if t % 2:
                with pytest.raises(_native.PmmError, match=f"cus=-{t}"):
                    _native.range_self_plan(100, -t)
            else:
                _native.range_self_plan(100 + j, 8)
            seen[t] = _native.last_error()
        return call

    run_threads([work(t) for t in range(T)], CALLS)
    for t in range(T):
        assert (f"cus=-{t}" in seen[t]) if t % 2 else seen[t] == "", (t, seen[t])
