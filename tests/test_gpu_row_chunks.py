"""The row-chunk loops of the materialised paths and the matmul entries, past their first chunk
(PMM_MATERIALISE_BUDGET; the table is tests/row_chunk_cases.py).

Every case runs three ways: with the knob unset (one chunk), with the budget at R * per_row for
each listed R (chunks of R rows), and on the CPU oracle.  The comparison is of bits: a knob run
equals the unset run byte for byte, and the unset run equals the oracle -- the same indices, the
same score bits, NaN where the oracle has NaN.  Every knob run also reads the launch count of the
chunked GEMM from the timing records (gemm_f32_matmul, gemm_f64_matmul, gemm_f32_scores,
gemm_f64_scores; select_f64_rows on the f64 row select) and asserts ceil(m / R): a case that ran
as one chunk fails on the count, whatever its values.

What a second chunk changes, and the rows that would show it: the shifted query rows and norms
(every query row is distinct; the starred rows of the second chunks see exact ties at the k-th
place, a NaN row and a zero-norm row), the shifted output rows, the score block and the tile
counter reused while the previous chunk's select or copy is in flight, and the sign pass of zero
scores (the matmul entries run it per chunk on shifted pointers: planted -0.0 sums and all-zero
query rows in the second and the last chunk).

Two runs use the real budget with the knob unset: f32 1030 x 524288 x 8, whose first chunk is
exactly 2^31 bytes and whose second has 6 rows that repeat rows 0 .. 5.

The sharded re-run runs on one device listed twice, as
tests/test_gpu_host_frame.py::test_f64_overflowed_shards_rerun_after_every_device does.

Power, shown once on scratch builds with one in-bounds mutation each (not committed):
  qn + r0 -> qn (both materialised executors)        17 of 31 tests fail: every cosine and euclidean
                                                     case of the host, device and handle tests and the
                                                     extension test (dot reads no norms; the full-size
                                                     run's second chunk repeats rows 0 .. 5, whose
                                                     norms the mutation reads)
  out_idx + r0 * k -> out_idx (and oi + r0 * k)      25 fail: every top-k test but the sharded re-run
                                                     (its rows share one index list), with the full-size
                                                     top-k
  out + r0 * n -> out (both matmul entries)          6 fail: the four matmul cases, the extension test,
                                                     the full-size matmul

Wall time on an MI355X: 14 s for the module's 31 tests, 11.7 s of it the process's first use of
torch in the f32 device-entry test; every other test is under 0.5 s, the two full-size runs
included (they stay in this module).
"""
from __future__ import annotations

import contextlib
import functools
import os
import time

import numpy as np
import pytest

import oracle
import row_chunk_cases as rc
from polars_matmul import _native
from row_chunk_cases import KNOB
from test_gpu_dirty_scratch import assert_same, roundup

pytestmark = pytest.mark.gpu


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


@contextlib.contextmanager
def launch_records():
    """Inside: launches(label) is the number of launches recorded since entry."""
    _native.timing_reset()
    _native.timing_enable(True)
    try:
        yield lambda label: _native.timing_read(label)[1]
    finally:
        _native.timing_enable(False)
        _native.timing_reset()


def assert_oracle_bits(got, want, label):
    """Arrays of one dtype: equal bits, or NaN on both sides."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{label}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"
    u = f"u{got.dtype.itemsize}"
    same = got.view(u) == want.view(u)
    if got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    if not same.all():
        at = np.argwhere(~same)[0]
        raise AssertionError(f"{label}: {int((~same).sum())} of {same.size} entries differ from the oracle, first at "
                             f"{tuple(int(x) for x in at)}: {got[tuple(at)]!r} != {want[tuple(at)]!r}")


@functools.lru_cache(maxsize=None)
def oracle_matmul(case):
    q, c = case.data()
    return np.asarray(oracle.matmul(q, c)).astype(case.dtype)


@functools.lru_cache(maxsize=None)
def oracle_topk(case, metric, k):
    q, c = case.data(metric, k)
    idx, sc = oracle.topk(q, c, k, metric)
    return np.asarray(idx).astype(np.uint32), np.asarray(sc).astype(case.dtype)


def assert_lists(got, case, metric, k, label, index_base=0):
    oi, osc = oracle_topk(case, metric, k)
    assert_oracle_bits(np.asarray(got[0]).view(np.uint32), oi + np.uint32(index_base), f"{label} indices")
    assert_oracle_bits(got[1], osc, f"{label} scores")


def chunked_runs(env, case, k, call, label, check_unset, extra_labels=(), launches_per_chunk=1, row_bytes=None):
    """call() with the knob unset (one launch of the chunked GEMM), checked by check_unset, then
    under every listed R: the unset run's bytes and ceil(m / R) launches."""
    for name, value in case.env.items():
        env.setenv(name, value)
    row_bytes = row_bytes or case.per_row(k)
    env.delenv(KNOB, raising=False)
    with launch_records() as launches:
        want = call()
        assert launches(case.label) == launches_per_chunk, f"{label}: {launches(case.label)} launches with the knob unset"
    check_unset(want)
    for r in case.rows:
        env.setenv(KNOB, rc.budget_of(r, row_bytes))
        with launch_records() as launches:
            got = call()
            counts = {nm: launches(nm) for nm in (case.label,) + tuple(extra_labels)}
        expect = rc.chunks(case.m, r) * launches_per_chunk
        assert counts == {nm: expect for nm in counts}, f"{label} R={r}: launches {counts}, {expect} chunks planned"
        assert_same(got, want, f"{label} R={r} against the knob unset")
    env.delenv(KNOB)
    return want


def topk_params(cases):
    return [pytest.param(c, metric, k, id=f"{c.name}-metric{metric}-k{k}") for c in cases for metric in c.metrics
            for k in c.ks]


# ---------------------------------------------------------------------------
# The host entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.MATMUL_CASES, ids=repr)
def test_matmul_in_row_chunks(env, case):
    q, c = case.data()
    chunked_runs(env, case, None, lambda: (np.array(_native.matmul_host(q, c)),), case.name,
                 lambda want: assert_oracle_bits(want[0], oracle_matmul(case), case.name))


@pytest.mark.parametrize("case,metric,k", topk_params(rc.TOPK_CASES))
def test_topk_in_row_chunks(env, case, metric, k):
    q, c = case.data(metric, k)
    label = f"{case.name} metric={metric} k={k}"
    extra = ("select_f64_rows",) if case.dtype == np.float64 and not rc.global_sort(k) else ()
    chunked_runs(env, case, k, lambda: _native.topk_host(q, c, k, metric), label,
                 lambda want: assert_lists(want, case, metric, k, label), extra_labels=extra)


def test_f64_fused_overflow_falls_back_in_row_chunks(env):
    """The fused scan overflows on the ascending corpus and the call is redone materialised in the
    same workspace: with the knob in 4 and in 6 chunks."""
    case, (metric,), (k,) = rc.F64_FALLBACK, rc.F64_FALLBACK.metrics, rc.F64_FALLBACK.ks
    q, c = case.data(metric, k)

    def call():
        with launch_records() as launches:
            out = _native.topk_host(q, c, k, metric)
            assert launches("gemm_f64_topk") >= 1, "the call did not start on the fused scan"
            call.reruns.append(launches(case.label))
        return out

    call.reruns = []

    def check(want):
        assert want[0].tolist() == [list(range(case.n - 1, case.n - 1 - k, -1))] * case.m
        assert_lists(want, case, metric, k, case.name)

    for name, value in case.env.items():
        env.setenv(name, value)
    want = call()
    check(want)
    for r in case.rows:
        env.setenv(KNOB, case.budget(r, k))
        assert_same(call(), want, f"{case.name} R={r} against the knob unset")
    assert call.reruns == [1] + [rc.chunks(case.m, r) for r in case.rows] and min(call.reruns[1:]) > 1, call.reruns


def test_f64_overflowed_shards_rerun_in_row_chunks(env, device_list):
    """Two shards (one device listed twice) overflow and are re-run materialised after every
    device has finished: each re-run in chunks of R rows of its own 2000-row shard."""
    case, (metric,), (k,) = rc.F64_SHARDED, rc.F64_SHARDED.metrics, rc.F64_SHARDED.ks
    q, c = case.data(metric, k)
    for name, value in case.env.items():
        env.setenv(name, value)
    want = _native.topk_host(q, c, k, metric)
    assert_lists(want, case, metric, k, f"{case.name}, one device")
    _native.set_devices([0] * rc.SHARDS)
    for r in (case.m,) + case.rows:
        env.setenv(KNOB, rc.budget_of(r, rc.per_row(rc.shard_rows(case), 8, k)))
        with launch_records() as launches:
            got = _native.topk_host(q, c, k, metric)
            fused, rerun, merges = launches("gemm_f64_topk"), launches(case.label), launches("merge_devices_f64")
        assert fused >= 2 * rc.SHARDS and merges == 1, (fused, merges)
        assert rerun == rc.SHARDS * rc.chunks(case.m, r), f"R={r}: {rerun} score launches"
        assert_same(got, want, f"{case.name} R={r} against one device")


# ---------------------------------------------------------------------------
# The device entries and the handles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [rc.F32_DEVICE, rc.F64_DEVICE], ids=repr)
def test_device_entry_with_index_base_in_row_chunks(env, case):
    import torch

    (metric,), (k,) = case.metrics, case.ks
    f64 = case.dtype == np.float64
    q, c = case.data(metric, k)
    m, n, d = case.m, case.n, case.d
    dt = torch.float64 if f64 else torch.float32
    # row strides above the padded d, each its own
    ldq, ldc = roundup(d, 16 if f64 else 32) + (6 if f64 else 36), roundup(d, 16 if f64 else 32) + (2 if f64 else 4)
    dev = torch.device("cuda:0")
    tq, tc = torch.zeros((m, ldq), dtype=dt, device=dev), torch.zeros((n, ldc), dtype=dt, device=dev)
    tq[:, :d], tc[:, :d] = torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(np.array(c)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        oi = torch.full((m, k), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        osc = torch.full((m, k), 123.0, dtype=dt, device=dev)
        if f64:
            _native.topk_f64_device(tq.data_ptr(), ldq, m, tc.data_ptr(), ldc, n, d, k, metric, oi.data_ptr(),
                                    osc.data_ptr(), index_base=rc.INDEX_BASE, stream=stream)
        else:
            # a caller's workspace of exactly the bytes the sizer names under the same knob, poisoned
            wb = _native.workspace_bytes(m, n, d, k, metric)
            ws = torch.full((wb,), 0xFF, dtype=torch.uint8, device=dev)
            _native.topk_device(tq.data_ptr(), ldq, m, tc.data_ptr(), ldc, n, d, k, metric, oi.data_ptr(), osc.data_ptr(),
                                index_base=rc.INDEX_BASE, workspace=ws.data_ptr(), workspace_bytes=wb, stream=stream)
        torch.cuda.synchronize()
        return oi.cpu().numpy().view(np.uint32), osc.cpu().numpy()

    extra = ("select_f64_rows",) if f64 else ()
    chunked_runs(env, case, k, call, case.name,
                 lambda want: assert_lists(want, case, metric, k, case.name, index_base=rc.INDEX_BASE), extra_labels=extra)


@pytest.mark.parametrize("case,metric,k", topk_params([rc.F32_HANDLE, rc.F64_HANDLE]))
def test_handle_in_row_chunks(env, case, metric, k):
    """A resident corpus with its norms computed at creation (c_norms on the f32 executor, cn_pre
    on the f64 one): multi-chunk calls equal the one-chunk call, the host entry and the oracle."""
    q, c = case.data(metric, k)
    label = f"{case.name} metric={metric}"
    dc = _native.DeviceCorpus(np.array(c))
    try:
        extra = ("select_f64_rows",) if case.dtype == np.float64 else ()
        want = chunked_runs(env, case, k, lambda: dc.topk(q, k, metric), label,
                            lambda want: assert_lists(want, case, metric, k, label), extra_labels=extra)
        env.setenv(KNOB, case.budget(case.rows[0], k))
        assert_same(_native.topk_host(q, c, k, metric), want, f"{label}: the host entry in chunks against the handle")
    finally:
        dc.close()


def test_through_the_extension(env):
    """polars_matmul.matmul and polars_matmul.topk at k = 1025 with the knob set: the result
    buffers (the matmul's from the pinned pool) are written by several copies or selects."""
    import polars_matmul

    case = rc.MATMUL_CASES[0]
    q, c = case.data()
    env.setenv(KNOB, case.budget(5))
    with launch_records() as launches:
        got = np.array(polars_matmul.matmul(q, c))
        assert launches(case.label) == rc.chunks(case.m, 5)
    assert_oracle_bits(got, oracle_matmul(case), "polars_matmul.matmul in 14 chunks")
    case, metric, k = rc.F32_HANDLE, rc.COS, 1025
    q, c = case.data(metric, k)
    env.setenv(KNOB, case.budget(5, k))
    with launch_records() as launches:
        idx, sc = polars_matmul.topk(q, c, k, "cosine")
        assert launches(case.label) == rc.chunks(case.m, 5)
    oi, osc = oracle_topk(case, metric, k)
    assert sc.dtype == np.float64
    assert_oracle_bits(np.asarray(idx).astype(np.uint32), oi, "polars_matmul.topk indices")
    assert_oracle_bits(sc, osc.astype(np.float64), "polars_matmul.topk scores")


# ---------------------------------------------------------------------------
# The real budget, knob unset
# ---------------------------------------------------------------------------
def test_matmul_at_the_real_budget(env):
    """f32 1030 x 524288 x 8: chunks of 1024 rows (exactly 2^31 bytes) and 6 rows; 2.16 GB result.
    Measured on an MI355X: 0.19 s in the call, 0.45 s for the test with the inputs and the checks."""
    q, c = rc.full_size_inputs()
    t0 = time.perf_counter()
    with launch_records() as launches:
        out = _native.matmul_host(q, c)
        count = launches("gemm_f32_matmul")
    print(f"matmul at the real budget: {time.perf_counter() - t0:.2f} s in the call")
    assert count == 2, f"{count} launches of the chunked GEMM"
    assert out.shape == (rc.FULL_M, rc.FULL_N) and out.dtype == np.float32
    for a, b in rc.FULL_PAIRS:
        assert np.array_equal(out[a].view(np.uint32), out[b].view(np.uint32)), f"rows {a} and {b} differ"
    want = np.asarray(oracle.matmul(np.ascontiguousarray(q[rc.FULL_SAMPLE]), c)).astype(np.float32)
    assert_oracle_bits(np.ascontiguousarray(out[rc.FULL_SAMPLE]), want, "matmul at the real budget, sampled rows")
    print(f"matmul at the real budget: {time.perf_counter() - t0:.2f} s with the checks")


def test_topk_at_the_real_budget(env):
    """The same shape at k = 1025, cosine: a score chunk of exactly 2^31 bytes, then one of 6 rows.
    Measured on an MI355X: 0.02 s in the call, 0.28 s for the test with the oracle's 68 rows."""
    q, c = rc.full_size_inputs()
    k = rc.FULL_K
    t0 = time.perf_counter()
    with launch_records() as launches:
        idx, sc = _native.topk_host(q, c, k, rc.COS)
        count = launches("gemm_f32_scores")
    print(f"top-k at the real budget: {time.perf_counter() - t0:.2f} s in the call")
    assert count == 2, f"{count} launches of the chunked GEMM"
    for a, b in rc.FULL_PAIRS:
        assert np.array_equal(idx[a], idx[b]) and np.array_equal(sc[a].view(np.uint32), sc[b].view(np.uint32)), \
            f"rows {a} and {b} differ"
    oi, osc = oracle.topk(np.ascontiguousarray(q[rc.FULL_SAMPLE]), c, k, rc.COS)
    assert_oracle_bits(np.ascontiguousarray(idx[rc.FULL_SAMPLE]), np.asarray(oi).astype(np.uint32), "top-k at the real budget, indices")
    assert_oracle_bits(np.ascontiguousarray(sc[rc.FULL_SAMPLE]), np.asarray(osc).astype(np.float32), "top-k at the real budget, scores")
    print(f"top-k at the real budget: {time.perf_counter() - t0:.2f} s with the checks")
