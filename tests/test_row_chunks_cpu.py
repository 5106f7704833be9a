"""The materialise budget's knob and the table of tests/row_chunk_cases.py, without a GPU.

pmm_topk_workspace_bytes of a materialised call is plan_materialise's total, so with
PMM_MATERIALISE_BUDGET set it must be the plan restated in row_chunk_cases (integer planning:
equality), with the knob unset the sizes recorded in tests/test_workspace_routes.py, and a value
the knob does not take must change nothing.  The rest are conditions on the table: every listed
R runs the loop past its first chunk, one R per case leaves a short last chunk, and the planted
rows sit where the cases say.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
import row_chunk_cases as rc
from polars_matmul import _native
from row_chunk_cases import BUDGET, KNOB
from test_workspace_routes import SIZES

F32 = _native.COMPUTE_F32
# (m, n, d, k): the materialised sizes of test_workspace_routes.SIZES, the row-select and the
# global-sort cases of the table, one row over and under a pow2 corpus
SHAPES = [(256, 16384, 256, 1025), (100, 5000, 100, 1025), (64, 8192, 96, 3000), (70, 9001, 40, 1025),
          (33, 8192, 96, 3000), (33, 8193, 96, 2017), (9, 4100, 24, 2016), (1, 1, 1, 1025)]


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    return monkeypatch


def test_global_sort_threshold_restated():
    # k = 2016 is the last row-select k: 2 k + 64 = 4096 = kRowSelMaxP
    assert not rc.global_sort(2016) and rc.global_sort(2017)
    assert rc.rowsel_p(1025) == 4096 and rc.rowsel_p(1100) == 4096 and rc.rowsel_p(10) == 128
    assert rc.per_row(8192, 4, 3000) == 8192 * 4 + 8192 * 16 and rc.per_row(4100, 8, 3000) == 4100 * 8 + 8192 * 16
    assert rc.per_row(9001, 4, 1025) == 9001 * 4 and rc.per_row(301, 4) == 301 * 4


def test_workspace_bytes_unset_is_the_recorded_size(clean_env):
    recorded = {(m, n, d, k): want for _, m, n, d, k, _, compute, screen, want, _ in SIZES
                if compute == F32 and k > rc.FUSED_MAX_K and screen is None}
    assert len(recorded) == 3
    for (m, n, d, k), want in recorded.items():
        assert _native.workspace_bytes(m, n, d, k, rc.COS, F32) == want == rc.materialised_bytes(m, n, k, 4)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + f"-k{s[3]}")
def test_workspace_bytes_follows_the_knob(clean_env, shape):
    m, n, d, k = shape
    row = rc.per_row(n, 4, k)
    unset = _native.workspace_bytes(m, n, d, k, rc.COS, F32)
    assert unset == rc.materialised_bytes(m, n, k, 4)
    for budget in (1, row - 1, row, 2 * row - 1, 2 * row, 7 * row + 5, m * row - 1, m * row, BUDGET - 1, BUDGET):
        clean_env.setenv(KNOB, str(budget))
        rows = max(1, min(m, budget // row))
        assert rc.plan_rows(m, row, budget) == rows
        for metric in rc.METRICS:
            assert _native.workspace_bytes(m, n, d, k, metric, F32) == rc.materialised_bytes(m, n, k, 4, budget), budget
    clean_env.delenv(KNOB)
    assert _native.workspace_bytes(m, n, d, k, rc.COS, F32) == unset


@pytest.mark.parametrize("text", ["0", "-1", "-4096", "abc", "", " 4096", "4096 ", "4096k", "0x1000", "1e3", "4096.0",
                                  "+4096", str(BUDGET + 1), str(1 << 32), str(1 << 64), "9" * 40])
def test_a_value_the_knob_does_not_take_changes_nothing(clean_env, text):
    assert rc.parse_knob(text) == BUDGET
    for m, n, d, k in SHAPES:
        unset = _native.workspace_bytes(m, n, d, k, rc.DOT, F32)
        clean_env.setenv(KNOB, text)
        assert _native.workspace_bytes(m, n, d, k, rc.DOT, F32) == unset, (text, m, n, d, k)
        clean_env.delenv(KNOB)


def test_the_knob_leaves_the_fused_routes_alone(clean_env):
    sizes = [(130, 5000, 96, 10, rc.COS, F32), (64, 4099, 256, 1024, rc.EUC, F32),
             (130, 16384, 256, 100, rc.COS, _native.COMPUTE_BF16)]
    unset = [_native.workspace_bytes(*s) for s in sizes]
    clean_env.setenv(KNOB, "4096")
    assert [_native.workspace_bytes(*s) for s in sizes] == unset


# ---------------------------------------------------------------------------
# Conditions on the table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.ALL_CASES, ids=repr)
def test_every_listed_budget_chunks_the_call(case):
    """Every R gives at least two chunks of the rule's rows; one R per case leaves a short last
    chunk.  The one exception is listed as such: R = m on the padded matmul shape, the budget of
    exactly the whole call, which must plan one chunk (and one byte less must plan two)."""
    n = rc.shard_rows(case) if case is rc.F64_SHARDED else case.n
    short = False
    for k in case.ks:
        row = rc.per_row(n, case.elem, k)
        assert row * case.m < BUDGET, "the unset run is one chunk"
        assert rc.plan_rows(case.m, row) == case.m
        for r in case.rows:
            budget = int(rc.budget_of(r, row))
            assert 1 <= budget <= BUDGET and rc.parse_knob(str(budget)) == budget
            assert rc.plan_rows(case.m, row, budget) == r
            if r == case.m:
                assert case.rows is rc.PADDED_ROWS and rc.chunks(case.m, r) == 1
                assert rc.plan_rows(case.m, row, budget - 1) == r - 1
                continue
            assert rc.chunks(case.m, r) >= 2, (case.name, r)
            short |= case.m % r != 0
    assert short, f"{case.name}: no R leaves a short last chunk"
    if case in (rc.F64_FALLBACK, rc.F64_SHARDED):
        assert max(rc.chunks(case.m, r) for r in case.rows) >= 3
    if case in rc.ENTRY_CASES:
        assert all(rc.chunks(case.m, r) >= 3 for r in case.rows)


def test_topk_shapes_take_the_route_they_name():
    assert all(k > rc.FUSED_MAX_K for c in (rc.F32_ROWSEL, rc.F32_GSORT, rc.F32_DEVICE, rc.F32_HANDLE) for k in c.ks)
    assert not rc.global_sort(1025) and not rc.global_sort(1100) and rc.global_sort(3000)
    # the f32 row select compacts when a row's buffer of P entries is full and keeps k of them:
    # n > 2 (P - 64) + 64 takes more than one compaction before the last batch
    assert rc.F32_ROWSEL.n > 2 * (rc.rowsel_p(1025) - 64) + 64


@pytest.mark.parametrize("case", [c for c in rc.MATMUL_CASES if c.d == 37], ids=repr)
def test_padded_matmul_rows_hold_the_signed_zeros(case):
    q, c = case.data()
    want = np.asarray(oracle.matmul(q, c))
    neg = np.signbit(want) & (want == 0)
    assert neg[list(rc.ZERO_SUM_ROWS)].any(axis=1).all(), "a planted row has no -0.0 sum"
    pos = ~np.signbit(want) & (want == 0)
    assert pos[list(rc.ZERO_SUM_ROWS)].any(axis=1).all()
    assert not q[list(rc.ZERO_QUERY_ROWS)].any() and (want[list(rc.ZERO_QUERY_ROWS)] == 0).all()
    for r in case.rows:
        if r == case.m:
            continue
        second = range(r, min(2 * r, case.m))
        last = range((rc.chunks(case.m, r) - 1) * r, case.m)
        assert set(second) & set(rc.ZERO_SUM_ROWS), f"R={r}: no -0.0 sum in the second chunk"
        assert set(last) & set(rc.ZERO_SUM_ROWS), f"R={r}: no -0.0 sum in the last chunk"
    assert any(z >= r for z in rc.ZERO_QUERY_ROWS for r in case.rows if r < case.m)


@pytest.mark.parametrize("case", rc.TOPK_CASES + rc.ENTRY_CASES, ids=repr)
def test_planted_rows_straddle_the_kth_place(case):
    """On the oracle: in a starred query row's list some of the duplicate corpus rows are in and
    some are out, the ones in are the lowest indices and their scores are one bit pattern."""
    for metric in case.metrics:
        for k in case.ks:
            q, c = case.data(metric, k)
            dup = rc.duplicate_rows(case, metric, k)
            assert dup.size == rc.DUPLICATES and np.isnan(c[rc.NAN_ROW]).any() and not c[rc.ZERO_ROW].any()
            star = case.second_chunk_rows()
            for r in case.rows:
                assert any(r <= s < 2 * r for s in star), f"R={r}: no starred row in the second chunk"
            idx, sc = oracle.topk(np.ascontiguousarray(q[star[:1]]), c, k, metric)
            inside = np.isin(np.asarray(idx)[0], dup)
            assert 0 < inside.sum() < rc.DUPLICATES, (case.name, metric, k, int(inside.sum()))
            assert sorted(np.asarray(idx)[0][inside]) == sorted(dup[:inside.sum()])
            assert len({x.tobytes() for x in np.asarray(sc)[0][inside]}) == 1
            assert inside[-1], "the ties do not reach the k-th place"


def test_full_size_shape_is_one_chunk_of_two_to_the_31():
    row = rc.per_row(rc.FULL_N, 4, rc.FULL_K)
    assert row == rc.per_row(rc.FULL_N, 4) and rc.plan_rows(rc.FULL_M, row) == rc.FULL_CHUNK
    assert rc.FULL_CHUNK * row == BUDGET and rc.chunks(rc.FULL_M, rc.FULL_CHUNK) == 2
    assert rc.FULL_PAIRS == tuple((r, 1024 + r) for r in range(6))
    assert {0, 1023, 1024, 1029} <= set(rc.FULL_SAMPLE) and len(rc.FULL_SAMPLE) == 68
