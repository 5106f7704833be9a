"""The wide-stride cases (tests/wide_stride_cases.py) without a device: the refusal of the f32 and
bf16 top-k entries, which precedes every device call, and the power of the cases' inputs.

Power: random rows pass a wrong kernel by luck if no winner lies where it misreads.  For every f32
and bf16 case, either operand and every span height of the kernels, the oracle's lists over the
rows as a clamped descriptor would deliver them (the far rows of each span zero), and as wrapped
32-bit offsets would (another row, or the poison), differ from the true lists.  The threshold is
"differs at all"; it is a condition on the inputs, checked on the oracle alone.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from polars_matmul import _native
from device_cases import COS, DOT, EUC
from wide_stride_cases import (BF16_CASES, DESC_MAX_BYTES, DESC_ROWS_MAX, ELEM, F32_CASES, F32_SEED_SKIPPED, FF_CASES,
                               LIMIT_BYTES, SOUND_CASES, TILE_ROWS, clamp_stride, misread_rows, refused_strides,
                               wrap_stride)


def as_f32(case, rows):
    if case.kind == "bf16":
        return np.ascontiguousarray((rows.astype(np.uint32) << 16).view(np.float32))
    return rows


def lists(case, q, c):
    k, metric = case.shape[3], case.shape[4]
    idx, sc = oracle.topk(q, c, k, metric)
    return np.asarray(idx), np.asarray(sc)


@pytest.mark.parametrize("case", F32_CASES + F32_SEED_SKIPPED + BF16_CASES + FF_CASES, ids=repr)
def test_inputs_tell_a_misread_from_the_truth(case):
    q, c = (as_f32(case, case.operand(nm).data) for nm in ("q", "c"))
    true_idx, _ = lists(case, q, c)
    width = {nm: case.operand(nm).tight_ld * ELEM[case.kind] for nm in ("q", "c")}
    for R in TILE_ROWS:
        # (a wave's query rows: one span of 32 in every f32 and bf16 kernel of the product)
        for name, stride, wrap in [("c", clamp_stride(R), False), ("c", wrap_stride(R), True)] + \
                ([("q", clamp_stride(R), False), ("q", wrap_stride(R), True)] if R == 32 else []):
            assert stride > LIMIT_BYTES  # (a stride the entry refuses)
            bad = misread_rows(c if name == "c" else q, R, stride, width[name], wrap)
            assert not np.array_equal(bad, c if name == "c" else q, equal_nan=True)
            idx, _ = lists(case, bad, c) if name == "q" else lists(case, q, bad)
            assert not np.array_equal(idx, true_idx), f"{case.name}: {name} in spans of {R} rows at {stride} bytes"


# (case, rows of the seed's sample): the f32 prologue's min(n, 256), PMM_SEED_NS, the bf16 default
SEEDED = [(c, min(c.shape[1], 256)) for c in F32_CASES if c.knobs.get("PMM_SEED") == "1"] + \
         [(c, 512) for c in F32_SEED_SKIPPED] + \
         [(c, int(c.knobs.get("PMM_SEED_NS", 1024))) for c in BF16_CASES if c.launches.get("seed_bf16") == 1]


@pytest.mark.parametrize("case,ns", SEEDED, ids=lambda v: repr(v))
def test_inputs_tell_a_clamped_seed_sample(case, ns):
    """The seed's threshold is the k-th best score of the first ns corpus rows, read through one
    descriptor over the sample.  With the sample's upper half read as zero rows, a threshold
    better than the row's true k-th best drops real results in the main pass.  A zero row is at
    distance |q| from q, nearer than most rows: on the euclidean cases the clamped threshold must
    beat the true k-th distance in at least one list.  On cosine and dot a zero row scores 0,
    below every true k-th best of these inputs, so a clamped sample can only lower the threshold:
    harmless, and asserted as such, so that the claim stands on the inputs."""
    q, c = (as_f32(case, case.operand(nm).data) for nm in ("q", "c"))
    k, metric = case.shape[3], case.shape[4]
    width = case.operand("c").tight_ld * ELEM[case.kind]
    stride = clamp_stride(ns)
    assert ns * stride > DESC_MAX_BYTES
    sample = misread_rows(c[:ns], ns, stride, width, False)
    assert not np.array_equal(sample, c[:ns])
    seeded = lists(case, q, sample)[1][:, k - 1].astype(np.float64)
    true = lists(case, q, c)[1][:, k - 1].astype(np.float64)
    if metric == EUC:
        assert np.any(seeded < true), f"{case.name}: no clamped threshold beats a true k-th distance"
    else:
        assert metric in (COS, DOT) and np.all(true > 0) and np.all(seeded <= true)


def test_limit_is_the_descriptor_over_the_tallest_span():
    assert LIMIT_BYTES % 16 == 0 and DESC_ROWS_MAX * LIMIT_BYTES <= DESC_MAX_BYTES < DESC_ROWS_MAX * (LIMIT_BYTES + 16)
    assert max(TILE_ROWS) == DESC_ROWS_MAX


def test_metrics_and_dims_of_the_table():
    """Every top-k kind runs the three metrics at d = 37 and d = 256 (bits: its one distance)."""
    for cases in (F32_CASES, BF16_CASES, FF_CASES, SOUND_CASES):
        for kind in {c.kind for c in cases}:
            seen = {(c.shape[2], c.shape[4]) for c in cases if c.kind == kind}
            want = {(d, mt) for d in (37, 256) for mt in ((COS,) if kind == "bits" else (COS, DOT, EUC))}
            assert want <= seen, (kind, sorted(want - seen))


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_wide_stride_is_refused_before_any_device_call(kind):
    """As test_boundary's null buffers: an argument error, raised as the wrappers raise the others."""
    fn = _native.topk_device if kind == "f32" else _native.topk_bf16_device
    a = np.zeros((4, 128), np.float32)
    oi, sc = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    tight = 128
    for ld in refused_strides(kind):
        for name in ("q", "c"):
            ldq, ldc = (ld, tight) if name == "q" else (tight, ld)
            with pytest.raises(_native.PmmError) as err:
                fn(a.ctypes.data, ldq, 1, a.ctypes.data, ldc, 1, 100, 1, 0, oi.ctypes.data, sc.ctypes.data)
            assert err.value.code == _native.PMM_ERR_ARG
            text = _native.last_error()
            assert text == str(err.value)
            assert f"ld{name}={ld}" in text and f"{LIMIT_BYTES} bytes" in text
            assert f"({LIMIT_BYTES // ELEM[kind]} elements)" in text
