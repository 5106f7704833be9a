"""The value cases (tests/value_cases.py) on the oracle alone: every case still
produces the score class it exists for, so an edit of the generator cannot
quietly turn the GPU value-range tests back into ``randn`` tests.  Presence and
one ordering fact are asserted, not counts: a reseed keeps these tests green.
No GPU.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from value_cases import CASES, value_cases

M, N, D = 19, 300, 37
METRIC = {"cosine": oracle.COSINE, "dot": oracle.DOT, "euclidean": oracle.EUCLIDEAN}


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def lists(request):
    """{(case, metric): (indices, scores in the inputs' width)}: the oracle's full ranked lists."""
    dtype = request.param
    out = {}
    for name, q, c in value_cases(dtype, M, N, D):
        assert q.shape == (M, D) and c.shape == (N, D) and q.dtype == c.dtype == dtype
        for metric, mid in METRIC.items():
            oi, osc = oracle.topk(q, c, N, mid)
            out[name, metric] = (np.asarray(oi), np.asarray(osc).astype(dtype))
    return dtype, out


def classes(s):
    tiny = np.finfo(s.dtype).tiny
    zero = s == 0
    return dict(subnormal=int(((np.abs(s) < tiny) & ~zero).sum()), neg_zero=int((zero & np.signbit(s)).sum()),
                pos_zero=int((zero & ~np.signbit(s)).sum()), nan=int(np.isnan(s).sum()),
                inf=int(np.isinf(s).sum()), finite=int(np.isfinite(s).sum()))


def test_the_generator_yields_the_five_cases(lists):
    assert {name for name, _ in lists[1]} == set(CASES)


def test_row_scales_spans_the_binades_and_the_norm_threshold(lists):
    dtype, out = lists
    dot = out["row_scales", "dot"][1]
    assert np.isfinite(dot).all() and np.unique(dot).size > 0.9 * dot.size
    e = np.frexp(dot[dot != 0])[1]
    assert e.max() - e.min() > (100 if dtype == np.float32 else 800)
    cos = classes(out["row_scales", "cosine"][1])
    # rows under the norm threshold score exactly 0, the others do not
    assert cos["pos_zero"] > 0 and cos["finite"] - cos["pos_zero"] - cos["neg_zero"] > 0


def test_underflow_has_subnormal_scores(lists):
    _, out = lists
    dot = out["underflow", "dot"][1]
    assert classes(dot)["subnormal"] > 0 and np.unique(dot).size > 100
    cos = out["underflow", "cosine"][1]
    assert classes(cos)["pos_zero"] == cos.size  # every norm under the threshold: pure index order
    assert np.array_equal(out["underflow", "cosine"][0], np.tile(np.arange(N), (M, 1)))
    euc = out["underflow", "euclidean"][1]
    assert np.isfinite(euc).all() and np.unique(euc).size > 100 and (euc > 0).any()


def test_overflow_has_nan_inf_and_both_zeros(lists):
    _, out = lists
    cos = classes(out["overflow", "cosine"][1])
    assert cos["nan"] > 0 and cos["neg_zero"] > 0 and cos["pos_zero"] > 0
    assert classes(out["overflow", "dot"][1])["inf"] > 0
    euc = classes(out["overflow", "euclidean"][1])
    assert euc["inf"] > 0 and euc["pos_zero"] > 0


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_signed_zero_interleaves_the_two_zeros_by_index(lists, metric):
    _, out = lists
    oi, sc = out["signed_zero", metric]
    k = classes(sc)
    assert k["neg_zero"] > 0 and k["pos_zero"] > 0
    # the tie rule is visible: some -0.0 is ranked before a +0.0 of higher
    # index and after a +0.0 of lower index
    seen = False
    for r in range(M):
        z = np.flatnonzero(sc[r] == 0)
        for p in z[np.signbit(sc[r, z])]:
            before = [j for j in z if j < p and not np.signbit(sc[r, j])]
            after = [j for j in z if j > p and not np.signbit(sc[r, j])]
            assert all(oi[r, j] < oi[r, p] for j in before) and all(oi[r, j] > oi[r, p] for j in after)
            seen = seen or (bool(before) and bool(after))
    assert seen


def test_nonfinite_has_nan_and_inf_scores(lists):
    _, out = lists
    assert classes(out["nonfinite", "cosine"][1])["nan"] > 0
    dot = classes(out["nonfinite", "dot"][1])
    assert dot["nan"] > 0 and dot["inf"] > 0
    euc = classes(out["nonfinite", "euclidean"][1])
    assert euc["inf"] > 0 and euc["pos_zero"] > 0
