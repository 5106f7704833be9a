"""The triangular schedule of the self range search's emit pass
(pmm_range_self_plan; host only, no GPU).  Query block b (BM rows) visits corpus
tile t (BN columns) iff the tile's last column is above the block's first row:
min(n, (t + 1) BN) - 1 > b BM.  The entry's count must equal that rule counted
here, pair by pair."""
from __future__ import annotations

import ctypes

import pytest

from polars_matmul import _native

TILE = {0: (128, 128), 3: (256, 256)}  # variant -> (BM, BN)


def visits_by_rule(n, bm, bn):
    QB, T = -(-n // bm), -(-n // bn)
    if n > 4096:  # (the rule is monotone in t: count from the first visited tile)
        total = 0
        for b in range(QB):
            t = next((t for t in range(min(T, b * bm // bn), T) if min(n, (t + 1) * bn) - 1 > b * bm), T)
            assert t == 0 or not min(n, t * bn) - 1 > b * bm
            total += T - t
        return total, QB * T
    return sum(min(n, (t + 1) * bn) - 1 > b * bm for b in range(QB) for t in range(T)), QB * T


@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("n", [1, 2, 128, 129, 513, 100000])
def test_visit_count_is_the_rule(n, variant):
    bm, bn = TILE[variant]
    v, visits, full = _native.range_self_plan(n, 256, variant)
    want, want_full = visits_by_rule(n, bm, bn)
    assert v == variant and (visits, full) == (want, want_full)
    T = -(-n // bn)
    assert visits <= T * (T + 1) // 2  # BM = BN: never more than the upper triangle with its diagonal


def test_513_rows_visit_14_of_25():
    assert _native.range_self_plan(513, 256, 0) == (0, 14, 25)
    assert _native.range_self_plan(1, 256, 0) == (0, 0, 1)  # one row has no pair


def test_the_ratio_tends_to_half():
    _, visits, full = _native.range_self_plan(262144, 256, 3)
    T = 1024
    assert full == T * T and visits == T * (T + 1) // 2


def test_chosen_variant_and_refusals():
    v_small, _, _ = _native.range_self_plan(513, 256, -1)
    v_large, _, _ = _native.range_self_plan(100000, 256, -1)
    assert (v_small, v_large) == (0, 3)
    lib = _native.lib()
    v, a, b = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    for args in ((-1, 256, 0), (10, 0, 0), (10, 256, 1), (10, 256, 5)):
        assert lib.pmm_range_self_plan(*args, ctypes.byref(v), ctypes.byref(a), ctypes.byref(b)) == _native.PMM_ERR_ARG
    assert lib.pmm_range_self_plan(10, 256, 0, None, ctypes.byref(a), ctypes.byref(b)) == _native.PMM_ERR_ARG
