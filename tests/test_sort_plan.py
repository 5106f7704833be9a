"""The sort plan of ragged key lists (pmm_sort_plan, ``_native.sort_plan``;
DESIGN.md §4d "Piece planner and sort driver") against a numpy restatement of
its rule, at every tier boundary.  Host only: no GPU."""
from __future__ import annotations

import numpy as np
import pytest

from polars_matmul import _native

I64_MAX = np.iinfo(np.int64).max
WAVE_MAX = 128  # kRangeWaveMax


def lengths(smax):
    return [0, 1, 2, 127, 128, 129, smax - 1, smax, smax + 1, 2 * smax, 2 * smax + 1, 3 * smax]


def restated(offsets, smax, cap):
    """The rule, piece by piece: a segment of more than smax keys is cut into
    pieces of smax (the last one shorter), any other is one piece."""
    counts = np.diff(offsets)
    T = np.where(counts > smax, -(-counts // smax), 1)
    row = np.repeat(np.arange(counts.size), T)  # the segment of every piece
    first = np.cumsum(T) - T                    # a segment's first piece
    t = np.arange(T.sum()) - first[row]         # a piece's place in its segment
    po = np.concatenate([[0], np.minimum(offsets[row] + (t + 1) * smax, offsets[row + 1])])
    lens = np.diff(po)
    mid = np.flatnonzero(lens > WAVE_MAX)
    kout = np.where(T > 1, np.minimum(cap, counts), 0)  # merged keys of a cut segment
    dst = np.cumsum(kout) - kout
    cp = np.flatnonzero(T[row] > 1)                     # the pieces of cut segments
    cut = np.zeros(cp.size, dtype=_native.SORT_PIECE)
    cut["self"], cut["first"], cut["T"] = cp, first[row[cp]], T[row[cp]]
    cut["kout"], cut["dst"] = kout[row[cp]], dst[row[cp]]
    return po, mid, int(lens[mid].max()) if mid.size else 0, cut, int(kout.sum())


@pytest.mark.parametrize("cap", [1, 100, 3 * 8192 + 1, I64_MAX])
@pytest.mark.parametrize("smax", [128, 256, 8192])
def test_sort_plan_equals_the_restated_rule(smax, cap):
    L = np.array(lengths(smax), dtype=np.int64)
    assert cap in (1, 100) or cap > L.max()
    offsets = np.concatenate([[0], np.cumsum(L)])
    po, mid, mid_max, cut, merged = _native.sort_plan(offsets, smax, cap)
    wpo, wmid, wmid_max, wcut, wmerged = restated(offsets, smax, cap)
    assert np.array_equal(po, wpo)
    assert np.array_equal(mid, wmid) and mid_max == wmid_max
    for name in _native.SORT_PIECE.names:
        assert np.array_equal(cut[name], wcut[name]), name
    assert merged == wmerged
    if smax == WAVE_MAX:  # no piece exceeds the wave tier
        assert mid.size == 0 and mid_max == 0

    # the pieces tile each segment exactly: consecutive, none longer than smax,
    # only a segment's last piece shorter, and every segment bound a piece bound
    lens = np.diff(po)
    assert po[0] == 0 and po[-1] == offsets[-1] and (lens >= 0).all() and (lens <= smax).all()
    assert np.isin(offsets, po).all()
    T = np.maximum(1, -(-L // smax))
    assert po.size - 1 == T.sum()
    ends = np.cumsum(T)
    for i in range(L.size):
        seg = lens[ends[i] - T[i]:ends[i]]
        assert seg.sum() == L[i] and (seg[:-1] == smax).all()
    # the dst ranges of cut rows: one per row, in order, disjoint and contiguous from 0
    rows = cut[cut["self"] == cut["first"]]
    assert np.array_equal(rows["kout"], np.minimum(cap, L[L > smax]))
    assert np.array_equal(rows["dst"], np.cumsum(rows["kout"]) - rows["kout"])
    assert merged == rows["kout"].sum()
    for r in rows:  # every piece of the row carries the row's record
        mine = cut[cut["first"] == r["first"]]
        assert mine.size == r["T"] and np.array_equal(mine["self"], r["first"] + np.arange(r["T"]))
        assert (mine["kout"] == r["kout"]).all() and (mine["dst"] == r["dst"]).all()


def test_sort_plan_refusals():
    ok = np.array([0, 5, 300], dtype=np.int64)
    for offsets, smax, cap in [(ok, 127, 1), (ok, 8193, 1), (ok, 256, 0), (np.array([1, 5], np.int64), 256, 1),
                               (np.array([0, 5, 4], np.int64), 256, 1)]:
        with pytest.raises(_native.PmmError) as ei:
            _native.sort_plan(offsets, smax, cap)
        assert ei.value.code == _native.PMM_ERR_ARG
    po, mid, mid_max, cut, merged = _native.sort_plan(np.zeros(1, np.int64), 256, 1)  # m = 0
    assert po.tolist() == [0] and mid.size == 0 and cut.size == 0 and (mid_max, merged) == (0, 0)
