"""The screened path's two-phase exact finish (screen_rescore_kernel,
csrc/pmm_kernels.hip), restated in NumPy: which of a row's entries are scored
exactly, given exact scores s, approximate scores a with |a - s| <= eps, k and
the row's starting bound T (every column of the exact top-k has a >= T).

  0. live = entries with a >= T; n_r <= k: all of them, done.
  1. P1 = the k live entries with the largest (a, lower index first); e_k =
     the least exact score among them.
  2. T2 = max(T, e_k - eps); of the rest, the entries with a >= T2.

The survivors must contain the exact top-k in the library's order (score
descending, lower index first), and never outnumber the live entries, which is
what a single pass at T scores.
"""
from __future__ import annotations

import numpy as np
import pytest

from parity import round_bf16
from test_screen_bound import rel_residual, screen_eps


def finish(s, a, eps, k, T):
    """-> (survivors, kept, rescored)"""
    live = np.flatnonzero(a >= T)
    kept = len(live)
    if kept <= k:
        return live, kept, kept
    order = live[np.lexsort((live, -a[live]))]
    p1, rest = order[:k], order[k:]
    e_k = s[p1].min()
    t2 = max(T, e_k - eps)
    surv = np.concatenate([p1, rest[a[rest] >= t2]])
    return surv, kept, len(surv)


def exact_topk(s, k):
    return np.lexsort((np.arange(len(s)), -s))[:k]


def check(s, a, eps, k, T):
    s, a = np.asarray(s, np.float64), np.asarray(a, np.float64)
    assert np.all(np.abs(a - s) <= eps * (1 + 1e-12))
    top = exact_topk(s, min(k, len(s)))
    assert np.all(a[top] >= T), "the case's starting bound drops a top-k column"
    surv, kept, rescored = finish(s, a, eps, k, T)
    assert set(top.tolist()) <= set(surv.tolist())
    assert rescored <= kept
    return kept, rescored


def kth(s, k):
    return np.sort(s)[::-1][min(k, len(s)) - 1]


EPS = 0.0043  # the flagship shape's slack


def test_random_scores():
    rs = np.random.RandomState(0)
    for n, k in ((2000, 100), (9037, 10), (300, 100), (50000, 100)):
        s = rs.randn(n) / np.sqrt(768.0)
        a = s + np.clip(rs.randn(n) * 2e-4, -EPS, EPS)
        for T in (-np.inf, kth(s, k) - 2 * EPS, kth(s, k) - EPS):
            kept, rescored = check(s, a, EPS, k, T)
        # a tight starting bound and a real error far below the slack: about
        # k plus one eps of band instead of two
        assert rescored <= kept


def test_adversarial_signs_around_the_kth():
    rs = np.random.RandomState(1)
    for n, k in ((2000, 100), (500, 10), (64, 1)):
        s = rs.randn(n) / np.sqrt(768.0)
        top = exact_topk(s, k)
        a = s + EPS  # non-members pushed up
        a[top] = s[top] - EPS  # members pushed down
        for T in (-np.inf, kth(s, k) - 2 * EPS, kth(s, k) - EPS):
            check(s, a, EPS, k, T)
        # and the other way round
        a = s - EPS
        a[top] = s[top] + EPS
        check(s, a, EPS, k, kth(s, k) - EPS)


def test_exact_duplicates_straddling_the_kth():
    rs = np.random.RandomState(2)
    base = rs.randn(40) / 8.0
    s = np.tile(base, 30)  # every score 30 times: the k-th falls inside a run
    for k in (1, 10, 100, 119, 120, 121):
        for a in (s.copy(), s + rs.uniform(-EPS, EPS, len(s))):
            for T in (-np.inf, kth(s, k) - EPS):
                check(s, a, EPS, k, T)


@pytest.mark.parametrize("n_r", [99, 100, 101, 1, 37])
def test_few_live_entries(n_r):
    # n_r = k, k + 1 and below k: the live entries are the whole row
    rs = np.random.RandomState(3)
    k = 100
    s = rs.randn(n_r) / 8.0
    a = s + rs.uniform(-EPS, EPS, n_r)
    kept, rescored = check(s, a, EPS, k, -np.inf)
    assert kept == n_r
    if n_r <= k:
        assert rescored == n_r


def test_k_equals_one():
    rs = np.random.RandomState(4)
    s = rs.randn(5000) / np.sqrt(768.0)
    a = s + rs.uniform(-EPS, EPS, 5000)
    kept, rescored = check(s, a, EPS, 1, -np.inf)
    assert rescored < kept


def test_all_scores_equal():
    s = np.full(777, 0.25)
    for k in (1, 100, 777):
        kept, rescored = check(s, s.copy(), EPS, k, -np.inf)
        assert kept == rescored == 777  # nothing can be ruled out
    rs = np.random.RandomState(5)
    check(s, s + rs.uniform(-EPS, EPS, 777), EPS, 100, 0.25 - EPS)


def test_crowded_band_keeps_everything():
    # every entry within eps of the k-th: all survive, none more than before
    rs = np.random.RandomState(6)
    s = 0.5 + rs.uniform(-1e-5, 1e-5, 3000)
    a = s + rs.uniform(-1e-4, 1e-4, 3000)
    kept, rescored = check(s, a, EPS, 10, kth(s, 10) - 2 * EPS)
    assert kept == rescored == 3000


def test_split_units_case_gathers_strictly_less():
    """The GPU suite's split-unit case (seed 12, 70 x 9037 x 200, k = 10, eight
    units of 18 tiles of 64 columns, test_gpu_screen_finish.py): a single pass
    scores every entry at or above the best bound a unit can publish, (the
    largest unit k-th) - 2 eps; the real bound is older and lower, so the real
    pass scores no fewer.  The two-phase rule scores strictly fewer, and the
    same set from any starting bound below e_k - eps."""
    rs = np.random.RandomState(12)
    q, c = rs.randn(70, 200).astype(np.float32), rs.randn(9037, 200).astype(np.float32)
    k, unit = 10, 18 * 64

    def cosine(x, y):
        x, y = x.astype(np.float64), y.astype(np.float64)
        return (x @ y.T) / (np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(y, axis=1)[None, :])

    s = cosine(q, c)
    qn = np.linalg.norm(q.astype(np.float64), axis=1)
    cn = np.linalg.norm(c.astype(np.float64), axis=1)
    a = (round_bf16(q).astype(np.float64) @ round_bf16(c).astype(np.float64).T) / (qn[:, None] * cn[None, :])
    rc = max(rel_residual(row) for row in c)
    kept_all = rescored_all = 0
    for r in range(len(q)):
        eps = screen_eps(rel_residual(q[r]), rc, 256)
        assert np.abs(a[r] - s[r]).max() <= eps
        best_unit_kth = max(kth(a[r, u:u + unit], k) for u in range(0, c.shape[0], unit))
        kept, rescored = check(s[r], a[r], eps, k, best_unit_kth - 2 * eps)
        assert rescored == check(s[r], a[r], eps, k, -np.inf)[1]
        kept_all += kept
        rescored_all += rescored
    print(f"kept {kept_all} rescored {rescored_all}")
    assert rescored_all < kept_all
