"""The screened top-k's guessed starting bound, restated in NumPy.

The library extrapolates each row's final k-th score from its seed sample
(mean + z standard deviations, z the normal quantile of rank t k of n), starts
the row's screen from max(proven bound, guess) and lets the exact finish decide
whether the guess held (screen_guess_kernel, gemm_bf16_ws_kernel's SCREEN path,
screen_rescore_kernel).  This file restates the rule over emulated units and
checks, on score sets the extrapolation is wrong for, the two properties the
exactness rests on:

  * a row whose guess was not confirmed is never finished (it is flagged for
    the re-run);
  * a row that is finished holds every column of its exact top-k, and its
    proven bound never exceeds its exact k-th score.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

NS = 1024  # the seed's sample columns
T = 4.0    # the library's default slack (kScreenGuessSlack)


def normal_upper_quantile(p):
    lo, hi = 0.0, 40.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def guess_bound(sample, k, n, eps, t=T):
    """The guessed bound of the exact k-th (gthr's space), or None."""
    z = normal_upper_quantile(t * k / n)
    g = float(np.mean(sample, dtype=np.float64) + z * np.std(sample, dtype=np.float64))
    if not abs(g) <= 1.0:
        return None
    return g - eps


def screen_row(exact, approx, k, eps, units, ctrig, guess):
    """One row through the emulated screen.  exact / approx: its n scores
    (|exact - approx| <= eps); units: column ranges, each with a segment of
    its own sharing the proven bound, as split units do.  Returns (status,
    proven bound, held columns), status one of "finished", "guess_missed" and
    "overflowed" (a band that outgrew its segment: re-run, as without a guess)."""
    seed = np.sort(approx[:NS])[-k] - eps  # proven: k columns have exact >= a_k - eps
    proven = seed
    held = []
    overflowed = False
    for lo, hi in units:
        start = proven if guess is None else max(proven, guess)
        thr = start - eps  # the unit's threshold in the approximate scores' space
        seg = []
        for j in range(lo, hi):
            if approx[j] >= thr:
                seg.append(j)
                if len(seg) > ctrig:  # compaction: publish a_k - eps, keep the band above a_k - 2 eps
                    a = np.sort(approx[seg])[-k]
                    proven = max(proven, a - eps)
                    thr = max(thr, a - 2 * eps)
                    band = [c for c in seg if approx[c] >= a - 2 * eps]
                    if len(band) > ctrig:
                        overflowed = True
                        thr = max(thr, a)
                        band = sorted(seg, key=lambda c: -approx[c])[:k]
                    seg = band
        held += seg
    if overflowed:
        return "overflowed", proven, held
    # the finish: live entries, the k best approximate ones scored exactly
    live = [c for c in held if approx[c] >= proven - eps]
    flagged = guess is not None and proven < guess
    if flagged:
        confirmed = False
        if len(live) > k:
            best = sorted(live, key=lambda c: -approx[c])[:k]
            confirmed = min(exact[c] for c in best) >= guess
        if not confirmed:
            return "guess_missed", proven, held
    return "finished", proven, held


def score_sets():
    rs = np.random.RandomState(5)
    n = 16384
    sets = {}
    sets["gaussian"] = rs.randn(n) * 0.09
    # bimodal: a cluster of near-duplicates in the sample only -> the guess overshoots every score
    b = rs.randn(n) * 0.05
    b[:256] = 0.8 + rs.randn(256) * 0.01
    sets["bimodal_in_sample"] = b
    # bimodal, the cluster outside the sample -> the guess is far too low (harmless)
    b2 = rs.randn(n) * 0.05
    b2[5000:5256] = 0.8 + rs.randn(256) * 0.01
    sets["bimodal_outside_sample"] = b2
    # heavy-tailed sample, light-tailed rest
    h = rs.randn(n) * 0.03
    h[:NS] = np.clip(rs.standard_t(2, NS) * 0.05, -0.95, 0.95)
    sets["heavy_tailed_sample"] = h
    sets["heavy_tailed"] = np.clip(rs.standard_t(3, n) * 0.05, -0.95, 0.95)
    sets["all_equal"] = np.full(n, 0.25)
    # fewer than k columns above a plateau of ties
    tie = rs.randn(n) * 0.02
    tie[rs.choice(n, 400, replace=False)] = 0.5
    sets["tied_kth"] = tie
    return sets


SETS = score_sets()


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("split", [1, 5])
@pytest.mark.parametrize("k", [100, 192])
def test_flag_rule_is_exact(name, split, k):
    exact = SETS[name]
    n = len(exact)
    eps = 0.004
    rs = np.random.RandomState(k + split)
    approx = exact + rs.uniform(-eps, eps, n)
    edges = np.linspace(0, n, split + 1).astype(int)
    units = list(zip(edges[:-1], edges[1:]))
    guess = guess_bound(approx[:NS], k, n, eps)
    status, proven, held = screen_row(exact, approx, k, eps, units, ctrig=448, guess=guess)
    kth = np.sort(exact)[-k]
    assert proven <= kth  # the proven bound, guessed start or not
    if status == "finished":
        # every column strictly above the exact k-th, and enough at it, are held
        held = set(held)
        assert all(j in held for j in np.nonzero(exact > kth)[0])
        assert sum(1 for j in held if exact[j] >= kth) >= k
    elif status == "guess_missed":
        # only a guess can stop a row from finishing, and only one that was not reached
        assert guess is not None and proven < guess


def test_overshoot_is_flagged_not_finished():
    # the construction tests/test_gpu_screen_guess.py relies on: the guess lies above every score
    exact = SETS["bimodal_in_sample"]
    eps = 0.004
    guess = guess_bound(exact[:NS], 100, len(exact), eps)
    assert guess is not None and guess > exact.max()
    status, _, _ = screen_row(exact, exact, 100, eps, [(0, len(exact))], 448, guess)
    assert status == "guess_missed"


def test_gaussian_guess_confirms():
    exact = SETS["gaussian"]
    eps = 0.004
    guess = guess_bound(exact[:NS], 100, len(exact), eps)
    kth = np.sort(exact)[-100]
    assert guess is not None and guess <= kth
    status, _, _ = screen_row(exact, exact, 100, eps, [(0, len(exact))], 448, guess)
    assert status == "finished"
