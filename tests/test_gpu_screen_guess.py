"""The screened top-k's guessed starting bound (PMM_SCREEN_GUESS, default on):
each row starts the screen from a bound extrapolated from its seed sample, and
a guess that no compaction or exact score confirms sends the row to the f32
re-run.  Whatever the guess does, the lists are the unscreened call's, bit for
bit: every case runs with PMM_F32_SCREEN=1 and compares indices and score bits
with PMM_F32_SCREEN=0 on the same inputs.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS = 0


@pytest.fixture(scope="module")
def native():
    from polars_matmul import _native

    assert _native.device_count() > 0, "no HIP device visible"
    return _native


def same_bits(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def screen_report(capfd):
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pmm screen]")]
    assert lines, "no screened call reported"
    rep = {}
    for tok in lines[0].split()[2:]:
        key, val = tok.split("=")
        rep[key] = float(val) if "." in val or "e" in val else int(val)
    return rep


def screened_vs_plain(native, monkeypatch, capfd, q, c, k, label, guess=None):
    """The screened call's lists and report; asserts they are the unscreened call's."""
    monkeypatch.setenv("PMM_SCREEN_DEBUG", "1")
    q = np.ascontiguousarray(q, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    monkeypatch.setenv("PMM_F32_SCREEN", "0")
    i0, s0 = native.topk_host(q, c, k, COS)
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    if guess is None:
        monkeypatch.delenv("PMM_SCREEN_GUESS", raising=False)
    else:
        monkeypatch.setenv("PMM_SCREEN_GUESS", guess)
    capfd.readouterr()
    i1, s1 = native.topk_host(q, c, k, COS)
    rep = screen_report(capfd)
    print(label, rep)
    assert np.array_equal(i1, i0), f"{label}: indices differ from the unscreened call"
    assert same_bits(s1, s0), f"{label}: scores differ from the unscreened call"
    return i1, s1, rep


def test_plain_gaussian(native, monkeypatch, capfd):
    # Gaussian scores are what the extrapolation assumes.  At the default
    # slack (rank 4 k of n) a miss needs the estimated quantile off by ln 4 / z
    # = 0.7 standard deviations against an estimation error of 0.06 (1024
    # samples): the expected number of missed rows is far below one, m / 32
    # leaves room for the cosine's non-Gaussian tail.
    rs = np.random.RandomState(21)
    m, n, d, k = 256, 16384, 128, 100
    _, _, rep = screened_vs_plain(native, monkeypatch, capfd, rs.randn(m, d), rs.randn(n, d), k, "plain")
    assert rep["guess"] == 1
    assert rep["overflowed"] == 0
    assert rep["guess_missed"] <= m // 32
    assert rep["rerun_rows"] == rep["guess_missed"]


def test_guess_off_is_the_same_output(native, monkeypatch, capfd):
    rs = np.random.RandomState(22)
    m, n, d, k = 256, 16384, 128, 100
    q, c = rs.randn(m, d), rs.randn(n, d)
    i1, s1, rep1 = screened_vs_plain(native, monkeypatch, capfd, q, c, k, "guess on")
    i0, s0, rep0 = screened_vs_plain(native, monkeypatch, capfd, q, c, k, "guess off", guess="0")
    assert rep1["guess"] == 1 and rep0["guess"] == 0 and rep0["guess_missed"] == 0
    assert np.array_equal(i1, i0) and same_bits(s1, s0)


def clustered(rs, d=128, clusters=64, per=256, a=0.75):
    """64 clusters of 256 near-duplicates (cosine with the centre about
    1 / sqrt(1 + a^2) = 0.8), cluster by cluster, so the seed's sample -- the
    first 1024 columns -- is clusters 0 .. 3 whole.  A query equal to one of
    those centres sees 256 sample scores near 0.8 and 768 near 0: mean 0.2,
    deviation 0.35, and a guess above every score the row has
    (tests/test_screen_guess_cpu.py::test_overshoot_is_flagged_not_finished)."""
    centres = rs.randn(clusters, d)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    noise = rs.randn(clusters * per, d) / np.sqrt(d) * a
    return centres, np.repeat(centres, per, axis=0) + noise


def test_clustered_corpus_overshoot_is_rerun(native, monkeypatch, capfd):
    rs = np.random.RandomState(23)
    m, k = 256, 100
    centres, c = clustered(rs)
    q = rs.randn(m, 128)
    q[:128] = centres[np.arange(128) % 4]  # one row block of queries at the centres of clusters 0 .. 3
    _, _, rep = screened_vs_plain(native, monkeypatch, capfd, q, c, k, "clustered")
    assert rep["guess"] == 1
    assert rep["guess_missed"] >= 128  # the block came back through the re-run
    assert rep["rerun_rows"] <= m // 8 + 1024 and rep["whole_call_f32"] == 0


@pytest.mark.parametrize("m,n,k", [(256, 8 * 1024, 192), (130, 16384, 100), (130, 70000, 100)])
def test_shapes(native, monkeypatch, capfd, m, n, k):
    # the smallest n the seed accepts at the largest k it accepts; one full and
    # one 2-row block; a corpus long enough for split units (S > 1), whose
    # segments share the proven bound while each starts from the guess
    rs = np.random.RandomState(m + n + k)
    _, _, rep = screened_vs_plain(native, monkeypatch, capfd, rs.randn(m, 128), rs.randn(n, 128), k, f"{m}x{n} k={k}")
    assert rep["guess"] == 1
    if n == 70000:
        assert rep["S"] > 1


def test_tied_kth(native, monkeypatch, capfd):
    # one corpus row repeated 300 times (> k): the rows near it have a k-th
    # score tied across more columns than k; ties go to the lower index
    rs = np.random.RandomState(24)
    m, n, d, k = 256, 16384, 128, 100
    c = rs.randn(n, d)
    rep_row = rs.randn(d)
    c[rs.choice(n, 300, replace=False)] = rep_row
    q = rs.randn(m, d)
    q[:64] = rep_row + 0.5 * rs.randn(64, d)
    screened_vs_plain(native, monkeypatch, capfd, q, c, k, "tied k-th")
