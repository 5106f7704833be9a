"""The screened f32 path's slack (screen_eps, csrc/pmm_device.h), restated in
NumPy and checked against emulated arithmetic: bf16 round-to-nearest-even by
bit operations, the bf16 product accumulated in f32 (in two different orders,
the kernel's is not documented) and the exact path's k-ordered f32 fmaf chain.
An empirical check is not the proof, but it catches a wrong
constant.
"""
from __future__ import annotations

import numpy as np

from parity import round_bf16


def screen_eps(rq, rc, dp):
    rnd = rq * (1.0 + rc) + rc
    accum = dp * (8.0 * (1.0 + 2.0 ** -7) + 2.0) * 2.0 ** -24
    return (rnd + accum) * (1.0 + 2.0 ** -9) + 2.0 ** -20


def rel_residual(x):
    """The pass's per-row bound of ||x - bf16(x)|| / ||x||."""
    x64 = x.astype(np.float64)
    r = x64 - round_bf16(x).astype(np.float64)
    return min(np.sqrt((r * r).sum() / (x64 * x64).sum()) * (1.0 + 2.0 ** -9), 2.0 ** -8)


def fma_chain(q, c):
    # f32 fmaf chain in natural K order: the product is exact in f64, one
    # rounding per step (double rounding f64 -> f32 differs from a true fmaf
    # only in ties of the 53-bit sum, far inside the bound under test)
    acc = np.float32(0.0)
    for a, b in zip(q, c):
        acc = np.float32(np.float64(a) * np.float64(b) + np.float64(acc))
    return acc


def bf16_dots(qb, cb):
    """f32 accumulation of the bf16 products: sequential, and pairwise in blocks of 32."""
    p = qb.astype(np.float64) * cb.astype(np.float64)  # bf16 x bf16 is exact in f32
    seq = np.float32(0.0)
    for x in p:
        seq = np.float32(np.float64(seq) + x)
    blk = np.float32(0.0)
    for i in range(0, len(p), 32):
        v = p[i:i + 32].astype(np.float32)
        while len(v) > 1:
            if len(v) % 2:
                v = np.concatenate([v, np.zeros(1, np.float32)])
            v = (v[0::2] + v[1::2]).astype(np.float32)
        blk = np.float32(blk + v[0])
    return seq, blk


def vectors():
    rs = np.random.RandomState(0)
    tie = np.float32(1.0 + 2.0 ** -8)  # a half-ulp tie of bf16
    for d in (1, 37, 128, 700, 768):
        yield rs.randn(d).astype(np.float32), rs.randn(d).astype(np.float32)
        sg = rs.choice([-1.0, 1.0], d)
        # systematic rounding: every element a tie, aligned and mixed signs
        yield (tie * np.ones(d)).astype(np.float32), (tie * np.ones(d)).astype(np.float32)
        yield (tie * sg * np.exp2(rs.randint(-3, 4, d))).astype(np.float32), (tie * sg).astype(np.float32)
        yield (tie * sg).astype(np.float32), (tie * rs.choice([-1.0, 1.0], d)).astype(np.float32)
        # elements spanning 2^-30 .. 2^30
        yield ((rs.randn(d) * np.exp2(rs.randint(-30, 31, d))).astype(np.float32),
               (rs.randn(d) * np.exp2(rs.randint(-30, 31, d))).astype(np.float32))
        # one dominant element
        a, b = rs.randn(d).astype(np.float32), rs.randn(d).astype(np.float32)
        a[d // 2] = 1000.0
        b[d // 3] = -997.0
        yield a, b
        # near-parallel and near-orthogonal pairs
        yield a, (a * np.float32(1.0 + 1e-5) + np.float32(1e-6) * b).astype(np.float32)


def test_slack_covers_the_bf16_dot_against_the_exact_chain():
    worst = 0.0
    for q, c in vectors():
        d = len(q)
        dp = -(-d // 128) * 128
        nq, nc = np.linalg.norm(q.astype(np.float64)), np.linalg.norm(c.astype(np.float64))
        eps = screen_eps(rel_residual(q), rel_residual(c), dp)
        exact = float(fma_chain(q, c))
        for approx in bf16_dots(round_bf16(q), round_bf16(c)):
            err = abs(exact - float(approx)) / (nq * nc)
            worst = max(worst, err / eps)
            assert err <= eps, (d, err, eps)
    assert 0.0 < worst <= 1.0


def test_slack_is_about_two_bf16_half_ulps():
    # the bound for worst-case rows: 2^-8 relative residual on both sides
    e = screen_eps(2.0 ** -8, 2.0 ** -8, 768)
    assert 2.0 ** -7 < e < 2.0 ** -7 * 1.1
    # and for N(0,1) rows about 0.0023 + 0.0005 of accumulation terms
    rs = np.random.RandomState(1)
    r = rel_residual(rs.randn(768).astype(np.float32))
    assert 0.001 < r < 0.002
    assert screen_eps(r, r, 768) < 0.004
