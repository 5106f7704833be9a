"""Inputs outside the comfortable value range, shared by the value-range tests.

``value_cases(dtype, m, n, d, seed)`` yields ``(name, q, c)`` for five cases
whose oracle lists hold subnormal scores, signed zeros, infinities and NaN (see
``CASES``).  The constants depend on the width: the f32 ones put products and
norms at the edges of f32's exponent range, the f64 ones at the edges of f64's.

A plain module: ``tests/test_value_cases.py`` pins, on the oracle alone, that
every case still produces the score class it exists for.
"""
from __future__ import annotations

import numpy as np

CASES = ("row_scales", "underflow", "overflow", "signed_zero", "nonfinite")

# The corpus rows ``signed_zero`` and ``nonfinite`` plant (n >= 300): a subset
# mask or a group labelling that wants to spread the planted rows reads these.
SIGNED_ZERO_ROWS = tuple(5 + 41 * j for j in range(7)) + (299,)
NONFINITE_ROWS = (3, 50, 120, 130, 200, 210, 260, 290)


def _consts(dtype):
    f32 = np.dtype(dtype) == np.float32
    return dict(scale_exp=40 if f32 else 300, under=-68 if f32 else -520, over=62 if f32 else 510,
                tiny=1e-30 if f32 else 1e-200)


def _pair(rs, dtype, m, n, d):
    return rs.randn(m, d).astype(dtype), rs.randn(n, d).astype(dtype)


def row_scales(dtype, m, n, d, rs):
    """randn rows, each times 2^e with its own integer e: scores over ~4e
    binades, norms on both sides of cosine's threshold."""
    e = _consts(dtype)["scale_exp"]
    q, c = _pair(rs, dtype, m, n, d)
    q = np.ldexp(q, rs.randint(-e, e + 1, size=(m, 1))).astype(dtype)
    c = np.ldexp(c, rs.randint(-e, e + 1, size=(n, 1))).astype(dtype)
    return q, c


def underflow(dtype, m, n, d, rs):
    """Both sides tiny: every dot product is subnormal, every norm under
    cosine's threshold, every squared distance subnormal."""
    q, c = _pair(rs, dtype, m, n, d)
    u = _consts(dtype)["under"]
    return np.ldexp(q, u).astype(dtype), np.ldexp(c, u).astype(dtype)


def overflow(dtype, m, n, d, rs):
    """Both sides huge, every 3rd corpus row and every 4th query row 4 times
    larger still: norm products overflow (cosines of -0.0 and +0.0), dot
    products overflow to +-inf, and inf - inf makes NaN."""
    q, c = _pair(rs, dtype, m, n, d)
    o = _consts(dtype)["over"]
    q, c = np.ldexp(q, o).astype(dtype), np.ldexp(c, o).astype(dtype)
    c[::3] *= 4
    q[::4] *= 4
    return q, c


def signed_zero(dtype, m, n, d, rs):
    """Planted rows whose dot products with q[0] and q[1] are +-t^2, which
    underflows to a zero with a sign, or exactly zero: -0.0 and +0.0 scores
    interleaved by index (SIGNED_ZERO_ROWS)."""
    assert m >= 3 and n >= 300 and d >= 4
    q, c = _pair(rs, dtype, m, n, d)
    t = dtype(_consts(dtype)["tiny"])
    e = np.eye(d, dtype=dtype)
    q[0] = e[0] + t * e[-1]
    q[1] = -e[0] - t * e[-1]
    rows = SIGNED_ZERO_ROWS
    c[rows[0]] = e[1] + t * e[-1]    # q0: +t^2 -> +0.0     q1: -t^2 -> -0.0
    c[rows[1]] = e[1] - t * e[-1]    # q0: -0.0             q1: +0.0
    c[rows[2]] = e[1]                # exactly +0.0 for both
    c[rows[3]] = -e[1] - t * e[-1]   # q0: -0.0             q1: +0.0
    c[rows[4]] = -e[1] + t * e[-1]   # q0: +0.0             q1: -0.0
    c[rows[5]] = -e[1]               # +0.0
    c[rows[6]] = e[1] - t * e[-1]    # q0: -0.0             q1: +0.0
    c[rows[7]] = dtype(-0.0)         # an all -0.0 row: zero norm
    q[2, :3] = dtype(-0.0)
    return q, c


def nonfinite(dtype, m, n, d, rs):
    """NaN, +inf and -inf elements on both sides, zero rows, exact ties."""
    assert m >= 5 and n >= 300 and d >= 4
    q, c = _pair(rs, dtype, m, n, d)
    r = NONFINITE_ROWS
    c[r[0], 1] = np.nan
    c[r[1], 2] = np.inf
    c[r[2], 0] = -np.inf
    c[r[3], 0], c[r[3], d - 1] = np.inf, -np.inf
    c[r[4]] = 0.0
    c[r[5]] = c[r[6]] = c[7]  # one row three times
    q[0, 3] = np.nan
    q[1, 0] = np.inf
    q[2, d - 1] = -np.inf
    q[3] = 0.0
    return q, c


_BUILD = {"row_scales": row_scales, "underflow": underflow, "overflow": overflow, "signed_zero": signed_zero,
          "nonfinite": nonfinite}


def value_case(name, dtype, m, n, d, seed=0):
    dtype = np.dtype(dtype).type
    rs = np.random.RandomState(1000 * seed + 17 * CASES.index(name) + (0 if dtype == np.float32 else 7))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        q, c = _BUILD[name](dtype, m, n, d, rs)
    return np.ascontiguousarray(q, dtype), np.ascontiguousarray(c, dtype)


def value_cases(dtype, m, n, d, seed=0):
    """Yields (name, q, c) for the five cases; q is (m, d), c is (n, d)."""
    for name in CASES:
        q, c = value_case(name, dtype, m, n, d, seed)
        yield name, q, c
