"""The row-chunk loops of the materialised paths and the matmul entries as a table of cases.

Four host loops of pmm_capi.hip cut a call into row chunks so that one score or result block
stays under the materialise budget (2 GiB): pmm_matmul_f32, pmm_matmul_f64, topk_f32_materialised
and topk_f64_materialised (also the f64 fused scan's overflow fallback and a sharded search's
deferred re-run).  PMM_MATERIALISE_BUDGET (bytes, a test knob: DESIGN.md §9) lowers the budget so
that the shapes below run the loops past their first chunk.  tests/test_gpu_row_chunks.py runs the
cases; tests/test_row_chunks_cpu.py pins the conditions on the table and the plan restated here.

The plan's rule (plan_materialise and the two matmul entries), restated:

  per_row  n * elem bytes; on the global-sort form of a top-k, n * elem + next_pow2(n) * 16
  rows     max(1, min(m, budget // per_row))

A budget of R * per_row therefore gives chunks of R rows and ceil(m / R) launches of the chunked
GEMM.  Nothing here touches a GPU at import.
"""
from __future__ import annotations

import functools

import numpy as np

from value_cases import value_case

COS, DOT, EUC = 0, 1, 2
METRICS = (COS, DOT, EUC)
KNOB = "PMM_MATERIALISE_BUDGET"
BUDGET = 1 << 31          # kMaterialiseBudget
ROWSEL_MAX_P = 4096       # kRowSelMaxP: the row select's largest per-row buffer
FUSED_MAX_K = 1024        # kFusedMaxK: f32 calls above it are materialised


def next_pow2(x, lo):
    p = lo
    while p < x:
        p <<= 1
    return p


def al256(x):
    return -(-x // 256) * 256


def rowsel_p(k):
    return next_pow2(2 * min(k, 1 << 20) + 64, 128)


def global_sort(k):
    return k > (ROWSEL_MAX_P - 64) // 2 or rowsel_p(k) > ROWSEL_MAX_P


def per_row(n, elem, k=None):
    """Bytes of one row of a chunk: k None for a matmul (the result row alone)."""
    return n * elem + (next_pow2(n, 2) * 16 if k is not None and global_sort(k) else 0)


def plan_rows(m, row_bytes, budget=BUDGET):
    return max(1, min(m, budget // row_bytes))


def chunks(m, rows):
    return -(-m // rows)


def budget_of(rows, row_bytes):
    """The knob's value for chunks of `rows` rows."""
    return str(rows * row_bytes)


def materialised_bytes(m, n, k, elem, budget=BUDGET):
    """plan_materialise's total: counter | query norms | corpus norms | score chunk | sort keys."""
    rows = plan_rows(m, per_row(n, elem, k), budget)
    keys = rows * next_pow2(n, 2) * 16 if global_sort(k) else 0
    return 256 + al256(m * elem) + al256(n * elem) + al256(rows * n * elem) + al256(keys)


def parse_knob(text):
    """What materialise_budget() makes of the knob's text: decimal digits naming 1 .. 2^31, else the constant."""
    if not text or not text.isascii() or not text.isdigit():
        return BUDGET
    v = int(text)
    return v if 1 <= v <= BUDGET else BUDGET


class Case:
    """kind "matmul" or "topk"; ks and metrics: every combination runs; rows: the listed R;
    env: knobs of the case beside the budget; label: the chunked GEMM's timing label."""

    def __init__(self, name, kind, dtype, m, n, d, rows, make, ks=(None,), metrics=(None,), env=None):
        self.name, self.kind, self.dtype = name, kind, np.dtype(dtype)
        self.m, self.n, self.d, self.rows, self.ks, self.metrics = m, n, d, tuple(rows), tuple(ks), tuple(metrics)
        self._make, self.env = make, dict(env or {})
        f64 = self.dtype == np.float64
        self.label = ("gemm_f64_" if f64 else "gemm_f32_") + ("matmul" if kind == "matmul" else "scores")

    def __repr__(self):
        return self.name

    @property
    def elem(self):
        return self.dtype.itemsize

    def per_row(self, k=None):
        return per_row(self.n, self.elem, k)

    def budget(self, rows, k=None):
        return budget_of(rows, self.per_row(k))

    @functools.lru_cache(maxsize=None)
    def data(self, metric=None, k=None):
        """(q, c): built once per (metric, k) and left unchanged."""
        q, c = self._make(self, metric, k)
        q, c = np.ascontiguousarray(q, self.dtype), np.ascontiguousarray(c, self.dtype)
        q.setflags(write=False)
        c.setflags(write=False)
        return q, c

    def second_chunk_rows(self):
        """One query row inside the second chunk of every listed R (and of no other R's first)."""
        return sorted({min(r + r // 2, self.m - 1) for r in self.rows if r < self.m})


# ---------------------------------------------------------------------------
# matmul
# ---------------------------------------------------------------------------
# Query rows that take the planted rows of the padded shape: one in the second chunk of every
# R in {1, 5, 32, 33, 66} and the last row (the last chunk of each; the second of R = 66).
ZERO_SUM_ROWS = (1, 6, 40, 66)     # copies of value_cases' signed_zero q[0] / q[1]: sums of -0.0 and +0.0
ZERO_QUERY_ROWS = (7, 41, 65)      # all-zero query rows (+0.0, -0.0, +0.0)


def matmul_padded(case, metric, k):
    """d = 37 pads to 64 (f32) and 48 (f64): the per-chunk sign pass runs on shifted pointers.
    value_cases' signed_zero inputs, its rows q[0] and q[1] copied to ZERO_SUM_ROWS."""
    q, c = value_case("signed_zero", case.dtype, case.m, case.n, case.d, seed=3)
    q = q.copy()
    for j, r in enumerate(ZERO_SUM_ROWS):
        q[r] = q[j % 2]
    for j, r in enumerate(ZERO_QUERY_ROWS):
        q[r] = -0.0 if j % 2 else 0.0
    return q, c


def matmul_tile_height(case, metric, k):
    """300 rows against the 256-row tile height, d = 256 unpadded; an all-zero row in the last chunk."""
    rs = np.random.RandomState(300 + case.elem)
    q, c = rs.randn(case.m, case.d), rs.randn(case.n, case.d)
    q[299] = 0.0
    q[256] = -q[0]
    return q, c


PADDED_ROWS = (1, 5, 32, 33, 66, 67)   # (67: the budget of exactly the whole call, one chunk)
TILE_ROWS = (255, 256, 257, 299)
MATMUL_CASES = [
    Case("matmul f32 padded 67x301x37", "matmul", np.float32, 67, 301, 37, PADDED_ROWS, matmul_padded),
    Case("matmul f32 300x130x256", "matmul", np.float32, 300, 130, 256, TILE_ROWS, matmul_tile_height),
    Case("matmul f64 padded 67x301x37", "matmul", np.float64, 67, 301, 37, PADDED_ROWS, matmul_padded),
    Case("matmul f64 300x130x256", "matmul", np.float64, 300, 130, 256, TILE_ROWS, matmul_tile_height),
]


# ---------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------
DUPLICATES = 7      # copies of one corpus row: ranks k - 3 .. k + 3 of the starred query rows
NAN_ROW, ZERO_ROW = 11, 23


def score64(qrow, c, metric):
    """Approximate scores in f64, better first under argsort: ranking only, never compared."""
    with np.errstate(all="ignore"):
        c64, q64 = c.astype(np.float64), qrow.astype(np.float64)
        dot = c64 @ q64
        if metric == DOT:
            return -dot
        if metric == COS:
            return -dot / (np.linalg.norm(c64, axis=1) * np.linalg.norm(q64) + 1e-300)
        return ((c64 - q64) ** 2).sum(axis=1)


def planted_topk(case, metric, k):
    """randn rows; the starred query rows (case.second_chunk_rows() and the last row) are one
    vector; the corpus row at its rank k - 3 stands DUPLICATES times in the corpus (in place of
    rows ranked last), so exact ties straddle the k-th place; one corpus row holds a NaN, one is
    all zero (a zero norm)."""
    rs = np.random.RandomState(case.m + case.n + case.d + 7 * (metric or 0))
    q, c = rs.randn(case.m, case.d).astype(case.dtype), rs.randn(case.n, case.d).astype(case.dtype)
    star = case.second_chunk_rows() + [case.m - 1]
    q[star] = q[star[0]]
    order = np.argsort(score64(q[star[0]], c, metric), kind="stable")
    order = order[~np.isin(order, (NAN_ROW, ZERO_ROW))]
    kk = min(k, case.n - 2 * DUPLICATES)
    proto = order[kk - 4]
    # spread through the corpus: rows ranked last, lowest and highest index first
    worst = np.sort(order[-200:])
    take = np.concatenate([worst[:3], worst[-3:]])
    c[take] = c[proto]
    c[NAN_ROW, 1] = np.nan
    c[ZERO_ROW] = 0.0
    return q, c


def duplicate_rows(case, metric, k):
    """The corpus rows of planted_topk's duplicate group (the prototype and its six copies)."""
    _, c = case.data(metric, k)
    rows, inverse, counts = np.unique(c, axis=0, return_inverse=True, return_counts=True)
    group = np.flatnonzero(counts == DUPLICATES)
    assert group.size == 1, (case.name, counts.max())
    return np.flatnonzero(inverse.reshape(-1) == group[0])


F64_OFF = {"PMM_F64_FUSED": "0"}
F32_ROWSEL = Case("f32 row select 70x9001x40", "topk", np.float32, 70, 9001, 40, (1, 7, 32, 69), planted_topk,
                  ks=(1025,), metrics=METRICS)
F32_GSORT = Case("f32 global sort 33x8192x96", "topk", np.float32, 33, 8192, 96, (1, 16, 32), planted_topk,
                 ks=(3000,), metrics=(COS, EUC))
F64_ROWSEL = Case("f64 row select 33x5000x24", "topk", np.float64, 33, 5000, 24, (1, 10, 32), planted_topk,
                  ks=(10, 1100), metrics=METRICS, env=F64_OFF)
F64_GSORT = Case("f64 global sort 9x4100x24", "topk", np.float64, 9, 4100, 24, (1, 4, 8), planted_topk,
                 ks=(3000,), metrics=METRICS, env=F64_OFF)
TOPK_CASES = [F32_ROWSEL, F32_GSORT, F64_ROWSEL, F64_GSORT]


def ascending(case, metric, k):
    """tests/test_gpu_parity.py::test_f64_fused_overflow_falls_back's corpus: every row beats
    every earlier one, so the fused scan's buffers overflow.  The query rows differ by a positive
    factor (a chunk that read another chunk's rows would return their scores)."""
    c = np.repeat(np.arange(case.n, dtype=np.float64)[:, None], case.d, axis=1) / case.n
    q = np.ones((case.m, case.d)) * (1.0 + np.arange(case.m)[:, None] / 64.0)
    return q, c


# 40 rows in chunks of 13 (4 chunks, the last of one row) and 7 (6 chunks)
F64_FALLBACK = Case("f64 fused-scan fallback 40x20000x16", "topk", np.float64, 40, 20000, 16, (13, 7), ascending,
                    ks=(10,), metrics=(DOT,), env={"PMM_F64_FUSED": "1"})
# the sharded form (tests/test_gpu_host_frame.py::test_f64_overflowed_shards_rerun_after_every_device):
# two shards of 2000 rows, each re-run materialised in chunks of R rows
F64_SHARDED = Case("f64 sharded re-run 12x4000x16", "topk", np.float64, 12, 4000, 16, (5, 1), ascending,
                   ks=(10,), metrics=(DOT,), env={"PMM_F64_FUSED": "1"})
SHARDS = 2


# the device entries (index_base = 1000, row strides above the padded d) and the handles
INDEX_BASE = 1000
F32_DEVICE = Case("f32 device entry 37x1500x37", "topk", np.float32, 37, 1500, 37, (16, 5), planted_topk,
                  ks=(1025,), metrics=(COS,))
F64_DEVICE = Case("f64 device entry 37x1500x37", "topk", np.float64, 37, 1500, 37, (16, 5), planted_topk,
                  ks=(1100,), metrics=(EUC,), env=F64_OFF)
F32_HANDLE = Case("f32 handle 37x1500x37", "topk", np.float32, 37, 1500, 37, (16, 5), planted_topk,
                  ks=(1025,), metrics=METRICS)
F64_HANDLE = Case("f64 handle 37x1500x37", "topk", np.float64, 37, 1500, 37, (16, 5), planted_topk,
                  ks=(1100,), metrics=METRICS, env=F64_OFF)
ENTRY_CASES = [F32_DEVICE, F64_DEVICE, F32_HANDLE, F64_HANDLE]

ALL_CASES = MATMUL_CASES + TOPK_CASES + [F64_FALLBACK, F64_SHARDED] + ENTRY_CASES


def shard_rows(case):
    return case.n // SHARDS


# ---------------------------------------------------------------------------
# The real budget, knob unset: the first chunk is exactly 2^31 bytes
# ---------------------------------------------------------------------------
FULL_M, FULL_N, FULL_D, FULL_K = 1030, 524288, 8, 1025
FULL_CHUNK = 1024                       # BUDGET // (FULL_N * 4)
FULL_PAIRS = tuple((r, FULL_CHUNK + r) for r in range(FULL_M - FULL_CHUNK))
FULL_SAMPLE = sorted({0, 1023, 1024, 1029} | {int(x) for x in np.linspace(2, 1021, 64)})


@functools.lru_cache(maxsize=None)
def full_size_inputs():
    """f32 1030 x 524288 x 8; query rows 1024 .. 1029 are copies of rows 0 .. 5."""
    rs = np.random.RandomState(2031)
    q = rs.randn(FULL_M, FULL_D).astype(np.float32)
    c = rs.randn(FULL_N, FULL_D).astype(np.float32)
    for a, b in FULL_PAIRS:
        q[b] = q[a]
    q.setflags(write=False)
    c.setflags(write=False)
    return q, c
