"""The cases, stride rungs and the read model of tests/test_gpu_wide_strides.py and
tests/test_wide_strides_cpu.py.  Nothing here touches a GPU.

Base shapes: m = 33 queries, n = 300 corpus rows, k = 10, d = 37 and 256: small enough that one
operand at a stride of 2^23 bytes and more stays under 6 GiB, ragged in d, more than one tile in n.
A route that needs a longer corpus takes the largest stride on the query side and a corpus stride
its memory allows.

Every f32 / bf16 case carries `launches`: timing name -> count of one call (pmm_timing_read
matches substrings), the report that the forced route ran; and `wide`: operand -> stride in bytes.
"""
from __future__ import annotations

import os
import re

import numpy as np

import device_cases as dc
from device_cases import COS, DOT, EUC, SCREEN_ON, topk_case

M, N, K, DIMS, METRICS = 33, 300, 10, (37, 256), (COS, DOT, EUC)
METRIC_NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
ELEM = {"f32": 4, "bf16": 2, "f64": 8, "i8": 1, "bits": 1}

# pmm_internal.h: one buffer descriptor ends at kDescMaxBytes; a GEMM's spans at most kDescRowsMax rows
_HDR = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "polars-matmul_amd", "csrc",
                         "pmm_internal.h")).read()
DESC_ROWS_MAX = int(re.search(r"constexpr int kDescRowsMax = (\d+);", _HDR).group(1))
DESC_MAX_BYTES = int(re.search(r"constexpr int64_t kDescMaxBytes = (0x[0-9A-Fa-f]+)ll;", _HDR).group(1), 16)
LIMIT_BYTES = (DESC_MAX_BYTES // DESC_ROWS_MAX) & ~15  # kMaxRowStrideBytes
assert DESC_MAX_BYTES == (1 << 31) - 1

# the spans of the f32 and bf16 GEMMs, in rows (GemmShape::BN of the six variants and the 32 query
# rows of a wave; kBf16BN, kBf16WsBN, kBf16FfBN and the fire-and-forget kernel's 64 rows per wave)
TILE_ROWS = (32, 64, 128, 256)
assert max(TILE_ROWS) == DESC_ROWS_MAX


def clamp_stride(R):
    """The rows of the upper half of an R-row span start past 2^31 bytes, none past 2^32."""
    return (1 << 31) // (R // 2) + 512


def wrap_stride(R):
    """The rows of the upper half of an R-row span start past 2^32 bytes."""
    return (1 << 32) // (R // 2) + 512


# the other entries index with 64-bit products; R is the operand's whole height
TOPK_RUNGS = {"c": {"first": (1 << 23) + 512, "both": (1 << 24) + 512},       # n = 300
              "q": {"first": (1 << 26) + 512, "both": (144 << 20) + 512}}    # m = 33
ROW_RUNGS = {"first": (1 << 25) + 512, "both": (1 << 26) + 512}              # 70 rows
MERGE_LIST_STRIDE = (1 << 28) + 64                                           # entries; 5 lists
for rows, rungs in ((N, TOPK_RUNGS["c"]), (M, TOPK_RUNGS["q"]), (70, ROW_RUNGS)):
    assert 1 << 31 <= rows * rungs["first"] and (rows - 1) * rungs["first"] < 1 << 32 <= (rows - 1) * rungs["both"]
    assert rows * rungs["both"] < 6 << 30


def refused_strides(kind):
    """Element strides the f32 / bf16 entries must refuse: one granule (16 bytes) above the limit,
    and the strides at which each span of TILE_ROWS would clamp or wrap."""
    nbytes = [LIMIT_BYTES + 16] + [f(R) for R in TILE_ROWS for f in (clamp_stride, wrap_stride)]
    assert min(nbytes) > LIMIT_BYTES
    return [b // ELEM[kind] for b in nbytes]


def _case(route, kind, m, n, d, k, metric, knobs, launches, wide=None):
    case = topk_case(f"{kind} {route} {METRIC_NAME[metric]} d={d}", kind, m, n, d, k, metric, knobs)
    case.launches = dict(launches)
    case.wide = wide or {"q": LIMIT_BYTES, "c": LIMIT_BYTES}
    for nm, rows in (("q", m), ("c", n)):
        assert rows * case.wide[nm] < 6 << 30
    return case


SEED = {"PMM_SEED": "1"}
# (route, knobs, launches).  n = 300: the sample is min(n, 256) rows, 256 * LIMIT_BYTES is the
# descriptor's last 4 KiB: the seeds run at the largest stride
F32_ROUTES = ([(f"variant {v}", {"PMM_GEMM_VARIANT": str(v)}, {f"f32_variant/{v}": 1, "gemm_f32_topk": 1})
               for v in range(6)]
              + [("variant 5 whole blocks", {"PMM_GEMM_VARIANT": "5", "PMM_CUS": "4"}, {"f32_variant/5": 1}),
                 ("seeded", SEED, {"gemm_f32_seed": 1, "seed_form/": 1, "seed_select": 0}),
                 ("seeded by the GEMM", {**SEED, "PMM_SEED_GEMM": "1"},
                  {"gemm_f32_seed": 1, "seed_select": 1, "seed_form/": 0}),
                 ("seeded LDS blocks", {**SEED, "PMM_SEED_LDS": "1"}, {"gemm_f32_seed": 1, "seed_form/lds": 1}),
                 ("seeded fmaf blocks", {**SEED, "PMM_SEED_MFMA": "0"}, {"gemm_f32_seed": 1, "seed_form/fmaf": 1}),
                 ("seeded MFMA blocks", {**SEED, "PMM_SEED_MFMA": "1"}, {"gemm_f32_seed": 1, "seed_form/mfma": 1})])
F32_CASES = [_case(route, "f32", M, N, d, K, metric, knobs, launches)
             for route, knobs, launches in F32_ROUTES for metric in METRICS for d in DIMS]
F32_CASES += [_case("screened", "f32", M, N, d, K, COS, SCREEN_ON, {"gemm_f32_topk/screen": 1}) for d in DIMS]
# the materialised route needs k > 1024: the shape of device_cases, the queries at the largest
# stride, the corpus at the widest its 4099 rows leave under the memory cap
MID = (1 << 20) + 512
F32_CASES += [_case("materialised k=1025", "f32", 64, 4099, 256, 1025, metric, {},
                    {"gemm_f32_scores": 1, "gemm_f32_topk": 0}, {"q": LIMIT_BYTES, "c": MID}) for metric in METRICS]
# a 512-row sample at the largest corpus stride does not fit one descriptor: the call runs unseeded
F32_SEED_SKIPPED = [_case("seed of 512 rows", "f32", M, 600, 37, K, metric, {**SEED, "PMM_SEED_NS": "512"},
                          {"gemm_f32_seed": 1}) for metric in METRICS]

WS, ONE = {"gemm_bf16_topk/ws": 1, "gemm_bf16_topk/one-wave": 0}, {"gemm_bf16_topk/ws": 0, "gemm_bf16_topk/one-wave": 1}
BF16_CASES = [_case(route, "bf16", M, n, d, K, metric, knobs, launches, wide)
              for route, knobs, n, launches, wide in (
                  ("wave-specialised", {}, N, WS, None),
                  ("one-wave", {"PMM_BF16_WS": "0"}, N, ONE, None),
                  ("unseeded", {"PMM_BF16_SEED": "0", "PMM_SEED_NS": "64"}, 600, {**WS, "seed_bf16": 0}, None),
                  # (the seed wants 4 k <= ns and n >= 8 ns)
                  ("seeded, sample of 64", {"PMM_BF16_SEED": "1", "PMM_SEED_NS": "64"}, 600, {**WS, "seed_bf16": 1}, None),
                  # its default sample of 1024 rows: n = 8192, the corpus at 2^19 + 512 bytes (4.3 GB)
                  ("seeded, default sample", {}, 8192, {**WS, "seed_bf16": 1}, {"q": LIMIT_BYTES, "c": (1 << 19) + 512}))
              for metric in METRICS for d in DIMS]
# the fire-and-forget kernel of the test library (64 query rows per wave, 32-column tiles, a
# sample of 256 rows at n = 4099), forced with PMM_BF16_FF=2; its K-step instantiations d / 128 =
# 1 and 2 as for the other bf16 kernels
FF_CASES = [_case("fire-and-forget", "bf16", 70, 4099, d, K, metric, {"PMM_BF16_FF": "2"},
                  {"gemm_bf16_topk/ff": 1, "seed_bf16": 1}, {"q": LIMIT_BYTES, "c": MID})
            for metric in METRICS for d in DIMS]
for _c in FF_CASES:
    # (the test library's re-run of unproven rows gathers whole strides of the query rows: the
    # last row is placed with its stride, where the product's entries end it at the padded width)
    _c.whole_rows = True

SOUND_CASES = [topk_case(f"f64 {route} {METRIC_NAME[metric]} d={d}", "f64", M, N, d, K, metric, knobs)
               for route, knobs in (("fused", {"PMM_F64_FUSED": "1"}), ("materialised", {"PMM_F64_FUSED": "0"}))
               for metric in METRICS for d in DIMS]
SOUND_CASES += [topk_case(f"i8 {METRIC_NAME[metric]} d={d}", "i8", M, N, d, K, metric) for metric in METRICS for d in DIMS]
SOUND_CASES += [topk_case(f"bits d={d}", "bits", M, N, d, K, COS) for d in DIMS]


# ---------------------------------------------------------------------------
# What a kernel would read through a clamped descriptor with 32-bit offsets
# ---------------------------------------------------------------------------
def misread_rows(rows, R, stride, width, wrap):
    """`rows` (float) as read in spans of R rows based at the span's first row, at `stride` bytes
    per row, `width` bytes read of each.  wrap = False: 64-bit offsets, the descriptor clamped at
    2^31 - 1 bytes -- a row that ends past it reads as zeros.  wrap = True: the offset also taken
    modulo 2^32 first -- the row reads as the row the wrapped offset addresses, or, where that is
    no row's start, as the poison behind a row (NaN)."""
    out = rows.copy()
    for i in range(rows.shape[0]):
        off = (i % R) * stride
        if wrap and off >= 1 << 32:
            off %= 1 << 32
            j, within = divmod(off, stride)
            out[i] = rows[i - i % R + j] if within == 0 and i - i % R + j < rows.shape[0] else np.nan
        if off + width > DESC_MAX_BYTES:
            out[i] = 0
    return out
