"""Measurements of the bit-row route (profiles/bits/README.md).

  python tools/experiments/bits_search.py [--out FILE] [--reps N] [--shapes 4096x256,1000x768] [--n ROWS]

One process.  Per shape (m queries x n corpus rows from d-dimensional random
normal f32 rows, k = 100) four resident handles of the same corpus: the f32
handle (the source; exact top-100 for the recall figure), the bit handle packed
from it on the device (this route), the Int8 handle of the same signs as +-1
bytes searched by `dot` (the nearest capability before this route: the same
MFMA count at 8x the HBM bytes; the dot of +-1 rows is D - 2 * distance, the
same order) and the bf16 handle searched by cosine.  Per round the three calls
alternate; the first round warms up and is dropped; figures are medians with
the minimum and maximum.  Wall times are host clocks around calls that end in a
synchronise (query upload and list download included); kernel times are the
library's stream events (pmm_timing_read).  The bit lists are compared with a
NumPy restatement on a few query rows at the full size.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))

import polars_matmul  # noqa: E402
from polars_matmul import _native  # noqa: E402

K = 100
# cdna_hip_programming.md "MFMA rate per dtype": i8 = 2x the bf16 rate; MI355X_MICROARCH.md: bf16 ~2.5 PF dense
I8_PEAK_OPS = 5.0e15
ROUND_NORMS_BF16_TBS = 5.28  # the one-pass round_norms_bf16 kernel over the same read (profiles/bf16_corpus)
KERNELS = ("bits_popcount", "gemm_bits_topk", "select_bits", "bits_finish", "bits_gather", "h2d", "d2h")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def restated(qb, cb, rows, k):
    """The restatement of tests/test_bits_cpu.py for a few query rows."""
    table = np.array([bin(i).count("1") for i in range(256)], np.uint16)
    idx, sc = [], []
    for i in range(rows):
        dist = table[np.bitwise_xor(cb, qb[i][None, :])].sum(1, dtype=np.int64)
        o = np.argsort(dist, kind="stable")[:k]
        idx.append(o.astype(np.uint32))
        sc.append(dist[o].astype(np.float64))
    return np.stack(idx), np.stack(sc)


def measure(m, n, d, reps):
    rng = np.random.default_rng(m + d)
    q = rng.standard_normal((m, d), dtype=np.float32)
    c = rng.standard_normal((n, d), dtype=np.float32)
    res = {"m": m, "n": n, "d": d, "w": -(-d // 8), "k": K}
    _native.timing_enable(True)
    hf = _native.DeviceCorpus(c)
    res["bytes_f32"] = hf.nbytes
    packs = []
    for _ in range(reps + 1):  # the pack kernel: a fresh bit handle per round, the last one kept
        _native.timing_reset()
        hb = hf.sign_bits()
        packs.append(_native.timing_read("pack_sign")[0])
        if len(packs) <= reps:
            hb.close()
    res["pack_ms"] = spread(packs[1:])
    res["pack_gb_per_s"] = (4.0 * n * d + n * res["w"]) / (res["pack_ms"]["median"] * 1e-3) / 1e9
    res["pack_share_of_round_norms_bf16"] = res["pack_gb_per_s"] / (ROUND_NORMS_BF16_TBS * 1e3)
    res["bytes_bits"] = hb.nbytes
    qb, cb = polars_matmul.pack_sign(q), polars_matmul.pack_sign(c)
    q1 = (q > 0).astype(np.int8) * np.int8(2) - np.int8(1)
    hi8 = _native.DeviceCorpus.int8((c > 0).astype(np.int8) * np.int8(2) - np.int8(1))
    res["bytes_i8"] = hi8.nbytes
    hbf = _native.DeviceCorpus(c, compute="bf16")
    res["bytes_bf16"] = hbf.nbytes
    wall = {"bits": [], "i8_dot": [], "bf16_cosine": []}
    kern = {name: [] for name in KERNELS}
    i8_gemm = []
    got = None
    for rep in range(reps + 1):
        _native.timing_reset()
        tb, got = timed(lambda: hb.topk(qb, K))
        ks = {name: _native.timing_read(name)[0] for name in KERNELS}
        _native.timing_reset()
        t8, got8 = timed(lambda: hi8.topk(q1, K, _native.METRIC_DOT))
        g8 = _native.timing_read("gemm_i8_topk")[0]
        tbf, _ = timed(lambda: hbf.topk(q, K, _native.METRIC_COSINE))
        if rep:
            wall["bits"].append(tb)
            wall["i8_dot"].append(t8)
            wall["bf16_cosine"].append(tbf)
            i8_gemm.append(g8)
            for name in KERNELS:
                kern[name].append(ks[name])
    _native.timing_enable(False)
    wi, ws = restated(qb, cb, 4, K)
    res["equal_to_restatement_rows_0_3"] = bool(np.array_equal(got[0][:4], wi) and np.array_equal(got[1][:4], ws))
    res["same_lists_as_i8_dot"] = bool(np.array_equal(got[0], got8[0]))
    res["wall_ms"] = {k: spread(v) for k, v in wall.items()}
    res["bits_kernel_ms"] = {k: spread(v) for k, v in kern.items()}
    res["i8_gemm_ms"] = spread(i8_gemm)
    dp = -(-res["w"] // 16) * 16
    gemm = res["bits_kernel_ms"]["gemm_bits_topk"]["median"]
    res["gemm_bits_fraction_of_i8_peak"] = 2.0 * m * n * 8 * dp / (gemm * 1e-3) / I8_PEAK_OPS
    res["ratio_i8_over_bits"] = res["wall_ms"]["i8_dot"]["median"] / res["wall_ms"]["bits"]["median"]
    res["ratio_bf16_over_bits"] = res["wall_ms"]["bf16_cosine"]["median"] / res["wall_ms"]["bits"]["median"]
    for name in ("f32", "bf16", "i8"):
        res[f"bytes_{name}_over_bits"] = res[f"bytes_{name}"] / res["bytes_bits"]
    # for information: recall@100 of "4 k Hamming, then exact re-rank" against the exact f32 top-100
    mr = min(m, 256)
    exact = hf.topk(q[:mr], K, _native.METRIC_COSINE)[0]
    near = np.sort(hb.topk(qb[:mr], 4 * K)[0], axis=1)
    offsets = np.arange(mr + 1, dtype=np.int64) * (4 * K)
    rer = hf.topk_candidates(q[:mr], offsets, near.reshape(-1), K, _native.METRIC_COSINE)[0]
    res["recall_at_100_of_4k_hamming_then_rerank"] = float(np.mean(
        [len(set(exact[i].tolist()) & set(rer[i].tolist())) / K for i in range(mr)]))
    for h in (hb, hi8, hbf, hf):
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bits", "measure.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="4096x256,1000x768")
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    out = {"peak_ops_assumed": I8_PEAK_OPS, "round_norms_bf16_tb_per_s": ROUND_NORMS_BF16_TBS, "shapes": []}
    for spec in a.shapes.split(","):
        m, d = (int(x) for x in spec.split("x"))
        r = measure(m, a.n, d, a.reps)
        out["shapes"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
