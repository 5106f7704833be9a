"""Measurements of the int8 route (profiles/int8/README.md).

  python tools/experiments/int8_search.py [--out FILE] [--reps N] [--shapes 4096x256,1000x768] [--n ROWS]

One process.  Per shape (m queries x n corpus rows x d, k = 100, cosine) three
resident handles of the same uniform int8 values: the int8 handle (this
route), the f64 handle (what an Int8 column took before: leg a) and the bf16
handle (leg b).  Per round the three calls alternate; the first round warms up
and is dropped; figures are medians with the minimum and maximum.  Wall times
are host clocks around calls that end in a synchronise (query upload and list
download included); kernel times are the library's stream events
(pmm_timing_read).  The int8 lists are compared with the f64 handle's, bit for
bit, at the full size.  The band (candidates a row hands to the finish) is
counted on the host for a few query rows from the NumPy restatement of the key.
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

from polars_matmul import _native  # noqa: E402

COS = _native.METRIC_COSINE
K = 100
# cdna_hip_programming.md "MFMA rate per dtype": i8 = 2x the bf16 rate; MI355X_MICROARCH.md: bf16 ~2.5 PF dense
I8_PEAK_OPS = 5.0e15
I8_KERNELS = ("norms_i8", "gemm_i8_topk", "select_i8", "i8_finish", "widen_i8_f64", "h2d", "d2h")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def band_per_row(q, c, rows=4):
    """Entries with key >= f32(a_k - 2 eps) for a few query rows (host)."""
    ci = c.astype(np.int32)
    Sc = (ci.astype(np.int64) ** 2).sum(1)
    fc = (1.0 / np.sqrt(Sc.astype(np.float64))).astype(np.float32)
    out = []
    for i in range(rows):
        qi = q[i].astype(np.int32)
        dot = ci @ qi
        fq = np.float32(1.0 / np.sqrt(float((qi.astype(np.int64) ** 2).sum())))
        a = dot.astype(np.float32) * (fq * fc)
        a_k = np.partition(a, -K)[-K]
        out.append(int(np.count_nonzero(a >= np.float32(a_k - np.float32(2.0 ** -20)))))
    return out


def measure(m, n, d, reps):
    rs = np.random.RandomState(m + d)
    q8 = rs.randint(-128, 128, size=(m, d)).astype(np.int8)
    c8 = rs.randint(-128, 128, size=(n, d)).astype(np.int8)
    res = {"m": m, "n": n, "d": d, "k": K, "metric": "cosine"}
    hi8 = _native.DeviceCorpus.int8(c8)
    res["bytes_i8"] = hi8.nbytes
    q64 = q8.astype(np.float64)
    hf64 = _native.DeviceCorpus(c8.astype(np.float64))
    res["bytes_f64"] = hf64.nbytes
    q32 = q8.astype(np.float32)
    hbf = _native.DeviceCorpus(c8.astype(np.float32), compute="bf16")
    res["bytes_bf16"] = hbf.nbytes
    wall = {"i8": [], "f64": [], "bf16": []}
    kern = {name: [] for name in I8_KERNELS}
    got = want = None
    _native.timing_enable(True)
    for rep in range(reps + 1):
        _native.timing_reset()
        t8, got = timed(lambda: hi8.topk(q8, K, COS))
        ks = {name: _native.timing_read(name)[0] for name in I8_KERNELS}
        t64, want = timed(lambda: hf64.topk(q64, K, COS))
        tbf, _ = timed(lambda: hbf.topk(q32, K, COS))
        if rep:
            wall["i8"].append(t8)
            wall["f64"].append(t64)
            wall["bf16"].append(tbf)
            for name in I8_KERNELS:
                kern[name].append(ks[name])
    _native.timing_enable(False)
    res["bit_equal_to_f64_handle"] = bool(np.array_equal(got[0], want[0])
                                          and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)))
    res["wall_ms"] = {k: spread(v) for k, v in wall.items()}
    res["i8_kernel_ms"] = {k: spread(v) for k, v in kern.items()}
    dp = -(-d // 64) * 64
    gemm = res["i8_kernel_ms"]["gemm_i8_topk"]["median"]
    res["gemm_i8_fraction_of_peak"] = 2.0 * m * n * dp / (gemm * 1e-3) / I8_PEAK_OPS
    res["finish_share_of_call"] = res["i8_kernel_ms"]["i8_finish"]["median"] / res["wall_ms"]["i8"]["median"]
    res["ratio_f64_over_i8"] = res["wall_ms"]["f64"]["median"] / res["wall_ms"]["i8"]["median"]
    res["ratio_bf16_over_i8"] = res["wall_ms"]["bf16"]["median"] / res["wall_ms"]["i8"]["median"]
    res["bytes_f64_over_i8"] = res["bytes_f64"] / res["bytes_i8"]
    res["band_candidates_per_row"] = band_per_row(q8, c8)
    for h in (hi8, hf64, hbf):
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8", "measure.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="4096x256,1000x768")
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    out = {"peak_ops_assumed": I8_PEAK_OPS, "shapes": []}
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
