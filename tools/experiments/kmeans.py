"""Measurements of k-means on a resident handle (profiles/kmeans/README.md).

  python tools/experiments/kmeans.py [--out-dir DIR] [--reps N] [--baseline-reps N]

One process, one shape: n = 1M rows of d = 768 drawn around 1024 planted
centres, K = 1024, euclidean, 10 updates from the same seeded ``init``, on a
resident f32 handle.  Per round, alternating: ``DeviceCorpus.kmeans`` and the
baseline -- what the commit before this entry offers: the top-1 of the rows
(uploaded as queries every iteration) on a ``DeviceCorpus`` of the centroids
for the labels, and a NumPy update on the host: a stable sort of the labels, then an
f64 ``np.add.reduceat`` over the sorted rows, the columns split over 16
threads.  Kernel times are the library's stream events (pmm_timing_read); wall
times are host clocks around calls that end in a synchronise.  The first
round warms up and is dropped; figures are medians with the minimum and maximum.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))

from polars_matmul import _native  # noqa: E402

ASSIGN = ("norms_f32", "gemm_f32_seed", "seed_select", "gemm_f32_topk", "merge_topk")
ORDER = ("kmeans_labels", "kmeans_order")
UPDATE = ("kmeans_update", "kmeans_finish")
STREAM_TBS = 5.28  # round_norms_bf16's rate in this project's profiles (DESIGN.md §4d "Bit rows")
THREADS = 16


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def host_update(x, labels, c, pool):
    """The parent's means: the clusters' f64 means by a stable sort and reduceat, 16 threads over the columns."""
    order = np.argsort(labels, kind="stable")
    sl = labels[order]
    keep = sl != _native.NO_GROUP
    order, sl = order[keep], sl[keep]
    starts = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
    ids, counts = sl[starts], np.diff(np.r_[starts, sl.size])
    out = c.copy()
    edges = np.linspace(0, x.shape[1], THREADS + 1).astype(int)

    def part(t):
        j = slice(edges[t], edges[t + 1])
        s = np.add.reduceat(x[:, j][order].astype(np.float64), starts, axis=0)
        out[ids, j] = (s / counts[:, None]).astype(np.float32)

    list(pool.map(part, [t for t in range(THREADS) if edges[t + 1] > edges[t]]))
    return out


def baseline(x, init, max_iter, pool):
    c, updates, prev = init.copy(), 0, None
    while True:
        idx, _ = dc_c(c).topk(x, 1, _native.METRIC_EUCLIDEAN)
        labels = idx[:, 0]
        if updates > 0 and np.array_equal(labels, prev):
            return c, labels, updates, True
        if updates == max_iter:
            return c, labels, updates, False
        c = host_update(x, labels, c, pool)
        prev = labels
        updates += 1


_centroid_handles = []


def dc_c(c):
    """A handle of the current centroids (the corpus side of the parent's top-1); the previous one is freed."""
    while _centroid_handles:
        _centroid_handles.pop().close()
    h = _native.DeviceCorpus(np.ascontiguousarray(c))
    _centroid_handles.append(h)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "kmeans"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-reps", type=int, default=1)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("kmeans: no HIP device visible")
    n, d, K, iters = args.n, args.d, args.k, args.iters
    rng = np.random.default_rng(42)
    mu = rng.standard_normal((K, d), dtype=np.float32)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= np.float32(3.0)
    x += mu[rng.integers(0, K, size=n)]
    init = np.ascontiguousarray(x[np.sort(np.random.RandomState(0).choice(n, K, replace=False))])
    dp = (d + 31) // 32 * 32
    dc = _native.DeviceCorpus(x)
    pool = ThreadPoolExecutor(THREADS)
    names = ASSIGN + ORDER + UPDATE + ("h2d", "d2h")
    rounds, base_rounds, final, base_final = [], [], None, None
    try:
        for r in range(args.reps + 1):
            _native.timing_enable(True)
            _native.timing_reset()
            t = time.perf_counter()
            final = dc.kmeans(init, _native.METRIC_EUCLIDEAN, iters)
            wall = (time.perf_counter() - t) * 1e3
            rec = {name: _native.timing_read(name) for name in names}
            _native.timing_reset()
            _native.timing_enable(False)
            if r > 0:
                rounds.append({"wall_ms": wall, "updates": final[3], "converged": final[4],
                               "kernels": {k: {"ms": v[0], "launches": v[1]} for k, v in rec.items()}})
            if 0 < r <= args.baseline_reps:
                t = time.perf_counter()
                base_final = baseline(x, init, iters, pool)
                base_rounds.append((time.perf_counter() - t) * 1e3)
    finally:
        while _centroid_handles:
            _centroid_handles.pop().close()
        dc.close()
        pool.shutdown()

    def per(names_, rd, launches_of):
        return sum(rd["kernels"][k]["ms"] for k in names_) / max(1, rd["kernels"][launches_of]["launches"])

    upd_ms = [rd["kernels"]["kmeans_update"]["ms"] / rd["kernels"]["kmeans_update"]["launches"] for rd in rounds]
    tbs = [n * dp * 4 / (ms * 1e-3) / 1e12 for ms in upd_ms]
    out = {
        "shape": {"n": n, "d": d, "K": K, "metric": "euclidean", "max_iter": iters},
        "kmeans": {
            "wall_ms": spread([rd["wall_ms"] for rd in rounds]),
            "updates": rounds[-1]["updates"], "converged": rounds[-1]["converged"],
            "assign_ms_per_iteration": spread([per(ASSIGN, rd, "gemm_f32_topk") for rd in rounds]),
            "ordering_ms_per_iteration": spread([per(ORDER, rd, "kmeans_order") for rd in rounds]),
            "update_ms_per_iteration": spread([per(UPDATE, rd, "kmeans_update") for rd in rounds]),
            "update_kernel_ms": spread(upd_ms),
            "update_kernel_TBps": spread(tbs),
            "update_kernel_fraction_of_stream_rate": statistics.median(tbs) / STREAM_TBS,
            "stream_rate_TBps": STREAM_TBS,
        },
        "rounds": rounds,
    }
    if base_rounds:
        out["baseline"] = {"wall_ms": spread(base_rounds), "updates": base_final[2], "converged": base_final[3],
                           "threads": THREADS}
        out["ratio_baseline_over_kmeans"] = statistics.median(base_rounds) / out["kmeans"]["wall_ms"]["median"]
        out["final_labels_equal"] = bool(np.array_equal(final[1], base_final[1]))
        out["final_labels_differing"] = int(np.count_nonzero(final[1] != base_final[1]))
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "measure.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}, indent=1))


if __name__ == "__main__":
    main()
