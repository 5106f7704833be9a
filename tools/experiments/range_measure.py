"""Measurements of range search (profiles/range/README.md).

  python tools/experiments/range_measure.py [--out FILE] [--reps N] [--parent-lib libpmm.so]

One process, one shape: 8192 queries x 1M corpus rows x 768, f32 cosine, on a
resident handle, the 256 x 256 tile variant forced for every call.  Two
thresholds are taken from a sample of the score distribution (256 queries x
65536 corpus rows on the host) so that a query row has about 10 and about 1000
hits.  Per round, alternating: the range call at each threshold and the fused
f32 top-k at k = 100 (unscreened, so that the f32 kernel runs) -- the latter
through ``--parent-lib`` when given (the library of the commit before range
search, loaded beside the product's), else through the product library, whose
top-k instantiations are the same code.  Kernel times are the library's stream
events (pmm_timing_read); wall times are host clocks around calls that end in
a synchronise.  The first round warms up and is dropped; figures are medians
with the minimum and maximum.
"""
from __future__ import annotations

import argparse
import ctypes
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
RANGE_KERNELS = ("gemm_f32_range", "range_bin", "range_sort_wave", "range_sort_block", "range_decode", "norms_f32",
                 "h2d", "d2h")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


class ParentLib:
    """The entries the comparison needs of another build of the library."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.pmm_corpus_create_f32.argtypes = [vp, i64, i64, ctypes.POINTER(vp)]
        L.pmm_topk_f32_corpus.argtypes = [vp, vp, i64, i64, i32, vp, vp]
        L.pmm_corpus_destroy.argtypes = [vp]
        L.pmm_timing_enable.argtypes = [i32]
        L.pmm_timing_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)]
        L.pmm_last_error.restype = ctypes.c_char_p
        self.L, self.h = L, vp()
        self.has_range = hasattr(L, "pmm_range_f32_corpus")

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.L.pmm_last_error().decode())

    def create(self, c):
        self.ok(self.L.pmm_corpus_create_f32(_native.ptr(c), c.shape[0], c.shape[1], ctypes.byref(self.h)))
        self.ok(self.L.pmm_timing_enable(1))

    def topk(self, q, k):
        idx = np.empty((q.shape[0], k), np.uint32)
        sc = np.empty((q.shape[0], k), np.float32)
        self.ok(self.L.pmm_timing_reset())
        t = time.perf_counter()
        self.ok(self.L.pmm_topk_f32_corpus(self.h, _native.ptr(q), q.shape[0], k, COS, _native.ptr(idx), _native.ptr(sc)))
        wall = (time.perf_counter() - t) * 1e3
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        self.ok(self.L.pmm_timing_read(b"gemm_f32_topk", ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, wall, idx, sc

    def close(self):
        self.L.pmm_corpus_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range", "measure.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    args = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("range_measure: no HIP device visible")
    m, n, d = args.m, args.n, args.d
    c = np.random.default_rng(42).standard_normal((n, d), dtype=np.float32)
    q = np.random.default_rng(43).standard_normal((m, d), dtype=np.float32)

    # thresholds from a sample of the score distribution
    sq, sc_ = q[:256].astype(np.float64), c[:min(n, 65536)].astype(np.float64)
    s = (sq @ sc_.T) / np.outer(np.linalg.norm(sq, axis=1), np.linalg.norm(sc_, axis=1))
    s = np.sort(s.reshape(-1))
    thr = {str(h): float(s[-max(1, int(round(h / n * s.size)))]) for h in (10, 1000)}

    os.environ["PMM_GEMM_VARIANT"] = "3"
    os.environ["PMM_F32_SCREEN"] = "0"
    dc = _native.DeviceCorpus(c)
    parent = ParentLib(args.parent_lib) if args.parent_lib else None
    if parent:
        parent.create(c)
    _native.timing_enable(True)
    rounds = {h: {"wall_ms": [], "total": 0, **{k: [] for k in RANGE_KERNELS}} for h in thr}
    topk_ms, topk_wall = [], []
    res = {}
    for i in range(args.reps + 1):
        for h, t in thr.items():
            _native.timing_reset()
            t0 = time.perf_counter()
            res[h] = dc.range(q, t, COS, cap=2000 * m)  # (room for both thresholds: one pass)
            wall = (time.perf_counter() - t0) * 1e3
            got = {k: _native.timing_read(k)[0] for k in RANGE_KERNELS}
            if i:
                rounds[h]["wall_ms"].append(wall)
                for k in RANGE_KERNELS:
                    rounds[h][k].append(got[k])
            rounds[h]["total"] = int(res[h][0][-1])
        if parent:
            ms, wall, ti, ts = parent.topk(q, 100)
        else:
            _native.timing_reset()
            t0 = time.perf_counter()
            ti, ts = dc.topk(q, 100, COS)
            wall = (time.perf_counter() - t0) * 1e3
            ms = _native.timing_read("gemm_f32_topk")[0]
        if i:
            topk_ms.append(ms), topk_wall.append(wall)
    _native.timing_reset()
    _native.timing_enable(False)

    # the lists against the top-k lists: a row with at most 100 hits is a prefix of its top-100
    o, gi, gs = res["10"]
    cnt = np.diff(o)
    rows = np.flatnonzero(cnt <= 100)
    prefix_ok = all(np.array_equal(gi[o[r]:o[r + 1]], ti[r, :cnt[r]]) and
                    np.array_equal(gs[o[r]:o[r + 1]].view(np.uint32), ts[r, :cnt[r]].view(np.uint32)) for r in rows)
    out = {
        "shape": {"m": m, "n": n, "d": d, "metric": "cosine", "variant": 3},
        "thresholds": thr,
        "topk_k100": {"library": "parent" if parent else "product", "gemm_f32_topk_ms": spread(topk_ms),
                      "wall_ms": spread(topk_wall)},
        "range": {},
        "range_10_lists_are_prefixes_of_topk_lists": {"rows_checked": int(rows.size), "ok": bool(prefix_ok)},
    }
    for h in thr:
        r = rounds[h]
        tot = r["total"]
        emit = statistics.median(r["gemm_f32_range"])
        out["range"][h] = {
            "threshold": thr[h], "total_hits": tot, "mean_hits_per_row": tot / m,
            "kernels_ms": {k: spread(r[k]) for k in RANGE_KERNELS}, "wall_ms": spread(r["wall_ms"]),
            "emit_over_topk_kernel": emit / statistics.median(topk_ms),
            "emit_TFLOPs": 2.0 * m * n * d / (emit * 1e-3) / 1e12,
            # records: 12 B each out of the emit pass; bin reads them and writes
            # the 8 B keys; sort and decode read and write 8 B each; 8 B each leave
            "record_bytes": {"emit_written": 12 * tot, "bin_read_plus_written": 20 * tot,
                             "sort_read_plus_written": 16 * tot, "decode_read_plus_written": 16 * tot,
                             "d2h": 8 * tot},
        }
    out["goal_emit_at_10_hits_within_1.05x_of_topk_kernel"] = bool(out["range"]["10"]["emit_over_topk_kernel"] <= 1.05)
    dc.close()
    if parent:
        parent.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
