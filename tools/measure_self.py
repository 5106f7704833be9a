#!/usr/bin/env python3
"""Self search against what the parent commit offers for one column searched
against itself: ``range(q = c)`` filtered to index > row, and ``topk(q = c,
k + 1)``.  Writes one JSON document to stdout (profiles/self/).

    python tools/measure_self.py --baseline-lib /path/to/parent/libpmm.so > profiles/self/measure.json

Workload: n x d f32 rows, cosine; a threshold that leaves about `hits` corpus
rows per query row in the full call (default: the Gaussian tail for random
rows); k = 100.  The baseline library (the parent commit's build, loaded beside
this tree's through ctypes) is alternated with the new calls in one process,
`rounds` times; medians are reported, with every round.  The emit passes' own
times come from each library's HIP-event timers (pmm_timing_read).  Without
--baseline-lib the baselines run on this tree's library (its range and top-k
entries are unchanged by self search).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from polars_matmul import _native  # noqa: E402
from measure_grouped import I32, I64, VP, Baseline, timed  # noqa: E402

COS = _native.METRIC_COSINE


class SelfBaseline(Baseline):
    """The parent's range entry and timers beside its top-k."""

    def __init__(self, path):
        super().__init__(path)
        self.lib.pmm_range_f32_corpus.argtypes = [VP, VP, I64, ctypes.c_float, I32, I64, VP, VP, VP,
                                                  ctypes.POINTER(ctypes.c_int64)]
        self.lib.pmm_timing_enable.argtypes = [I32]
        self.lib.pmm_timing_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_int64)]

    def range(self, h, q, t, cap, offsets, idx, sc):
        total = ctypes.c_int64(0)
        assert self.lib.pmm_range_f32_corpus(h, _native.ptr(q), q.shape[0], t, COS, cap, _native.ptr(offsets),
                                             _native.ptr(idx), _native.ptr(sc), ctypes.byref(total)) == 0
        return total.value

    def kernel_ms(self, name):
        ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
        assert self.lib.pmm_timing_read(name.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0
        return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=_native.LIB_PATH)
    ap.add_argument("--n", type=int, default=262_144)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--hits", type=float, default=10.0)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n, d, k = a.n, a.d, a.k
    c = rng.standard_normal((n, d), dtype=np.float32)
    if a.threshold is None:
        # cosine of random rows ~ N(0, 1/d): the tail that leaves `hits` of n rows
        from statistics import NormalDist

        a.threshold = NormalDist().inv_cdf(1.0 - a.hits / n) / np.sqrt(d)
    t = float(np.float32(a.threshold))
    out = {"workload": vars(a), "device_count": _native.device_count()}

    base = SelfBaseline(a.baseline_lib)
    bh = base.create(c)
    dc = _native.DeviceCorpus(c)
    cus = 256
    v, visits, full = _native.range_self_plan(n, cus)
    out["plan"] = {"variant": v, "block_tile_visits": visits, "block_tile_full": full, "visit_ratio": visits / full}

    cap = max(1 << 16, 64 * n)
    bo = np.empty(n + 1, np.int64)
    bi, bs = np.empty(cap, np.uint32), np.empty(cap, np.float32)
    ti, ts = np.empty((n, k + 1), np.uint32), np.empty((n, k + 1), np.float32)
    # (the new entries through the C ABI into buffers allocated once, as the
    # baseline's: a fresh numpy array per call would add its page faults)
    so = np.empty(n + 1, np.int64)
    si, ss = np.empty(cap, np.uint32), np.empty(cap, np.float32)
    gi, gs = np.empty((n, k), np.uint32), np.empty((n, k), np.float32)
    lib, ptr = _native.lib(), _native.ptr
    state = {}

    def base_range():
        state["base_total"] = base.range(bh, c, t, cap, bo, bi, bs)

    def self_range():
        total = ctypes.c_int64(0)
        _native.check(lib.pmm_range_f32_self(dc._h, t, COS, cap, ptr(so), ptr(si), ptr(ss), ctypes.byref(total)))
        state["self_total"] = total.value

    def base_topk():
        base.topk(bh, c, k + 1, ti, ts)

    def self_topk():
        _native.check(lib.pmm_topk_f32_self(dc._h, k, COS, ptr(gi), ptr(gs)))

    for fn in (base_range, self_range, base_topk, self_topk):  # warm-up: arenas, kernels loaded
        fn()
    assert state["base_total"] <= cap and state["self_total"] <= cap
    base.lib.pmm_timing_enable(1)
    _native.timing_enable(True)
    ms = {nm: [] for nm in ("base_range", "self_range", "base_topk", "self_topk", "base_emit", "self_emit", "drop_self")}
    for _ in range(a.rounds):  # alternating rounds
        base.lib.pmm_timing_reset()
        _native.timing_reset()
        ms["base_range"].append(timed(base_range))
        ms["self_range"].append(timed(self_range))
        ms["base_emit"].append(base.kernel_ms("gemm_f32_range"))
        ms["self_emit"].append(_native.timing_read("gemm_f32_self")[0])
        ms["base_topk"].append(timed(base_topk))
        ms["self_topk"].append(timed(self_topk))
        ms["drop_self"].append(_native.timing_read("drop_self")[0])
    base.lib.pmm_timing_enable(0)
    _native.timing_enable(False)
    med = statistics.median
    out["ms"] = {nm: med(v) for nm, v in ms.items()}
    out["rounds_ms"] = ms
    out["ratio"] = {"emit_self_over_base": med(ms["self_emit"]) / med(ms["base_emit"]),
                    "range_self_over_base": med(ms["self_range"]) / med(ms["base_range"]),
                    "topk_self_over_base": med(ms["self_topk"]) / med(ms["base_topk"])}
    out["bytes_not_uploaded"] = int(n) * d * 4
    out["hits"] = {"baseline_total": int(state["base_total"]), "self_total": int(so[-1]),
                   "baseline_per_row": state["base_total"] / n}

    # the lists of a sample of rows against the filtered baseline, bit for bit
    sample = np.arange(0, n, max(1, n // a.sample))[:a.sample]
    ok_range = ok_topk = True
    for i in sample:
        ri, rs = bi[bo[i]:bo[i + 1]], bs[bo[i]:bo[i + 1]]
        keep = ri > i
        ok_range &= bool(np.array_equal(si[so[i]:so[i + 1]], ri[keep])
                         and np.array_equal(ss[so[i]:so[i + 1]].view(np.uint32), rs[keep].view(np.uint32)))
        other = ti[i] != i
        if other.all():
            other[-1] = False
        ok_topk &= bool(np.array_equal(gi[i], ti[i][other]) and np.array_equal(gs[i].view(np.uint32),
                                                                              ts[i][other].view(np.uint32)))
    out["equal_on_sample"] = {"rows": int(sample.size), "range": ok_range, "topk": ok_topk}
    print(f"medians ms: range {out['ms']['base_range']:.1f} -> {out['ms']['self_range']:.1f} (emit "
          f"{out['ms']['base_emit']:.1f} -> {out['ms']['self_emit']:.1f}, visit ratio {visits / full:.4f}); top-k "
          f"{out['ms']['base_topk']:.1f} -> {out['ms']['self_topk']:.1f}; equal {out['equal_on_sample']}",
          file=sys.stderr, flush=True)
    base.destroy(bh)
    dc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
