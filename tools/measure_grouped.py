#!/usr/bin/env python3
"""Grouped search against what the parent commit offers (one derived handle and
one top-k call per label), and the crossover between the grouped kernel and
the per-pair loop.  Writes one JSON document to stdout (profiles/grouped/).

    python tools/measure_grouped.py --baseline-lib /path/to/parent/libpmm.so > profiles/grouped/measure.json

Workload: n x d f32 corpus, `labels` labels of about n / labels rows, `qper`
queries per label, k = 10, cosine.  The baseline library (the parent commit's
build, loaded beside this tree's through ctypes) is alternated with the new
call in one process, `rounds` times; medians are reported.  Without
--baseline-lib the baseline runs on this tree's library (the subset entries
are unchanged by grouped search).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))
from polars_matmul import _native  # noqa: E402

COS = _native.METRIC_COSINE
VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


class Baseline:
    """The subset entries of a libpmm.so loaded by path."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.pmm_corpus_create_f32.argtypes = [VP, I64, I64, ctypes.POINTER(VP)]
        self.lib.pmm_corpus_subset_ids.argtypes = [VP, VP, I64, ctypes.POINTER(VP)]
        self.lib.pmm_topk_f32_corpus.argtypes = [VP, VP, I64, I64, I32, VP, VP]
        self.lib.pmm_corpus_destroy.argtypes = [VP]

    def create(self, c):
        h = VP()
        assert self.lib.pmm_corpus_create_f32(_native.ptr(c), c.shape[0], c.shape[1], ctypes.byref(h)) == 0
        return h

    def subset(self, h, ids):
        s = VP()
        assert self.lib.pmm_corpus_subset_ids(h, _native.ptr(ids), ids.size, ctypes.byref(s)) == 0
        return s

    def topk(self, h, q, k, idx, sc):
        assert self.lib.pmm_topk_f32_corpus(h, _native.ptr(q), q.shape[0], k, COS, _native.ptr(idx), _native.ptr(sc)) == 0

    def destroy(self, h):
        self.lib.pmm_corpus_destroy(h)


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=_native.LIB_PATH)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--labels", type=int, default=1000)
    ap.add_argument("--qper", type=int, default=10)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--crossover", type=int, default=1)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    c = np.random.default_rng(0).standard_normal((a.n, a.d), dtype=np.float32)
    cl = rs.randint(0, a.labels, size=a.n).astype(np.uint32)
    ql = np.repeat(np.arange(a.labels, dtype=np.uint32), a.qper)
    rs.shuffle(ql)
    q = rs.randn(ql.size, a.d).astype(np.float32)
    m, k = ql.size, a.k
    out = {"workload": vars(a), "device_count": _native.device_count()}

    base = Baseline(a.baseline_lib)
    ids = [np.flatnonzero(cl == g).astype(np.uint32) for g in range(a.labels)]
    rows = [np.flatnonzero(ql == g) for g in range(a.labels)]
    qs = [np.ascontiguousarray(q[r]) for r in rows]
    bi = [np.empty((r.size, k), np.uint32) for r in rows]
    bs = [np.empty((r.size, k), np.float32) for r in rows]
    bh = base.create(c)
    subs = [base.subset(bh, i) for i in ids]

    dc = _native.DeviceCorpus(c)
    part = dc.partition(cl, a.labels)

    def baseline_search():
        for g in range(a.labels):
            base.topk(subs[g], qs[g], k, bi[g], bs[g])

    def baseline_with_derivation():
        for g in range(a.labels):
            s = base.subset(bh, ids[g])
            base.topk(s, qs[g], k, bi[g], bs[g])
            base.destroy(s)

    got = [None]

    def grouped():
        got[0] = part.topk_grouped(q, ql, k, COS)

    for fn in (baseline_search, grouped):  # warm-up: arenas, kernels loaded
        fn()
    t_base, t_der, t_new = [], [], []
    for _ in range(a.rounds):  # alternating rounds
        t_base.append(timed(baseline_search))
        t_new.append(timed(grouped))
        t_der.append(timed(baseline_with_derivation))
    gi, gs, gl = got[0]
    same = all(np.array_equal(gi[rows[g]], bi[g]) and np.array_equal(gs[rows[g]].view(np.uint32), bs[g].view(np.uint32))
               for g in range(a.labels))
    out["equal_to_baseline"] = bool(same and np.all(gl == k))
    med = statistics.median
    out["ms"] = {"baseline_search_only": med(t_base), "baseline_with_derivations": med(t_der), "grouped": med(t_new),
                 "rounds": {"baseline_search_only": t_base, "baseline_with_derivations": t_der, "grouped": t_new}}
    print(f"medians ms: {out['ms']['baseline_search_only']:.2f} search-only, {out['ms']['baseline_with_derivations']:.2f} "
          f"with derivations, {out['ms']['grouped']:.2f} grouped; equal {out['equal_to_baseline']}", file=sys.stderr,
          flush=True)
    out["ratio_search_only_over_grouped"] = med(t_base) / med(t_new)
    out["ratio_with_derivations_over_grouped"] = med(t_der) / med(t_new)

    # the kernel's own time by HIP events against its floors
    _native.timing_enable(True)
    ker = []
    for _ in range(a.rounds):
        _native.timing_reset()
        grouped()
        ker.append(_native.timing_read("grouped_topk_f32")[0])
    _native.timing_enable(False)
    sizes = np.bincount(cl, minlength=a.labels).astype(np.int64)
    mq = np.bincount(ql, minlength=a.labels).astype(np.int64)
    units = -(-mq // 16)
    dp = -(-a.d // 32) * 32
    bytes_read = float((units * sizes).sum()) * dp * 4
    flops = 2.0 * float((mq * sizes).sum()) * a.d
    out["kernel"] = {"ms": med(ker), "rounds": ker, "segment_bytes_read": bytes_read,
                     "hbm_floor_ms": bytes_read / 8e12 * 1e3, "flops": flops, "mfma_floor_ms": flops / 157.3e12 * 1e3}
    for h in subs:
        base.destroy(h)
    base.destroy(bh)
    part.close()
    dc.close()

    # crossover: groups of 256 .. 64k rows at 16 queries per group, both paths forced
    if a.crossover:
        out["crossover"] = []
        for seg in (256, 1024, 4096, 16384, 65536):
            groups = max(1, min(64, (1 << 20) // seg))
            n2 = groups * seg
            c2 = np.random.default_rng(seg).standard_normal((n2, a.d), dtype=np.float32)
            cl2 = np.repeat(np.arange(groups, dtype=np.uint32), seg)
            ql2 = np.repeat(np.arange(groups, dtype=np.uint32), 16)
            q2 = rs.randn(ql2.size, a.d).astype(np.float32)
            d2 = _native.DeviceCorpus(c2)
            p2 = d2.partition(cl2, groups)
            row = {"segment_rows": seg, "groups": groups, "queries_per_group": 16}
            res = {}
            for path in ("kernel", "loop"):
                os.environ["PMM_GROUPED"] = path
                p2.topk_grouped(q2, ql2, k, COS)
                ts = []
                for _ in range(a.rounds):
                    ts.append(timed(lambda: res.__setitem__(path, p2.topk_grouped(q2, ql2, k, COS))))
                row[path + "_ms"] = med(ts)
            os.environ.pop("PMM_GROUPED", None)
            row["equal"] = bool(np.array_equal(res["kernel"][0], res["loop"][0])
                                and np.array_equal(res["kernel"][1].view(np.uint32), res["loop"][1].view(np.uint32)))
            out["crossover"].append(row)
            print(f"crossover {row}", file=sys.stderr, flush=True)
            p2.close()
            d2.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
