#!/usr/bin/env python3
"""Probed search against the two ways the parent commit offers several probes,
and its recall against the exhaustive search.  Writes one JSON document to
stdout (profiles/probed/).

    python tools/measure_probed.py --baseline-lib /path/to/parent/libpmm.so > profiles/probed/measure.json

Workload (the grouped profile's): an n x d f32 corpus in `labels` clusters of
about n / labels rows (a centre plus noise per row; the generating cluster is
the row's label), m queries drawn the same way, k = 10, cosine; every query
probes the nprobe clusters whose centres score highest (one top-k call on the
centres, not timed).  Baselines, on the baseline library (the parent commit's
build, loaded beside this tree's through ctypes; without --baseline-lib this
tree's, whose grouped and candidate entries are unchanged):

  1. nprobe calls of pmm_topk_f32_grouped plus a NumPy merge by (score, row);
  2. pmm_topk_f32_candidates with every probed group expanded into row ids
     (the expansion itself is not timed).

Both are asserted bit-equal to the probed call before anything is timed; the
three calls alternate in one process, `rounds` times, and medians are reported.
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
ptr = _native.ptr


class Baseline:
    """The grouped and candidate entries of a libpmm.so loaded by path."""

    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        lib.pmm_corpus_create_f32.argtypes = [VP, I64, I64, ctypes.POINTER(VP)]
        lib.pmm_corpus_partition.argtypes = [VP, VP, I64, ctypes.POINTER(VP)]
        lib.pmm_topk_f32_grouped.argtypes = [VP, VP, I64, VP, I64, I32, VP, VP, VP]
        lib.pmm_topk_f32_candidates.argtypes = [VP, VP, I64, VP, VP, I64, I32, VP, VP, VP]
        lib.pmm_corpus_destroy.argtypes = [VP]

    def create(self, c):
        h = VP()
        assert self.lib.pmm_corpus_create_f32(ptr(c), c.shape[0], c.shape[1], ctypes.byref(h)) == 0
        return h

    def partition(self, h, labels, G):
        p = VP()
        assert self.lib.pmm_corpus_partition(h, ptr(labels), G, ctypes.byref(p)) == 0
        return p

    def grouped(self, p, q, ql, k, idx, sc, lens):
        assert self.lib.pmm_topk_f32_grouped(p, ptr(q), q.shape[0], ptr(ql), k, COS, ptr(idx), ptr(sc), ptr(lens)) == 0

    def candidates(self, h, q, off, ids, k, idx, sc, lens):
        assert self.lib.pmm_topk_f32_candidates(h, ptr(q), q.shape[0], ptr(off), ptr(ids), k, COS, ptr(idx), ptr(sc),
                                                ptr(lens)) == 0


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def merge_lists(idx, sc, k):
    """Per row the best k of P lists (idx, sc: (P, m, k)), best score first, ties to the lower row."""
    P, m, _ = idx.shape
    ai = idx.transpose(1, 0, 2).reshape(m, P * k)
    as_ = sc.transpose(1, 0, 2).reshape(m, P * k)
    rows = np.repeat(np.arange(m), P * k)
    order = np.lexsort((ai.reshape(-1), -as_.reshape(-1), rows)).reshape(m, P * k)[:, :k]
    flat_i, flat_s = ai.reshape(-1), as_.reshape(-1)
    return flat_i[order], flat_s[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=_native.LIB_PATH)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--labels", type=int, default=1024)
    ap.add_argument("--m", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--noise", type=float, default=1.0)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    G, k, m = a.labels, a.k, a.m
    centres = rng.standard_normal((G, a.d), dtype=np.float32)
    cl = rng.integers(0, G, size=a.n).astype(np.uint32)
    c = rng.standard_normal((a.n, a.d), dtype=np.float32)
    c *= np.float32(a.noise)
    c += centres[cl]
    q = rng.standard_normal((m, a.d), dtype=np.float32) * np.float32(a.noise) + centres[rng.integers(0, G, size=m)]
    q = np.ascontiguousarray(q, dtype=np.float32)
    out = {"workload": vars(a), "device_count": _native.device_count(), "nprobe": {}}

    base = Baseline(a.baseline_lib)
    bh = base.create(c)
    bp = base.partition(bh, cl, G)
    dc = _native.DeviceCorpus(c)
    part = dc.partition(cl, G)
    sizes = np.bincount(cl, minlength=G).astype(np.int64)
    group_rows = [np.flatnonzero(cl == g).astype(np.uint32) for g in range(G)]
    exact_i, _ = dc.topk(q, k, COS)
    ranked, _ = _native.topk_host(q, centres, max(a.nprobe), COS)  # the coarse quantiser: nearest centres first
    med = statistics.median
    dp = -(-a.d // 32) * 32

    for P in a.nprobe:
        probes = np.ascontiguousarray(ranked[:, :P], dtype=np.uint32)
        po = np.arange(m + 1, dtype=np.int64) * P
        pl = probes.reshape(-1)
        cols = [np.ascontiguousarray(probes[:, j]) for j in range(P)]
        gi, gs = np.empty((P, m, k), np.uint32), np.empty((P, m, k), np.float32)
        gl = np.empty(m, np.uint32)
        ids = [np.sort(np.concatenate([group_rows[g] for g in probes[i]])) for i in range(m)]
        coff = np.concatenate([[0], np.cumsum([x.size for x in ids])]).astype(np.int64)
        cids = np.concatenate(ids)
        del ids
        ci, cs, clen = np.empty((m, k), np.uint32), np.empty((m, k), np.float32), np.empty(m, np.uint32)
        got, merged = [None], [None]

        def probed():
            got[0] = part.topk_probed(q, po, pl, k, COS)

        def grouped_calls():
            for j in range(P):
                base.grouped(bp, q, cols[j], k, gi[j], gs[j], gl)
            merged[0] = merge_lists(gi, gs, k)

        def candidates():
            base.candidates(bh, q, coff, cids, k, ci, cs, clen)

        for fn in (probed, grouped_calls, candidates):  # warm-up; and the lists, compared before any timing
            fn()
        pi, ps, plen = got[0]
        assert np.all(plen == k) and np.all(clen == k)
        eq1 = bool(np.array_equal(pi, merged[0][0]) and np.array_equal(ps.view(np.uint32), merged[0][1].view(np.uint32)))
        eq2 = bool(np.array_equal(pi, ci) and np.array_equal(ps.view(np.uint32), cs.view(np.uint32)))
        assert eq1 and eq2, (P, eq1, eq2)
        t_new, t_grp, t_cand = [], [], []
        for _ in range(a.rounds):  # alternating rounds
            t_grp.append(timed(grouped_calls))
            t_new.append(timed(probed))
            t_cand.append(timed(candidates))
        _native.timing_enable(True)
        ker, mrg = [], []
        for _ in range(a.rounds):
            _native.timing_reset()
            probed()
            ker.append(_native.timing_read("probed_topk_f32")[0])
            mrg.append(_native.timing_read("probe_merge")[0])
        _native.timing_enable(False)
        slots = np.bincount(pl, minlength=G).astype(np.int64)
        bytes_read = float((-(-slots // 16) * sizes).sum()) * dp * 4
        recall = float(np.mean([np.intersect1d(pi[i], exact_i[i]).size for i in range(m)])) / k
        row = {"equal_to_grouped_calls": eq1, "equal_to_candidates": eq2,
               "ms": {"probed": med(t_new), "grouped_calls_and_merge": med(t_grp), "candidates": med(t_cand),
                      "rounds": {"probed": t_new, "grouped_calls_and_merge": t_grp, "candidates": t_cand}},
               "kernel": {"ms": med(ker), "segment_bytes_read": bytes_read,
                          "bytes_per_second": bytes_read / (med(ker) * 1e-3), "share_of_8e12": bytes_read / (med(ker) * 1e-3) / 8e12},
               "probe_merge": {"ms": med(mrg), "share_of_call": med(mrg) / med(t_new)},
               "candidate_ids": int(cids.size), "recall_at_k": recall}
        out["nprobe"][str(P)] = row
        print(f"nprobe {P}: probed {med(t_new):.2f} ms, grouped calls + merge {med(t_grp):.2f} ms, candidates "
              f"{med(t_cand):.2f} ms; kernel {med(ker):.2f} ms ({row['kernel']['share_of_8e12']:.2f} of 8 TB/s), merge "
              f"{med(mrg):.3f} ms; recall@{k} {recall:.4f}", file=sys.stderr, flush=True)
    part.close()
    dc.close()
    base.lib.pmm_corpus_destroy(bp)
    base.lib.pmm_corpus_destroy(bh)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
