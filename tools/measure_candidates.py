#!/usr/bin/env python3
"""Candidate search against what the parent commit offers for per-row lists:
(a) one derived handle and one top-k call per query row, (b) the full-corpus
top-k at the same m.  Writes one JSON document to stdout (profiles/candidates/).

    python tools/measure_candidates.py --baseline-lib /path/to/parent/libpmm.so > profiles/candidates/measure.json

Workload: m queries x (n x d f32 corpus), `cands` random candidates per row,
k = 100, cosine.  The baseline library (the parent commit's build, loaded
beside this tree's through ctypes) is alternated with the new call in one
process, `rounds` times; medians are reported.  Baseline (a) runs over a
`sample` of the rows and is scaled by m / sample.  Without --baseline-lib the
baselines run on this tree's library (its subset and top-k entries are
unchanged by candidate search).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from polars_matmul import _native  # noqa: E402
from measure_grouped import Baseline, timed  # noqa: E402

COS = _native.METRIC_COSINE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=_native.LIB_PATH)
    ap.add_argument("--m", type=int, default=10_000)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--full-rounds", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    c = rng.standard_normal((a.n, a.d), dtype=np.float32)
    q = rng.standard_normal((a.m, a.d), dtype=np.float32)
    # `cands` distinct random rows per list, ascending: one uniformly random row from each of `cands` equal strata
    w = a.n // a.cands
    ids = (np.arange(a.cands, dtype=np.int64)[None, :] * w + rng.integers(0, w, size=(a.m, a.cands))).astype(np.uint32)
    offsets = np.arange(a.m + 1, dtype=np.int64) * a.cands
    m, k = a.m, min(a.k, a.cands)
    out = {"workload": vars(a), "device_count": _native.device_count()}

    base = Baseline(a.baseline_lib)
    bh = base.create(c)
    dc = _native.DeviceCorpus(c)
    sample = np.arange(0, m, max(1, m // a.sample))[:a.sample]
    qs = [np.ascontiguousarray(q[i:i + 1]) for i in sample]
    bi = np.empty((sample.size, k), np.uint32)
    bs = np.empty((sample.size, k), np.float32)
    fi = np.empty((m, k), np.uint32)
    fs = np.empty((m, k), np.float32)

    def per_row():  # (a): what a user of the parent commit does for per-row lists
        for j, i in enumerate(sample):
            s = base.subset(bh, np.ascontiguousarray(ids[i]))
            base.topk(s, qs[j], k, bi[j:j + 1], bs[j:j + 1])
            base.destroy(s)

    def full():  # (b): the whole corpus at the same m
        base.topk(bh, q, k, fi, fs)

    got = [None]

    def candidates():
        got[0] = dc.topk_candidates(q, offsets, ids.reshape(-1), k, COS)

    for fn in (per_row, candidates, full):  # warm-up: arenas, kernels loaded
        fn()
    t_row, t_new, t_full = [], [], []
    for r in range(a.rounds):  # alternating rounds
        t_row.append(timed(per_row))
        t_new.append(timed(candidates))
        if r < a.full_rounds:
            t_full.append(timed(full))
    gi, gs, gl = got[0]
    out["equal_to_per_row_baseline"] = bool(np.array_equal(gi[sample], bi) and (gl == k).all()
                                            and np.array_equal(gs[sample].view(np.uint32), bs.view(np.uint32)))
    med = statistics.median
    scale = m / sample.size
    out["ms"] = {"per_row_sample": med(t_row), "per_row_sample_rows": int(sample.size), "per_row_scaled": med(t_row) * scale,
                 "per_row_each": med(t_row) / sample.size, "full_corpus": med(t_full), "candidates": med(t_new),
                 "rounds": {"per_row_sample": t_row, "full_corpus": t_full, "candidates": t_new}}
    out["ratio_per_row_over_candidates"] = med(t_row) * scale / med(t_new)
    out["ratio_full_over_candidates"] = med(t_full) / med(t_new)

    # the passes' own times by HIP events; the score pass as gathered bytes per second
    _native.timing_enable(True)
    names = ("cand_score", "range_sort_wave", "range_sort_block", "cand_merge", "cand_decode", "h2d", "d2h", "norms_f32")
    ker = {nm: [] for nm in names}
    for _ in range(a.rounds):
        _native.timing_reset()
        candidates()
        for nm in names:
            ker[nm].append(_native.timing_read(nm)[0])
    _native.timing_enable(False)
    dp = -(-a.d // 32) * 32
    gathered = float(m) * a.cands * dp * 4
    score_ms = med(ker["cand_score"])
    out["passes_ms"] = {nm: med(v) for nm, v in ker.items()}
    out["score_pass"] = {"ms": score_ms, "rounds": ker["cand_score"], "gathered_bytes": gathered,
                         "tb_per_s": gathered / (score_ms * 1e-3) / 1e12,
                         "fraction_of_gathered_row_rate_5p5": gathered / (score_ms * 1e-3) / 5.5e12,
                         "fraction_of_subset_gather_2p74": gathered / (score_ms * 1e-3) / 2.74e12}
    print(f"medians ms: per-row {out['ms']['per_row_scaled']:.1f} (scaled from {sample.size} rows), full corpus "
          f"{out['ms']['full_corpus']:.1f}, candidates {out['ms']['candidates']:.2f}; score pass {score_ms:.3f} ms = "
          f"{out['score_pass']['tb_per_s']:.2f} TB/s; equal {out['equal_to_per_row_baseline']}", file=sys.stderr, flush=True)
    base.destroy(bh)
    dc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
