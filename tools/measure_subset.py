"""Measurements of subset search on derived handles (profiles/subset/README.md).

  python tools/measure_subset.py [--out FILE] [--reps N]

One process; the variants of each comparison alternate round by round and the
figures are medians with the minimum and maximum (the first round warms up).

a. creation at a 1M x 768 f32 parent with a seeded half mask: the derived
   handle (wall clock, and its parts by the library's stream events: bitmap
   upload, compaction, row gather, image gather) against the only way without
   it -- DeviceCorpus(c[ids]) from host memory, the NumPy take included.
b. a 1000 x s x 768, k = 100 cosine search on the derived handle against the
   same search on the host-built handle of c[ids] (same kernels, same rows:
   equal lists after mapping, equal times within the run-to-run spread).
c. the remap launch at 1000 x 10000 x 256, k = 10 with every row selected,
   against the parent handle's call.
d. ``_topk(..., subset=mask)`` on its second call (a cache hit) against
   ``_topk`` on a pre-filtered corpus on its second call.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pyarrow as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))

from polars_matmul import _native  # noqa: E402
from polars_matmul import _polars_matmul as pm  # noqa: E402

COS = _native.METRIC_COSINE
PARTS = {"bitmap_upload": "h2d", "compaction_count_scan": "subset_mask_count", "compaction_write": "subset_mask_write",
         "row_gather": "subset_gather_rows", "image_gather": "subset_gather_image"}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def fixed(a):
    return pa.FixedSizeListArray.from_arrays(pa.array(a.reshape(-1)), a.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=6)
    args = ap.parse_args()
    out = {}
    n, d = 1_000_000, 768
    c = np.random.default_rng(42).standard_normal((n, d), dtype=np.float32)
    q = np.random.default_rng(43).standard_normal((1000, d), dtype=np.float32)
    mask = np.random.default_rng(44).random(n) < 0.5
    amask = pa.array(mask)
    ids = np.flatnonzero(mask).astype(np.uint32)
    s = int(ids.size)
    parent = _native.DeviceCorpus(c)

    # a. creation, first without and then with a parent image
    def creation(label):
        der, host = [], []
        parts = {k: [] for k in PARTS}
        _native.timing_enable(True)
        for i in range(args.reps + 1):
            _native.timing_reset()
            ms, sub = wall(lambda: parent.subset(amask))
            got = {k: _native.timing_read(v)[0] for k, v in PARTS.items()}
            has_image = sub.nbytes == _native.subset_device_bytes(s, d, screen=True)
            sub.close()
            _native.timing_reset()
            hm, h = wall(lambda: _native.DeviceCorpus(np.ascontiguousarray(c[ids])))
            h.close()
            if i:
                der.append(ms), host.append(hm)
                for k in PARTS:
                    parts[k].append(got[k])
        _native.timing_reset()
        _native.timing_enable(False)
        g = statistics.median(parts["row_gather"]) * 1e-3
        out["creation_" + label] = {
            "s": s, "derived_wall_ms": spread(der), "host_built_wall_ms": spread(host),
            "ratio_host_over_derived": statistics.median(host) / statistics.median(der),
            "parts_ms": {k: spread(v) for k, v in parts.items()}, "derived_has_image": bool(has_image),
            "row_gather_read_TBps": s * d * 4 / g / 1e12, "row_gather_read_plus_write_TBps": 2 * s * d * 4 / g / 1e12,
            "row_gather_read_fraction_of_8TBps": s * d * 4 / g / 8e12,
        }

    creation("parent_without_image")
    os.environ["PMM_F32_SCREEN"] = "1"
    parent.topk(q[:8], 10, COS)  # the parent builds its screen image
    del os.environ["PMM_F32_SCREEN"]
    creation("parent_with_image")

    # b. the search itself
    os.environ["PMM_F32_SCREEN"] = "0"  # (the same route on both handles, whatever images they hold)
    sub = parent.subset(amask)
    host = _native.DeviceCorpus(np.ascontiguousarray(c[ids]))
    ta, tb = [], []
    for i in range(args.reps + 2):
        a, _ = wall(lambda: sub.topk(q, 100, COS))
        b, _ = wall(lambda: host.topk(q, 100, COS))
        if i >= 2:
            ta.append(a), tb.append(b)
    gi, gs = sub.topk(q, 100, COS)
    hi, hs = host.topk(q, 100, COS)
    sub.close(), host.close()
    del os.environ["PMM_F32_SCREEN"]
    out["topk_1000xSx768_k100"] = {
        "derived_ms": spread(ta), "host_built_ms": spread(tb),
        "bit_equal_after_mapping": bool(np.array_equal(gi, ids[hi]) and
                                        np.array_equal(gs.view(np.uint32), hs.view(np.uint32)))}
    parent.close()

    # c. the remap launch
    g = np.random.default_rng(7)
    c1, q1 = g.standard_normal((10000, 256), dtype=np.float32), g.standard_normal((1000, 256), dtype=np.float32)
    p1 = _native.DeviceCorpus(c1)
    s1 = p1.subset(np.ones(10000, bool))
    ta, tb, tr = [], [], []
    _native.timing_enable(True)
    for i in range(4 * args.reps + 2):
        _native.timing_reset()
        a, _ = wall(lambda: s1.topk(q1, 10, COS))
        r = _native.timing_read("remap_index")[0]
        b, _ = wall(lambda: p1.topk(q1, 10, COS))
        if i >= 2:
            ta.append(a), tb.append(b), tr.append(r)
    _native.timing_reset()
    _native.timing_enable(False)
    s1.close(), p1.close()
    out["remap_1000x10000x256_k10"] = {"derived_ms": spread(ta), "parent_ms": spread(tb),
                                       "remap_index_event_ms": spread(tr),
                                       "note": "wall clocks taken with the library's event timing on"}

    # d. _topk end to end, second calls
    aq, ac = fixed(q), fixed(c)
    af = fixed(np.ascontiguousarray(c[ids]))
    pm.clear_corpus_cache()
    first_subset, _ = wall(lambda: pm._topk(aq, ac, 100, "cosine", subset=amask))
    first_filtered, _ = wall(lambda: pm._topk(aq, af, 100, "cosine"))
    ta, tb = [], []
    for i in range(args.reps):
        a, ra = wall(lambda: pm._topk(aq, ac, 100, "cosine", subset=amask))
        b, rb = wall(lambda: pm._topk(aq, af, 100, "cosine"))
        ta.append(a), tb.append(b)
    ia = ra.values.field("index").to_numpy(zero_copy_only=False)
    ib = rb.values.field("index").to_numpy(zero_copy_only=False)
    pm.clear_corpus_cache()
    out["_topk_1000x1Mx768_k100_half_mask"] = {
        "subset_first_call_ms": first_subset, "prefiltered_first_call_ms": first_filtered,
        "subset_cache_hit_ms": spread(ta), "prefiltered_cache_hit_ms": spread(tb),
        "indices_equal_after_mapping": bool(np.array_equal(ia, ids[ib]))}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
