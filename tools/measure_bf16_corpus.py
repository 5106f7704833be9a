"""Measurements of the bf16 corpus handle (profiles/bf16_corpus/README.md).

  python tools/measure_bf16_corpus.py [--out FILE] [--reps N]

a. round_norms_bf16 (one launch: rows rounded and all four norm arrays) at
   1M x 768 against the three launches it replaces (f32_to_bf16, norms_bf16
   with squared = 0 and 1), each timed by the library's own stream events
   (pmm_timing_*): the first through a handle creation, the others through the
   host bf16 call, which runs them on buffers of the same shape.
b. a bf16 top-k through the handle against the host call
   (topk_host(..., COMPUTE_BF16), what the parent does), wall clock.
c. free HBM before and after a handle's creation against corpus_device_bytes.

Runs alternate between the variants; medians with the minimum and maximum.
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

from polars_matmul import _native  # noqa: E402

COS, EUC, BF16 = _native.METRIC_COSINE, _native.METRIC_EUCLIDEAN, _native.COMPUTE_BF16


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    out = {}
    n, d = 1_000_000, 768
    c = np.random.default_rng(42).standard_normal((n, d), dtype=np.float32)
    q = np.random.default_rng(43).standard_normal((1000, d), dtype=np.float32)

    # c. memory, first: nothing of this process is on the device yet but the runtime
    _native.device_memory()
    free0, total = _native.device_memory()
    t = time.perf_counter()
    dc = _native.DeviceCorpus(c, compute="bf16")
    create_ms = (time.perf_counter() - t) * 1e3
    free1, _ = _native.device_memory()
    dc.close()
    free2, _ = _native.device_memory()
    f32 = _native.DeviceCorpus(c)
    free3, _ = _native.device_memory()
    f32.close()
    out["memory_1Mx768"] = {
        "total": total, "free_before": free0, "free_after_bf16_handle": free1, "free_after_close": free2,
        "bf16_handle_took": free0 - free1, "f32_handle_took": free2 - free3,
        "corpus_device_bytes_bf16": _native.corpus_device_bytes(n, d, np.float32, compute="bf16"),
        "corpus_device_bytes_f32": _native.corpus_device_bytes(n, d, np.float32),
        "first_creation_wall_ms": create_ms,
    }

    # a. the one-pass kernel against the three launches
    _native.timing_enable(True)
    one, conv, ncos, neuc = [], [], [], []
    q8 = q[:8]
    for i in range(args.reps + 1):
        _native.timing_reset()
        h = _native.DeviceCorpus(c, compute="bf16")
        ms = _native.timing_read("round_norms_bf16")[0]
        h.close()
        _native.timing_reset()
        _native.topk_host(q8, c, 10, COS, compute=BF16)
        cv = _native.timing_read("f32_to_bf16")[0]
        nc = _native.timing_read("norms_bf16")[0]
        _native.timing_reset()
        _native.topk_host(q8, c, 10, EUC, compute=BF16)
        ne = _native.timing_read("norms_bf16")[0]
        if i:  # (the first round warms up)
            one.append(ms), conv.append(cv), ncos.append(nc), neuc.append(ne)
    _native.timing_reset()
    _native.timing_enable(False)
    three = [a + b + e for a, b, e in zip(conv, ncos, neuc)]
    elems = n * d
    out["kernel_1Mx768"] = {
        "round_norms_bf16_ms": spread(one), "three_launches_ms": spread(three),
        "f32_to_bf16_ms": spread(conv), "norms_bf16_cosine_ms": spread(ncos), "norms_bf16_euclidean_ms": spread(neuc),
        "round_norms_bf16_GBps_of_6B_per_element": elems * 6 / (statistics.median(one) * 1e-3) / 1e9,
        "three_launches_GBps_of_10B_per_element": elems * 10 / (statistics.median(three) * 1e-3) / 1e9,
        "note": "the three launches' events also span the 8 query rows' launches (microseconds)",
    }

    # b. handle against the host call
    for label, (m, nn, dd, k) in {"1000x10000x256_k10": (1000, 10000, 256, 10),
                                  "1000x1Mx768_k100": (1000, n, d, 100)}.items():
        if nn == n:
            cc, qq = c, q
        else:
            g = np.random.default_rng(7)
            cc, qq = g.standard_normal((nn, dd), dtype=np.float32), g.standard_normal((m, dd), dtype=np.float32)
        t = time.perf_counter()
        h = _native.DeviceCorpus(cc, compute="bf16")
        create = (time.perf_counter() - t) * 1e3
        th, tp = [], []
        for i in range(args.reps + 2):
            a = wall(lambda: h.topk(qq, k, COS))
            b = wall(lambda: _native.topk_host(qq, cc, k, COS, compute=BF16))
            if i >= 2:
                th.append(a), tp.append(b)
        gi, gs = h.topk(qq, k, COS)
        hi, hs = _native.topk_host(qq, cc, k, COS, compute=BF16)
        h.close()
        out["topk_" + label] = {"handle_ms": spread(th), "host_call_ms": spread(tp), "creation_wall_ms": create,
                                "bit_equal": bool(np.array_equal(gi, hi) and
                                                  np.array_equal(gs.view(np.uint32), hs.view(np.uint32)))}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
