#!/usr/bin/env python3
"""Duplicate groups (pmm_components_f32_self) against what the parent commit
offers for the same job: ``range_self`` and a union-find on the host over its
CSR lists.  Writes one JSON document to stdout (profiles/components/).

    python tools/measure_components.py > profiles/components/measure.json

Case a: n x d f32 rows (random normal), cosine, a threshold that leaves about
`hits` rows per row in a full range call.  The components pass
(``gemm_f32_components``) against the self emit pass run count-only
(``gemm_f32_self``, cap = 0) -- the same library, the same process, alternating,
both from the HIP-event timers -- and the whole components call against
``range_self`` with lists plus the host union-find (numpy: hook every label
onto the smaller one across each pair, jump pointers, until nothing moves).
Case b: the same rows with `copies` of them replaced by one repeated row: the
components call against ``range_self`` count-only, the only form of it that
fits in memory there, and the device memory each call's arena takes (the drop
in free memory over the first call of a fresh thread: arenas are per thread).
The self entries are untouched by this change, so this tree's library is the
parent's for them.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))
from polars_matmul import _native  # noqa: E402

COS = _native.METRIC_COSINE


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def host_components(offsets, idx, n):
    """labels[i] = the smallest row of i's component of the CSR pairs."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    cols = idx.astype(np.int64)
    lab = np.arange(n, dtype=np.int64)
    while True:
        a, b = lab[rows], lab[cols]
        m = np.minimum(a, b)
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        while True:
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            return lab.astype(np.uint32)
        lab = new


class Calls:
    """The C entries into buffers allocated once."""

    def __init__(self, dc, t, cap):
        n = dc.n
        self.dc, self.t, self.cap, self.n = dc, t, cap, n
        self.labels = np.empty(n, np.uint32)
        self.offsets = np.empty(n + 1, np.int64)
        self.idx, self.sc = np.empty(cap, np.uint32), np.empty(cap, np.float32)
        self.components = self.pairs = self.total = self.count_total = 0
        self.host_labels = None

    def components_call(self):
        nc, npairs = ctypes.c_int64(0), ctypes.c_int64(0)
        _native.check(_native.lib().pmm_components_f32_self(self.dc._h, self.t, COS, _native.ptr(self.labels),
                                                            ctypes.byref(nc), ctypes.byref(npairs)))
        self.components, self.pairs = nc.value, npairs.value

    def self_count(self):
        total = ctypes.c_int64(0)
        _native.check(_native.lib().pmm_range_f32_self(self.dc._h, self.t, COS, 0, _native.ptr(self.offsets), None,
                                                       None, ctypes.byref(total)))
        self.count_total = total.value

    def self_lists(self):
        total = ctypes.c_int64(0)
        _native.check(_native.lib().pmm_range_f32_self(self.dc._h, self.t, COS, self.cap, _native.ptr(self.offsets),
                                                       _native.ptr(self.idx), _native.ptr(self.sc),
                                                       ctypes.byref(total)))
        self.total = total.value
        assert self.total <= self.cap

    def parent_way(self):
        self.self_lists()
        self.host_labels = host_components(self.offsets, self.idx[:self.total], self.n)


def alternate(pairs, rounds):
    """pairs: (name, fn, timer name or None) run in turn, `rounds` times."""
    ms = {}
    for _ in range(rounds):
        for name, fn, timer in pairs:
            _native.timing_reset()
            ms.setdefault(name, []).append(timed(fn))
            if timer:
                ms.setdefault(timer, []).append(_native.timing_read(timer)[0])
    return ms


def arena_taken(fn):
    """The drop in free device memory over fn's first call on a fresh thread."""
    out = []

    def run():
        before = _native.device_memory()[0]
        fn()
        out.append(before - _native.device_memory()[0])

    th = threading.Thread(target=run)
    th.start()
    th.join()
    return int(out[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262_144)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--hits", type=float, default=10.0)
    ap.add_argument("--copies", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rounds-b", type=int, default=2)
    ap.add_argument("--case", choices=["a", "b", "both"], default="both")
    a = ap.parse_args()
    n, d = a.n, a.d
    rng = np.random.default_rng(0)
    c = rng.standard_normal((n, d), dtype=np.float32)
    # cosine of random rows ~ N(0, 1/d): the tail that leaves `hits` of n rows
    t = float(np.float32(statistics.NormalDist().inv_cdf(1.0 - a.hits / n) / np.sqrt(d)))
    out = {"workload": dict(vars(a), threshold=t), "device_count": _native.device_count()}
    med = statistics.median
    _native.timing_enable(True)

    if a.case in ("a", "both"):
        dc = _native.DeviceCorpus(c)
        calls = Calls(dc, t, max(1 << 16, 64 * n))
        for fn in (calls.components_call, calls.self_count, calls.parent_way):  # warm-up
            fn()
        ms = alternate([("components_call", calls.components_call, "gemm_f32_components"),
                        ("self_count_call", calls.self_count, "gemm_f32_self")], a.rounds)
        ms.update(alternate([("components_call_2", calls.components_call, None),
                             ("range_self_plus_host_union_find", calls.parent_way, None)], a.rounds))
        ms["host_union_find"] = [timed(lambda: host_components(calls.offsets, calls.idx[:calls.total], n))
                                 for _ in range(a.rounds)]
        _native.timing_reset()
        calls.components_call()
        label_ms = _native.timing_read("components_label")[0]
        out["a"] = {
            "ms": {k: med(v) for k, v in ms.items()}, "rounds_ms": ms, "components_label_ms": label_ms,
            "pairs": calls.pairs, "components": calls.components, "range_self_total": calls.total,
            "count_only_total": calls.count_total,
            "labels_equal_host": bool(np.array_equal(calls.labels, calls.host_labels)),
            "ratio": {"pass_components_over_self": med(ms["gemm_f32_components"]) / med(ms["gemm_f32_self"]),
                      "call_components_over_parent_way":
                          med(ms["components_call_2"]) / med(ms["range_self_plus_host_union_find"])},
        }
        print(f"a: pass {med(ms['gemm_f32_components']):.1f} vs self count-only {med(ms['gemm_f32_self']):.1f} ms; "
              f"call {med(ms['components_call_2']):.1f} vs range_self + host {med(ms['range_self_plus_host_union_find']):.1f}"
              f" ms; pairs {calls.pairs} = {calls.total}; equal {out['a']['labels_equal_host']}", file=sys.stderr,
              flush=True)
        dc.close()

    if a.case in ("b", "both"):
        rows = np.sort(rng.permutation(n)[:a.copies])
        cb = c.copy()
        cb[rows] = cb[rows[0]]
        small = _native.DeviceCorpus(cb[:1024])  # (code objects loaded before free memory is read)
        warm = Calls(small, t, 1)
        warm.components_call(), warm.self_count()
        small.close()
        dc = _native.DeviceCorpus(cb)
        calls = Calls(dc, t, 1)
        arena = {"components": arena_taken(calls.components_call), "range_self_count_only": arena_taken(calls.self_count)}
        for fn in (calls.components_call, calls.self_count):  # warm-up on this thread
            fn()
        ms = alternate([("components_call", calls.components_call, "gemm_f32_components"),
                        ("self_count_call", calls.self_count, "gemm_f32_self")], a.rounds_b)
        group = a.copies * (a.copies - 1) // 2
        out["b"] = {
            "ms": {k: med(v) for k, v in ms.items()}, "rounds_ms": ms, "pairs": calls.pairs,
            "count_only_total": calls.count_total, "pairs_of_the_repeated_row": group,
            "components": calls.components,
            # (the copies' component may hold other rows too, some below the first copy)
            "copies_share_one_label": bool((calls.labels[rows] == calls.labels[rows[0]]).all()
                                           and calls.labels[rows[0]] <= rows[0]),
            "arena_bytes": arena,
            "range_self_list_run_record_bytes": 20 * calls.count_total,
            "ratio": {"pass_components_over_self": med(ms["gemm_f32_components"]) / med(ms["gemm_f32_self"])},
        }
        print(f"b: pass {med(ms['gemm_f32_components']):.1f} vs self count-only {med(ms['gemm_f32_self']):.1f} ms; "
              f"pairs {calls.pairs} = {calls.count_total}; arena {arena}", file=sys.stderr, flush=True)
        dc.close()
    _native.timing_enable(False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
