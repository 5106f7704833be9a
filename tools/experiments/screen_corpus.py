#!/usr/bin/env python3
"""Measurements of the f32 cosine screen on corpus handles (profiles/screen_corpus/README.md).

One process, one GPU.  The new library is polars_matmul/libpmm.so; --parent names a library built from
the parent commit (loaded beside it through ctypes alone, since it lacks the new entries), whose handle
calls run unscreened.  Variants alternate inside one loop; figures are medians with min and max.

  python tools/experiments/screen_corpus.py --parent polars-matmul_amd/polars_matmul/libpmm_parent.so \
      --out profiles/screen_corpus/measure.json [--only c3,stages,crossover,kernel,zero]
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

COS = 0
STAGES = ("norms_f32/prepare", "norms_f32/round", "seed_bf16/screen", "gemm_f32_topk/screen", "merge_topk/rescore",
          "merge_topk", "norms_f32", "gemm_f32_topk", "gemm_f32_seed", "seed_select", "h2d", "d2h",
          "corpus_image_build")
vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


class Lib:
    """The handle entries of one library through ctypes (works for the parent's library too)."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.pmm_corpus_create_f32.argtypes = [vp, i64, i64, ctypes.POINTER(vp)]
        self.lib.pmm_topk_f32_corpus.argtypes = [vp, vp, i64, i64, i32, vp, vp]
        self.lib.pmm_corpus_destroy.argtypes = [vp]
        self.lib.pmm_last_error.restype = ctypes.c_char_p

    def create(self, c):
        h = vp()
        rc = self.lib.pmm_corpus_create_f32(c.ctypes.data, c.shape[0], c.shape[1], ctypes.byref(h))
        assert rc == 0, self.lib.pmm_last_error()
        return h

    def topk(self, h, q, k, idx, sc):
        t = time.perf_counter()
        rc = self.lib.pmm_topk_f32_corpus(h, q.ctypes.data, q.shape[0], k, COS, idx.ctypes.data, sc.ctypes.data)
        dt = (time.perf_counter() - t) * 1e3
        assert rc == 0, self.lib.pmm_last_error()
        return dt

    def destroy(self, h):
        self.lib.pmm_corpus_destroy(h)


def handle_bytes(h):
    out = ctypes.c_size_t(0)
    _native.check(_native.lib().pmm_corpus_bytes(h, ctypes.byref(out)))
    return out.value


def split():
    """{stage: ms} of the calling thread's timing records (exact label match is not offered: longer labels
    that contain a shorter one are subtracted)."""
    raw = {s: _native.timing_read(s) for s in STAGES}
    out = {}
    for s, (ms, cnt) in raw.items():
        for t, (ms2, cnt2) in raw.items():
            if t != s and s in t:
                ms, cnt = ms - ms2, cnt - cnt2
        if cnt:
            out[s] = round(ms, 4)
    return out


def rand(rows, d, seed):
    return np.random.default_rng(seed).standard_normal((rows, d), dtype=np.float32)


def timed_new(new, h, q, k, idx, sc):
    _native.timing_enable(True)
    _native.timing_reset()
    ms = new.topk(h, q, k, idx, sc)
    sp = split()
    _native.timing_reset()
    _native.timing_enable(False)
    return ms, sp


def stage_sum(sp):
    return sum(v for s, v in sp.items() if s not in ("h2d", "d2h", "corpus_image_build"))


def run_c3(new, parent, res, m, n, d, k, rounds):
    os.environ.pop("PMM_F32_SCREEN", None)
    c, q = rand(n, d, 1), rand(m, d, 2)
    idx, sc = np.empty((m, k), np.uint32), np.empty((m, k), np.float32)
    idx_p, sc_p = np.empty((m, k), np.uint32), np.empty((m, k), np.float32)
    hn = new.create(c)
    hp = parent.create(c) if parent else None
    b0 = handle_bytes(hn)
    first_ms, first_split = timed_new(new, hn, q, k, idx, sc)  # builds the image
    out = {"shape": [m, n, d, k], "first_call_ms": first_ms, "first_call_split": first_split,
           "image_build_ms": first_split.get("corpus_image_build"), "image_bytes": handle_bytes(hn) - b0}
    t_new, t_par, splits = [], [], []
    for _ in range(rounds):
        ms, sp = timed_new(new, hn, q, k, idx, sc)
        t_new.append(ms)
        splits.append(sp)
        if parent:
            t_par.append(parent.topk(hp, q, k, idx_p, sc_p))
    out["new_ms"] = med(t_new)
    out["new_split_median"] = {s: statistics.median([sp.get(s, 0.0) for sp in splits]) for s in splits[0]}
    out["new_stage_sum_ms"] = med([stage_sum(sp) for sp in splits])
    if parent:
        out["parent_ms"] = med(t_par)
        out["lists_equal"] = bool(np.array_equal(idx, idx_p) and np.array_equal(sc.view(np.uint32), sc_p.view(np.uint32)))
        parent.destroy(hp)
    res["c3"] = out
    return c, q, hn


def run_stages(res, c, q, k, rounds):
    """The device entry's screened call at the same shape, rows resident (torch), its timed stages summed."""
    import torch

    m, d = q.shape
    n = c.shape[0]
    dev = torch.device("cuda:0")
    tq, tc = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)
    oi = torch.empty((m, k), dtype=torch.int32, device=dev)
    osc = torch.empty((m, k), dtype=torch.float32, device=dev)
    wb = _native.workspace_bytes(m, n, d, k, COS)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    sums, splits = [], []
    for r in range(rounds + 1):
        _native.timing_enable(True)
        _native.timing_reset()
        _native.topk_device(tq.data_ptr(), d, m, tc.data_ptr(), d, n, d, k, COS, oi.data_ptr(), osc.data_ptr(),
                            workspace=ws.data_ptr(), workspace_bytes=wb, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        sp = split()
        _native.timing_reset()
        _native.timing_enable(False)
        if r:
            sums.append(stage_sum(sp))
            splits.append(sp)
    res["device_entry"] = {"workspace_bytes": wb, "stage_sum_ms": med(sums),
                           "split_median": {s: statistics.median([sp.get(s, 0.0) for sp in splits]) for s in splits[0]}}
    del tq, tc, ws
    torch.cuda.empty_cache()


def run_crossover(new, res, d, k, rounds):
    table = []
    for m, n in ((1000, 10_000), (1000, 100_000), (1000, 1_000_000), (10_000, 100_000), (100_000, 10_000),
                 (100_000, 100_000), (10_000, 1_000_000)):
        c, q = rand(n, d, n), rand(m, d, m)
        idx, sc = np.empty((m, k), np.uint32), np.empty((m, k), np.float32)
        h = new.create(c)
        t = {"0": [], "1": []}
        for r in range(rounds + 1):
            for knob in ("1", "0"):
                os.environ["PMM_F32_SCREEN"] = knob
                ms = new.topk(h, q, k, idx, sc)
                if r:
                    t[knob].append(ms)
        os.environ.pop("PMM_F32_SCREEN")
        new.destroy(h)
        table.append({"m": m, "n": n, "f32_handle_ms": med(t["0"]), "screened_handle_ms": med(t["1"])})
        print(json.dumps(table[-1]), flush=True)
    res["crossover"] = table


def run_kernel(res, n, d, rounds):
    """screen_prepare_kernel over n x d against the two-pass preparation of the device entry (its
    "norms_f32/round" records with one query row: norms_pair + screen_round over the corpus, plus the query
    row's launches)."""
    import torch

    dev = torch.device("cuda:0")
    tc = torch.from_numpy(rand(n, d, 5)).to(dev)
    dpb = -(-d // 128) * 128
    out = torch.empty((n, dpb), dtype=torch.int16, device=dev)
    f = [torch.empty((n,), dtype=torch.float32, device=dev) for _ in range(3)]
    bad = torch.empty((n,), dtype=torch.int32, device=dev)
    pair = torch.zeros(2, dtype=torch.int32, device=dev)
    tq = torch.from_numpy(rand(1, d, 6)).to(dev)
    oi = torch.empty((1, 100), dtype=torch.int32, device=dev)
    osc = torch.empty((1, 100), dtype=torch.float32, device=dev)
    os.environ["PMM_F32_SCREEN"] = "1"
    st = torch.cuda.current_stream().cuda_stream
    one, two = [], []
    for r in range(rounds + 1):
        _native.timing_enable(True)
        _native.timing_reset()
        _native.screen_prepare_device(tc.data_ptr(), d, n, d, out.data_ptr(), dpb, norm=f[0].data_ptr(),
                                      inv_norm=f[1].data_ptr(), rel=f[2].data_ptr(), unsafe=bad.data_ptr(),
                                      scalars=pair.data_ptr(), stream=st)
        _native.topk_device(tq.data_ptr(), d, 1, tc.data_ptr(), d, n, d, 100, COS, oi.data_ptr(), osc.data_ptr(),
                            stream=st)
        torch.cuda.synchronize()
        a, b = _native.timing_read("screen_prepare")[0], _native.timing_read("norms_f32/round")[0]
        _native.timing_reset()
        _native.timing_enable(False)
        if r:
            one.append(a)
            two.append(b)
    os.environ.pop("PMM_F32_SCREEN")
    elems = n * d
    res["kernel"] = {"shape": [n, d], "screen_prepare_ms": med(one), "two_pass_ms": med(two),
                     "screen_prepare_TBps_at_6B": 6 * elems / (statistics.median(one) * 1e-3) / 1e12,
                     "two_pass_TBps_at_10B": 10 * elems / (statistics.median(two) * 1e-3) / 1e12}


def run_zero(new, parent, res, c, q, k, rounds):
    c = c.copy()
    c[12345, :] = 0.0
    m = q.shape[0]
    idx, sc = np.empty((m, k), np.uint32), np.empty((m, k), np.float32)
    hn = new.create(c)
    hp = parent.create(c) if parent else None
    first, sp = timed_new(new, hn, q, k, idx, sc)
    later, par = [], []
    for _ in range(rounds):
        later.append(new.topk(hn, q, k, idx, sc))
        if parent:
            par.append(parent.topk(hp, q, k, idx, sc))
    res["zero_row"] = {"first_call_ms": first, "first_call_split": sp, "later_ms": med(later),
                       "bytes_after": handle_bytes(hn), "parent_ms": med(par) if par else None}
    new.destroy(hn)
    if parent:
        parent.destroy(hp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--out", default="profiles/screen_corpus/measure.json")
    ap.add_argument("--only", default="c3,stages,crossover,kernel,zero")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    only = a.only.split(",")
    new = Lib(_native.LIB_PATH)
    parent = Lib(os.path.abspath(a.parent)) if a.parent else None
    res = {}
    if os.path.exists(a.out):
        res = json.load(open(a.out))
    d, k = 768, 100
    c = q = hn = None

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)

    if "c3" in only or "stages" in only or "zero" in only:
        c, q, hn = run_c3(new, parent, res, a.m, a.n, d, k, a.rounds)
        print(json.dumps(res["c3"]), flush=True)
        new.destroy(hn)
        save()
    if "stages" in only:
        run_stages(res, c, q, k, a.rounds)
        print(json.dumps(res["device_entry"]), flush=True)
        save()
    if "zero" in only:
        run_zero(new, parent, res, c, q, k, a.rounds)
        print(json.dumps(res["zero_row"]), flush=True)
        save()
    c = q = None
    if "kernel" in only:
        run_kernel(res, a.n, d, a.rounds)
        print(json.dumps(res["kernel"]), flush=True)
        save()
    if "crossover" in only:
        run_crossover(new, res, d, k, a.rounds)
    save()


if __name__ == "__main__":
    main()
