"""Signed zeros, subnormals, overflow and non-finite values on every exact path.

Every test runs the five value cases of ``tests/value_cases.py`` through one
route and ends at ``oracle.topk`` (``oracle.matmul`` / ``oracle.norms`` for the
two routes that return no lists) on the same inputs: indices equal, score bits
equal with NaN equal to NaN, lengths equal where a route returns them.  There
are no tolerances in this file and no comparison of one device path with
another only.

Shapes: m = 19, n = 300, d = 37 (ragged in all three dimensions, two
256-column blocks, d padded to 64); routes that need more rows use n = 1100.
The oracle's full ranked list of a (width, case, n, metric) is computed once
and sliced: under the total order (score, NaN last, lower index) the top-k is
the first k entries of the ranked list.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from polars_matmul import _native
from test_gpu_grouped import assert_exact as assert_grouped_exact
from test_gpu_grouped import truth as grouped_truth
from test_gpu_parity import assert_bitexact
from test_gpu_range import assert_same as assert_same_csr
from test_gpu_range import cut, ranked
from value_cases import CASES, value_case

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
METRICS = (COS, DOT, EUC)
ORACLE_METRIC = {COS: oracle.COSINE, DOT: oracle.DOT, EUC: oracle.EUCLIDEAN}
NAME = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
M, N, D = 19, 300, 37
N_BIG = 1100
F32, F64 = np.float32, np.float64
WIDTH = {"f32": F32, "f64": F64}

case_param = pytest.mark.parametrize("case", CASES)
width_param = pytest.mark.parametrize("width", ["f32", "f64"])


@functools.lru_cache(maxsize=None)
def inputs(width, case, n=N):
    q, c = value_case(case, WIDTH[width], M, n, D)
    q.setflags(write=False)
    c.setflags(write=False)
    return q, c


@functools.lru_cache(maxsize=None)
def full_lists(width, case, n, metric):
    """The oracle's ranked lists over all n rows: (indices, f64 scores)."""
    q, c = inputs(width, case, n)
    oi, osc = oracle.topk(q, c, n, ORACLE_METRIC[metric])
    oi, osc = np.asarray(oi), np.asarray(osc)
    oi.setflags(write=False)
    osc.setflags(write=False)
    return oi, osc


def want_topk(width, case, n, metric, k):
    oi, osc = full_lists(width, case, n, metric)
    return oi[:, :k], osc[:, :k]


def same_bits(got, want, dtype):
    got, want = np.ascontiguousarray(got, dtype), np.ascontiguousarray(want, dtype)
    u = np.uint32 if np.dtype(dtype) == F32 else np.uint64
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))


def assert_lists(got, want, width, label):
    """got == want: indices, and score bits (NaN == NaN) in the route's width."""
    idx, sc = got
    oi, osc = want
    if width == "f32":
        assert sc.dtype == F32, label
        assert_bitexact(idx, sc, oi, osc, label)
        return
    assert sc.dtype == F64 and idx.shape == oi.shape, (label, sc.dtype, idx.shape, oi.shape)
    bad = idx.astype(np.int64) != oi.astype(np.int64)
    assert not bad.any(), f"{label}: {int(bad.sum())} indices differ, first at {np.argwhere(bad)[0]}"
    same = same_bits(sc, osc, F64)
    assert same.all(), (f"{label}: {int((~same).sum())} scores differ, e.g. "
                        f"{[hex(x) for x in sc[~same][:3].view(np.uint64)]} vs "
                        f"{[hex(x) for x in np.ascontiguousarray(osc)[~same][:3].view(np.uint64)]}")


def host_topk(width, case, n, metric, k, label):
    q, c = inputs(width, case, n)
    assert_lists(_native.topk_host(q, c, k, metric), want_topk(width, case, n, metric, k), width,
                 f"{label} {case} {NAME[metric]} k={k}")


@pytest.fixture
def device_list():
    yield
    _native.set_devices([])


# ---- fused f32 top-k, default plan ----
@case_param
def test_f32_fused_default_plan(case):
    for metric in METRICS:
        for k in (1, 10, N):
            host_topk("f32", case, N, metric, k, "fused f32")


# ---- each tile variant (n = 1100: more than one tile, a candidate compaction) ----
@case_param
def test_f32_every_tile_variant(case, monkeypatch):
    for variant in ("0", "1", "2", "3", "4", "5", "5:whole"):
        if variant.endswith(":whole"):
            variant = variant.split(":")[0]
            monkeypatch.setenv("PMM_CUS", "4")
        monkeypatch.setenv("PMM_GEMM_VARIANT", variant)
        for metric in METRICS:
            host_topk("f32", case, N_BIG, metric, 10, f"variant {variant}")


# ---- threshold seeding, each seed mode the suite forces ----
SEED_MODES = ({}, {"PMM_SEED_GEMM": "1"}, {"PMM_SEED_LDS": "1"}, {"PMM_SEED_MFMA": "0"}, {"PMM_SEED_MFMA": "1"})


@case_param
def test_f32_threshold_seeding(case, monkeypatch):
    monkeypatch.setenv("PMM_SEED", "1")
    for mode in SEED_MODES:
        with monkeypatch.context() as mp:
            for key, val in mode.items():
                mp.setenv(key, val)
            for metric in METRICS:
                host_topk("f32", case, N_BIG, metric, 10, f"seed {mode}")


# ---- materialised f32: k past the fused limit of 1024 ----
@case_param
def test_f32_materialised_k_above_1024(case):
    for metric in METRICS:
        for k in (1025, N_BIG):
            host_topk("f32", case, N_BIG, metric, k, "materialised f32")


# ---- screened cosine, on host arrays and on a handle ----
@case_param
def test_f32_screened_cosine(case, monkeypatch):
    # whatever the screen decides (rows re-run, or the whole call handed to the
    # f32 kernel: these inputs are full of rows it calls unsafe), the lists are
    # the oracle's
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    q, c = inputs("f32", case)
    for k in (10, 100):
        want = want_topk("f32", case, N, COS, k)
        assert_lists(_native.topk_host(q, c, k, COS), want, "f32", f"screened host {case} k={k}")
        dc = _native.DeviceCorpus(c)
        try:
            for call in ("first", "cached image"):
                assert_lists(dc.topk(q, k, COS), want, "f32", f"screened handle ({call}) {case} k={k}")
        finally:
            dc.close()


# ---- .pmm.matmul ----
@width_param
@case_param
def test_matmul(case, width):
    q, c = inputs(width, case)
    got, want = _native.matmul_host(q, c), oracle.matmul(q, c)
    same = same_bits(got, want, WIDTH[width])
    assert got.dtype == want.dtype and same.all(), \
        f"matmul {width} {case}: {int((~same).sum())} of {same.size} differ, e.g. {got[~same][:3]} vs {want[~same][:3]}"


# ---- norms ----
@width_param
@case_param
def test_norms(case, width):
    import torch

    dt = WIDTH[width]
    dev = torch.device("cuda:0")
    ld = D + 3
    for side, a in zip("qc", inputs(width, case)):
        rows = a.shape[0]
        buf = torch.zeros((rows, ld), dtype=torch.float32 if dt == F32 else torch.float64, device=dev)
        buf[:, :D] = torch.from_numpy(np.array(a)).to(dev)
        out = torch.empty(rows, dtype=buf.dtype, device=dev)
        for squared in (False, True):
            _native.norms_device(buf.data_ptr(), ld, rows, D, squared, out.data_ptr(), f64=dt == F64,
                                 stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got, want = out.cpu().numpy(), oracle.norms(np.array(a), squared=squared)
            same = same_bits(got, want, dt)
            assert same.all(), (f"norms {width} {case} {side} squared={squared}: rows {np.flatnonzero(~same)[:5]} "
                                f"{got[~same][:3]} vs {want[~same][:3]}")


# ---- corpus handle and subset (f32 and f64 parents) ----
def subset_truth(q, c, ids, k, metric):
    oi, osc = oracle.topk(q, np.ascontiguousarray(c[ids]), k, ORACLE_METRIC[metric])
    return ids[np.asarray(oi).astype(np.int64)].astype(np.uint32), np.asarray(osc)


@width_param
@case_param
def test_handle_and_subset(case, width):
    # the mask keeps every other row and the complement the rest, so every
    # planted row is searched in one of the two derived handles
    q, c = inputs(width, case)
    mask = np.arange(N) % 2 == 0
    dc = _native.DeviceCorpus(c)
    try:
        subs = [(sel, dc.subset(sel)) for sel in (mask, ~mask)]
        try:
            for metric in METRICS:
                for k in (10, N):
                    assert_lists(dc.topk(q, k, metric), want_topk(width, case, N, metric, k), width,
                                 f"handle {width} {case} {NAME[metric]} k={k}")
                for sel, sub in subs:
                    ids = np.flatnonzero(sel)
                    for k in (10, ids.size):
                        assert_lists(sub.topk(q, k, metric), subset_truth(q, c, ids, k, metric), width,
                                     f"subset {width} {case} {NAME[metric]} k={k} first row {ids[0]}")
        finally:
            for _, sub in subs:
                sub.close()
    finally:
        dc.close()


# ---- grouped, kernel and loop (f32), loop (f64) ----
@width_param
@case_param
def test_grouped_kernel_and_loop(case, width, monkeypatch):
    # three labels, row r in group r % 3: the planted rows (value_cases.
    # SIGNED_ZERO_ROWS, NONFINITE_ROWS) fall in all three; every query visits
    # every group over the three label shifts.  k = 128 exceeds a group's 100
    # rows: the lists are padded and the lengths compared.  (An f64 handle has
    # no grouped kernel: PMM_GROUPED=kernel takes the loop there, as it does
    # for any k or d beyond the kernel's limits.)
    q, c = inputs(width, case)
    dt = WIDTH[width]
    cl = (np.arange(N) % 3).astype(np.uint32)
    dc = _native.DeviceCorpus(c)
    try:
        part = dc.partition(cl, 3)
        try:
            for shift in range(3):
                ql = ((np.arange(M) + shift) % 3).astype(np.uint32)
                for metric in METRICS:
                    for k in (10, 128):
                        want = grouped_truth(q, c, ql, cl, k, metric)
                        for path in ("kernel", "loop"):
                            monkeypatch.setenv("PMM_GROUPED", path)
                            assert_grouped_exact(part.topk_grouped(q, ql, k, metric), want, k,
                                                 f"grouped {path} {width} {case} {NAME[metric]} k={k} shift={shift}", dt)
        finally:
            part.close()
    finally:
        dc.close()


# ---- range ----
@case_param
def test_range(case):
    q, c = inputs("f32", case)
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            full = ranked(q, c, metric)
            finite = full[1][np.isfinite(full[1])]
            thresholds = [0.0, -0.0, float("inf"), float("-inf")]
            if finite.size:
                thresholds.append(float(np.median(finite)))
            for t in thresholds:
                assert_same_csr(dc.range(q, t, metric), cut(full, t, metric), f"range {case} {NAME[metric]} t={t!r}")
    finally:
        dc.close()


# ---- f64 fused and materialised ----
@case_param
def test_f64_fused_and_materialised(case, monkeypatch):
    for fused, tile in (("1", "64"), ("1", "128"), ("0", "64")):
        monkeypatch.setenv("PMM_F64_FUSED", fused)
        monkeypatch.setenv("PMM_F64_TILE", tile)
        for metric in METRICS:
            for k in (10, N):
                host_topk("f64", case, N, metric, k, f"f64 fused={fused} tile={tile}")


# ---- sharded f32 and f64: host arrays and a handle ----
@width_param
@case_param
def test_sharded(case, width, device_list):
    # three shards of 100 rows on one device; k = 150 is larger than a shard
    q, c = inputs(width, case)
    _native.set_devices([0, 0, 0])
    dc = _native.DeviceCorpus(c)
    try:
        assert dc.shards == 3
        for metric in METRICS:
            for k in (10, 150):
                want = want_topk(width, case, N, metric, k)
                assert_lists(_native.topk_host(q, c, k, metric), want, width,
                             f"sharded host {width} {case} {NAME[metric]} k={k}")
                assert_lists(dc.topk(q, k, metric), want, width, f"sharded handle {width} {case} {NAME[metric]} k={k}")
    finally:
        dc.close()


# ---- sharded lists shorter than k with an odd number of entries ----
@pytest.mark.parametrize("width,fused", [("f64", "1"), ("f64", "0"), ("f32", None)])
def test_sharded_short_shards_odd_sizes(width, fused, device_list, monkeypatch):
    # m = 31, 8 shards of 12 or 13 rows, k = 64: every shard's compact list
    # holds m * kg entries, an odd number for the 13-row shards (the f64 score
    # half sits at an offset of its own, 8-byte aligned)
    if fused is not None:
        monkeypatch.setenv("PMM_F64_FUSED", fused)
    m, n, d, k = 31, 101, 37, 64
    rs = np.random.RandomState(11)
    q, c = rs.randn(m, d).astype(WIDTH[width]), rs.randn(n, d).astype(WIDTH[width])
    c[n - 5:] = c[:5]  # ties across shards
    _native.set_devices([0] * 8)
    for metric in METRICS:
        oi, osc = oracle.topk(q, c, k, ORACLE_METRIC[metric])
        assert_lists(_native.topk_host(q, c, k, metric), (np.asarray(oi), np.asarray(osc)), width,
                     f"short shards {width} fused={fused} {NAME[metric]}")
