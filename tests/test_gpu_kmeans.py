"""k-means on resident f32 handles (pmm_kmeans_f32_corpus, DeviceCorpus.kmeans,
polars_matmul.kmeans, _kmeans, .pmm.kmeans) against the restatement of
tests/kmeans_cases.py: labels, centroid bits, score bits, ``updates`` and
``converged`` must all be equal.  There are no tolerances in this file.

The shapes cover every d in {1, 3, 32, 33, 130, 256}, K in {1, 2, 3, 64, 257},
n in {K, 257, 1000, 5000}, both metrics and max_iter in {0, 1, 5}; each case
draws its own rows, so each computes its restatement once.  The n = 5000 cases
assert on the restatement that at least two updates changed labels.
"""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

import kmeans_cases as kc
import polars_matmul
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUC, COS = _native.METRIC_EUCLIDEAN, _native.METRIC_COSINE
NAME = {EUC: "euclidean", COS: "cosine"}
assert (EUC, COS) == (kc.EUC, kc.COS)
NO_GROUP = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, label):
    """got: the engine's five results; want: kmeans_ref's (six)."""
    assert got[3] == want[3] and bool(got[4]) == want[4], f"{label}: updates {got[3]} / {want[3]}, converged {got[4]} / {want[4]}"
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), \
        f"{label}: {np.count_nonzero(got[1] != want[1])} labels differ"
    assert np.array_equal(bits(got[2]), bits(want[2])), f"{label}: score bits differ"
    assert got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])), \
        f"{label}: centroid bits differ in rows {np.flatnonzero((bits(got[0]) != bits(want[0])).any(axis=1))[:8]}"


def run(x, init, metric, max_iter):
    dc = _native.DeviceCorpus(x)
    try:
        return dc.kmeans(init, metric, max_iter)
    finally:
        dc.close()


# ---- 1. shapes ----
# (d, K, n, metric, max_iter)
SHAPES = [
    (1, 1, 1, EUC, 0), (1, 2, 257, COS, 1), (3, 3, 1000, EUC, 5), (3, 64, 64, COS, 5), (32, 2, 1000, EUC, 5),
    (32, 64, 5000, EUC, 5), (33, 3, 257, EUC, 1), (33, 257, 257, EUC, 5), (33, 64, 1000, COS, 0),
    (130, 257, 1000, COS, 5), (130, 3, 5000, COS, 5), (130, 1, 257, EUC, 5), (256, 257, 5000, EUC, 5),
    (256, 2, 2, COS, 1), (256, 64, 257, EUC, 0), (1, 3, 5000, EUC, 5), (3, 257, 5000, COS, 1), (32, 1, 1000, COS, 1),
    (3, 257, 5000, COS, 5), (256, 2, 1000, COS, 5),
]


@pytest.mark.parametrize("d,K,n,metric,max_iter", SHAPES)
def test_shapes_equal_the_restatement(d, K, n, metric, max_iter):
    seed = 1000 * d + K + n
    # 16 planted centres whatever K is, so that few clusters split overlapping groups and move for several updates
    x, _, _ = kc.planted(n, d, 16, seed, noise=2.0)
    init = kc.default_init(x, K, seed)
    want = kc.kmeans_ref(x, init, metric, max_iter)
    print(f"d={d} K={K} n={n} {NAME[metric]} max_iter={max_iter}: updates {want[3]}, converged {want[4]}, "
          f"changes {want[5]}")
    if n == 5000 and max_iter == 5:
        assert sum(ch > 0 for ch in want[5]) >= 2, f"a degenerate case: label changes per update {want[5]}"
    assert_same(run(x, init, metric, max_iter), want, f"d={d} K={K} n={n} {NAME[metric]} max_iter={max_iter}")


# ---- 2. piece edges ----
def test_piece_edges_with_mixed_magnitudes():
    sizes = (255, 256, 257, 512, 513)
    x, init = kc.piece_edge_rows(sizes)
    want = kc.kmeans_ref(x, init, EUC, 1)
    assert tuple(np.bincount(want[1], minlength=len(sizes))) == sizes  # planted by construction
    one_level = kc.kmeans_ref(x, init, EUC, 1, piece=None)
    assert not np.array_equal(bits(want[0]), bits(one_level[0]))  # the piece order shows in these rows
    assert_same(run(x, init, EUC, 1), want, "piece edges")


# ---- 3. special rows and centroids ----
def special(d=33, n=600, seed=9):
    x, _, _ = kc.planted(n, d, 4, seed, noise=1.0)
    return x, kc.default_init(x, 4, seed)


def test_empty_cluster_keeps_its_bits():
    x, init = special()
    init[2] = np.float32(1e6)  # far from every row: no member
    init[2, 0] = np.float32(-0.0)
    for metric in (EUC,):
        want = kc.kmeans_ref(x, init, metric, 3)
        assert not (want[1] == 2).any() and np.array_equal(bits(want[0][2]), bits(init[2]))
        got = run(x, init, metric, 3)
        assert_same(got, want, "empty cluster")
        assert np.array_equal(bits(got[0][2]), bits(init[2]))


@pytest.mark.parametrize("metric", [EUC, COS])
def test_identical_centroids_tie_to_the_lower(metric):
    x, init = special()
    init[3] = init[1]
    want = kc.kmeans_ref(x, init, metric, 0)
    assert (want[1] == 1).any() and not (want[1] == 3).any()
    assert_same(run(x, init, metric, 0), want, "identical centroids, the assignment")
    # one update: the higher one stayed empty and keeps its bits (after it the two differ, so later updates may fill it)
    got = run(x, init, metric, 1)
    assert_same(got, kc.kmeans_ref(x, init, metric, 1), "identical centroids, one update")
    assert np.array_equal(bits(got[0][3]), bits(init[1]))
    assert_same(run(x, init, metric, 3), kc.kmeans_ref(x, init, metric, 3), "identical centroids, three updates")


def test_nan_row_is_in_no_cluster():
    """Rows whose every score is NaN.  Under the reference's rules only cosine
    has them -- an infinite element gives inf / inf -- since its euclidean
    epilogue folds a NaN squared distance to 0 (Rust's f32::max) and a NaN norm
    takes cosine's zero-norm branch."""
    metric = COS
    x, init = special()
    x[17, 5] = np.inf
    x[400, 0], x[400, 7] = np.inf, -np.inf
    want = kc.kmeans_ref(x, init, metric, 3)
    assert want[1][17] == NO_GROUP and want[1][400] == NO_GROUP and not np.isnan(want[0]).any()
    got = run(x, init, metric, 3)
    assert_same(got, want, "NaN rows")
    assert got[2].view(np.uint32)[17] == 0x7FC00000
    # the column form: null
    col = pa.FixedSizeListArray.from_arrays(pa.array(x.reshape(-1)), x.shape[1])
    out = pm._kmeans_labels(col, 4, NAME[metric], 3, init=init)
    assert out.type == pa.uint32() and out.null_count == 2 and not out[17].is_valid and not out[400].is_valid
    assert out.to_pylist() == [None if v == NO_GROUP else int(v) for v in want[1]]


def test_zero_row_under_cosine_is_labelled_but_not_counted():
    x, init = special()
    x[5] = 0.0
    x[6] = np.float32(1e-9)  # a norm under the zero-norm rule
    want = kc.kmeans_ref(x, init, COS, 2)
    assert want[1][5] == 0 and want[1][6] != NO_GROUP  # every score 0: the tie goes to centroid 0
    # (counting row 5 would change centroid 0: the restatement's count leaves it out)
    members = np.flatnonzero(kc.assign(x, init, COS)[0] == 0)
    total, count = kc.cluster_sum(x, members, kc.oracle.norms(x))
    assert count < members.size
    assert_same(run(x, init, COS, 2), want, "zero row")


# ---- 4. entries ----
def test_subset_handle_numbers_its_own_rows():
    x, _, _ = kc.planted(700, 33, 5, 3, noise=1.5)
    ids = np.arange(1, 700, 3, dtype=np.uint32)
    sub_rows = np.ascontiguousarray(x[ids])
    init = kc.default_init(sub_rows, 5, 1)
    dc = _native.DeviceCorpus(x)
    try:
        sub = dc.subset(ids)
        try:
            for metric in (EUC, COS):
                got = sub.kmeans(init, metric, 4)
                assert got[1].shape == (ids.size,)
                assert_same(got, kc.kmeans_ref(sub_rows, init, metric, 4), f"subset {NAME[metric]}")
        finally:
            sub.close()
    finally:
        dc.close()


def raw(dc, K, init, metric, max_iter, n):
    cent = np.empty((K, init.shape[1]), dtype=np.float32)
    labels = np.empty(n, dtype=np.uint32)
    sc = np.empty(n, dtype=np.float32)
    up, cv = ctypes.c_int64(-1), ctypes.c_int(-1)
    rc = _native.lib().pmm_kmeans_f32_corpus(dc._h, K, _native.ptr(init), metric, max_iter, _native.ptr(cent),
                                             _native.ptr(labels), _native.ptr(sc), ctypes.byref(up), ctypes.byref(cv))
    return rc, _native.last_error()


def test_other_handles_are_refused_and_the_handle_serves_on():
    x, _, _ = kc.planted(300, 32, 3, 4)
    init = kc.default_init(x, 3, 4)
    made = []
    try:
        f = _native.DeviceCorpus(x)
        made.append(f)
        want = kc.kmeans_ref(x, init, EUC, 2)
        others = [("partitioned", f.partition((np.arange(300) % 3).astype(np.uint32), 3)),
                  ("f64", _native.DeviceCorpus(x.astype(np.float64))), ("bf16", _native.DeviceCorpus(x, compute="bf16")),
                  ("int8", _native.DeviceCorpus.int8((x * 10).astype(np.int8))), ("bit", f.sign_bits())]
        made += [dc for _, dc in others]
        for what, dc in others:
            rc, msg = raw(dc, 3, np.ascontiguousarray(init[:, :dc.d]), EUC, 2, dc.n)
            assert rc == _native.PMM_ERR_ARG and what in msg, (what, rc, msg)
            assert_same(f.kmeans(init, EUC, 2), want, f"after the {what} refusal")
        # argument refusals on a good handle, then it still serves
        for args, text in (((0, init, EUC, 1), "K must be >= 1"), ((301, np.zeros((301, 32), np.float32), EUC, 1), "<= n"),
                           ((3, init, _native.METRIC_DOT, 1), "dot product"), ((3, init, 7, 1), "metric"),
                           ((3, init, EUC, -1), "max_iter")):
            rc, msg = raw(f, args[0], args[1], args[2], args[3], 300)
            assert rc == _native.PMM_ERR_ARG and text in msg, (args[0], rc, msg)
        assert_same(f.kmeans(init, EUC, 2), want, "after the argument refusals")
        try:
            _native.set_devices([0, 0])
            two = _native.DeviceCorpus(x)
            made.append(two)
            assert two.shards == 2
            assert raw(two, 3, init, EUC, 1, 300)[0] == _native.PMM_ERR_UNSUPPORTED
        finally:
            _native.set_devices([])
    finally:
        for dc in made:
            dc.close()


def test_multivector_handle_clusters_its_tokens():
    x, _, _ = kc.planted(500, 33, 4, 6)
    offs = np.arange(0, 501, 5, dtype=np.int64)
    init = kc.default_init(x, 4, 6)
    mv = _native.DeviceCorpus.multivector(x, offs)
    try:
        assert_same(mv.kmeans(init, COS, 3), kc.kmeans_ref(x, init, COS, 3), "multi-vector")
    finally:
        mv.close()


# ---- 5. scratch ----
def test_same_bits_on_poisoned_scratch_and_between_guard_bands(monkeypatch):
    d, K, n = 33, 5, 1500
    for metric in (EUC, COS):
        x, _, _ = kc.planted(n, d, K, 8, noise=2.0)
        if metric == COS:
            x[3, 2] = np.inf  # (a row in no cluster: the sort's last key)
        init = kc.default_init(x, K, 8)
        dc = _native.DeviceCorpus(x)
        try:
            want = kc.kmeans_ref(x, init, metric, 3)
            assert (want[1][3] == NO_GROUP) == (metric == COS)
            for poison in ("0xFF", "0x7F", "0x01"):
                monkeypatch.setenv("PMM_ARENA_POISON", poison)
                assert_same(dc.kmeans(init, metric, 3), want, f"{NAME[metric]} poison {poison}")
            monkeypatch.delenv("PMM_ARENA_POISON")
            G = 1024
            bufs = [np.full(m + 2 * G, 0xA5A5A5A5, dtype=np.uint32) for m in (K * d, n, n)]
            cent = bufs[0][G:G + K * d].view(np.float32).reshape(K, d)
            labels = bufs[1][G:G + n]
            sc = bufs[2][G:G + n].view(np.float32)
            up, cv = ctypes.c_int64(-1), ctypes.c_int(-1)
            rc = _native.lib().pmm_kmeans_f32_corpus(dc._h, K, _native.ptr(init), metric, 3, _native.ptr(cent),
                                                     _native.ptr(labels), _native.ptr(sc), ctypes.byref(up),
                                                     ctypes.byref(cv))
            assert rc == _native.PMM_OK, _native.last_error()
            assert_same((cent, labels, sc, up.value, cv.value), want, "guarded outputs")
            for b, m in zip(bufs, (K * d, n, n)):
                assert (b[:G] == 0xA5A5A5A5).all() and (b[G + m:] == 0xA5A5A5A5).all()
        finally:
            dc.close()


# ---- 6. the Python surface ----
NS_SCRIPT = r'''
import json, sys, types
sys.path.insert(0, %(pkg)r)
pl = types.ModuleType("polars")
class _DT:
    def __init__(self, name, *args):
        self.name, self.args = name, args
pl.UInt32, pl.Float32, pl.Float64 = _DT("UInt32"), _DT("Float32"), _DT("Float64")
pl.List = lambda inner: _DT("List", inner)
pl.Struct = lambda fields: _DT("Struct", tuple(fields.items()))
pl.Array = lambda inner, n: _DT("Array", inner, n)
class Expr:
    def __init__(self):
        self.calls = []
    def map_batches(self, fn, **kw):
        self.calls.append((fn, kw))
        return ("mapped", kw)
class Series:
    pass
registry = {}
def register_expr_namespace(name):
    def deco(cls):
        registry[name] = cls
        return cls
    return deco
pl.Expr, pl.Series = Expr, Series
pl.api = types.SimpleNamespace(register_expr_namespace=register_expr_namespace)
sys.modules["polars"] = pl

import numpy as np, pyarrow as pa
import polars_matmul
x = np.load(%(rows)r)
e = Expr(); polars_matmul.PmmNamespace(e).kmeans(%(K)d, %(metric)r, %(max_iter)d, seed=%(seed)d)
fn, kw = e.calls[0]
col = pa.FixedSizeListArray.from_arrays(pa.array(x.reshape(-1)), x.shape[1])
out = fn(col)
print(json.dumps({"elementwise": kw["is_elementwise"], "dtype": kw["return_dtype"].name, "labels": out.to_pylist()}))
'''


def test_every_entry_returns_the_same_labels_and_a_cached_column_uploads_nothing(monkeypatch, tmp_path):
    d, K, n, seed = 256, 7, 1100, 3  # 1.1 MiB of rows: cacheable
    x, _, _ = kc.planted(n, d, K, 12, noise=2.0)
    init = kc.default_init(x, K, seed)
    want = kc.kmeans_ref(x, init, EUC, 4)
    assert_same(run(x, init, EUC, 4), want, "_native")
    col = pa.FixedSizeListArray.from_arrays(pa.array(x.reshape(-1)), d)
    pm.clear_corpus_cache()
    try:
        monkeypatch.setattr(pm, "_CACHE_ON", True)
        assert_same(polars_matmul.kmeans(x, K, "euclidean", 4, seed=seed), want, "polars_matmul.kmeans, seed")
        assert_same(polars_matmul.kmeans(x, K, "euclidean", 4, init=init), want, "polars_matmul.kmeans, matrix")
        ids = np.sort(np.random.RandomState(seed).choice(n, K, replace=False))
        assert_same(polars_matmul.kmeans(x, K, "l2", 4, init=ids), want, "polars_matmul.kmeans, row ids")
        pm.clear_corpus_cache()

        def h2d(fn):
            _native.timing_enable(True)
            _native.timing_reset()
            try:
                return fn(), _native.timing_read("h2d")[1]
            finally:
                _native.timing_reset()
                _native.timing_enable(False)

        # a column that is already a cached top-k corpus: k-means uploads its K centroids and nothing else
        pm._topk(pa.FixedSizeListArray.from_arrays(pa.array(x[:3].reshape(-1)), d), col, 2, "euclidean")
        assert len(pm._cache) == 1
        got, uploads = h2d(lambda: pm._kmeans(col, K, "euclidean", 4, seed=seed))
        assert_same(got, want, "_kmeans on the cached column")
        assert uploads == 1 and len(pm._cache) == 1, uploads
        got, uploads = h2d(lambda: pm._kmeans(col, K, "euclidean", 4, init=init))
        assert_same(got, want, "_kmeans again")
        assert uploads == 1, uploads
        labels = pm._kmeans_labels(col, K, "euclidean", 4, seed=seed)
        assert labels.null_count == 0 and np.array_equal(np.asarray(labels.to_numpy()), want[1])
    finally:
        pm.clear_corpus_cache()
    # .pmm.kmeans against the stand-in polars of tests/test_namespace.py, in a process of its own
    rows = str(tmp_path / "rows.npy")
    np.save(rows, x)
    script = NS_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd"), "rows": rows, "K": K, "metric": "euclidean",
                          "max_iter": 4, "seed": seed}
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["elementwise"] is False and out["dtype"] == "UInt32"
    assert out["labels"] == [int(v) for v in want[1]]
