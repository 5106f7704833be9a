"""CPU side of k-means (pmm_kmeans_f32_corpus, DeviceCorpus.kmeans,
``polars_matmul.kmeans``, ``_kmeans``, ``.pmm.kmeans``): the restatement of
tests/kmeans_cases.py on its own, the piece rule's visibility, the header and
bindings, every refusal before any library call, the namespace (against a
stand-in ``polars`` in a subprocess, as tests/test_bits_cpu.py) and the new
kernels' resources (hipcc cross-compiles gfx950 here)."""
from __future__ import annotations

import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pyarrow as pa
import pytest

import kmeans_cases as kc
import polars_matmul
from isa_util import CSRC, FLAGS, HIPCC, have_hipcc
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- the restatement ----
def test_restatement_recovers_a_planted_partition():
    rs = np.random.RandomState(0)
    mu = np.array([[10.0] * 8, [-10.0] * 8, [10.0, -10.0] * 4], dtype=np.float32)
    truth = (np.arange(300) % 3).astype(np.uint32)
    x = (mu[truth] + 0.5 * rs.randn(300, 8)).astype(np.float32)
    for metric in (kc.EUC, kc.COS):
        c, labels, scores, updates, converged, changes = kc.kmeans_ref(x, x[[0, 1, 2]], metric, 25)
        assert converged and 1 <= updates < 25 and changes[-1] == 0
        assert np.array_equal(labels, truth)  # (row r starts cluster r: the planted numbering)
        assert scores.dtype == np.float32 and labels.dtype == np.uint32
        if metric == kc.EUC:
            assert np.abs(c - mu).max() < 0.2
    # max_iter = 0 is the pure assignment against the initial centroids
    c, labels, _, updates, converged, _ = kc.kmeans_ref(x, mu, kc.EUC, 0)
    assert updates == 0 and not converged and np.array_equal(bits(c), bits(mu)) and np.array_equal(labels, truth)


def test_piece_order_is_visible_in_the_bits():
    # 513 members of one cluster: +2^54, 511 ones, -2^54.  In pieces of 256 the
    # second piece's 256 ones are summed on their own and survive; one running
    # sum loses every one of them to 2^54's rounding.
    x = np.ones((513, 2), dtype=np.float32)
    x[0, 0], x[512, 0] = kc.BIG, -kc.BIG
    members = np.arange(513)
    two, n2 = kc.cluster_sum(x, members, None)
    one, n1 = kc.cluster_sum(x, members, None, piece=None)
    assert n1 == n2 == 513
    assert two[0] == 256.0 and one[0] == 0.0 and two[1] == one[1] == 513.0
    assert bits(two)[0] != bits(one)[0]
    # interleaved magnitudes, as the GPU test's rows: the f32 centroids differ too
    xe, init = kc.piece_edge_rows()
    a, b = kc.kmeans_ref(xe, init, kc.EUC, 1), kc.kmeans_ref(xe, init, kc.EUC, 1, piece=None)
    assert tuple(np.bincount(a[1])) == (255, 256, 257, 512, 513)
    assert not np.array_equal(bits(a[0]), bits(b[0]))
    assert np.array_equal(bits(a[0][:2]), bits(b[0][:2]))  # one piece: the same sum


def test_zero_norm_members_keep_their_place_and_are_not_counted():
    x = np.ones((4, 2), dtype=np.float32)
    x[1] = 0.0
    norms = kc.oracle.norms(x)
    total, count = kc.cluster_sum(x, np.arange(4), norms)
    assert count == 3 and np.allclose(total, 3 / np.sqrt(2.0))
    lab = np.zeros(4, dtype=np.uint32)
    lab[3] = kc.NO_GROUP
    c = kc.update(x, lab, np.full((2, 2), 7.0, dtype=np.float32), kc.COS, norms)
    assert np.array_equal(bits(c[1]), bits(np.full(2, 7.0, dtype=np.float32)))  # an empty cluster keeps its bits
    assert np.allclose(c[0], 1 / np.sqrt(2.0))  # rows 0 and 2: row 1 is not counted, row 3 is in no cluster


# ---- header and bindings ----
def test_entry_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    m = re.search(r"\bint pmm_kmeans_f32_corpus\s*\(([^;]*)\)\s*;", text)
    assert m, "pmm_kmeans_f32_corpus not declared in include/pmm.h"
    assert len(m.group(1).split(",")) == 10
    assert "pmm_kmeans_f32_corpus" in _native.EXPORTED_SYMBOLS
    fn = _native.lib().pmm_kmeans_f32_corpus
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    assert hasattr(_native.DeviceCorpus, "kmeans")
    for name in ("kmeans", "_kmeans"):
        assert hasattr(polars_matmul, name)
    assert "kmeans" in polars_matmul.__all__
    # the piece length: one constant, stated in both headers and in the restatement
    internal = open(os.path.join(CSRC, "pmm_internal.h")).read()
    a = re.search(r"constexpr int kKmeansPiece = (\d+);", internal)
    b = re.search(r"#define PMM_KMEANS_PIECE (\d+)", text)
    assert a and b and int(a.group(1)) == int(b.group(1)) == kc.P == 256
    assert len(re.findall(r"kKmeansPiece = ", internal)) == 1
    assert "csrc/pmm_kmeans.hip" in open(os.path.join(ROOT, "polars-matmul_amd", "Makefile")).read()


def test_host_refusals_touch_no_device():
    import ctypes

    L = _native.lib()
    up, cv = ctypes.c_int64(0), ctypes.c_int(0)
    buf = np.zeros(8, dtype=np.float32)
    lab = np.zeros(8, dtype=np.uint32)
    p = _native.ptr
    assert L.pmm_kmeans_f32_corpus(None, 1, p(buf), 2, 1, p(buf), p(lab), None, ctypes.byref(up),
                                   ctypes.byref(cv)) == _native.PMM_ERR_ARG
    assert _native.last_error() == "null corpus"
    # with a (never read) handle: every argument error comes before the handle is looked at
    fake = ctypes.c_void_p(8)
    for args, text in (((1, None, 2, 1, p(buf), p(lab)), "null argument"), ((1, p(buf), 2, 1, None, p(lab)), "null argument"),
                       ((1, p(buf), 2, 1, p(buf), None), "null argument"), ((0, p(buf), 2, 1, p(buf), p(lab)), "K must be >= 1"),
                       ((1 << 32, p(buf), 2, 1, p(buf), p(lab)), "K out of range"),
                       ((1, p(buf), 2, -1, p(buf), p(lab)), "max_iter must be >= 0"),
                       ((1, p(buf), 1, 1, p(buf), p(lab)), "does not maximise a dot product"),
                       ((1, p(buf), 9, 1, p(buf), p(lab)), "invalid metric id 9")):
        K, init, metric, it, oc, ol = args
        rc = L.pmm_kmeans_f32_corpus(fake, K, init, metric, it, oc, ol, None, ctypes.byref(up), ctypes.byref(cv))
        assert rc == _native.PMM_ERR_ARG and text in _native.last_error(), (text, rc, _native.last_error())


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library or of a device helper fails the test."""

    def boom(*a, **k):
        raise AssertionError("library call before the k-means checks")

    for name in ("lib", "topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str",
                 "device_count", "set_devices"):
        monkeypatch.setattr(_native, name, boom)
    return monkeypatch


X = np.zeros((6, 4), dtype=np.float32)


def col(x, dtype=pa.float32()):
    return pa.FixedSizeListArray.from_arrays(pa.array(x.reshape(-1), type=dtype), x.shape[1])


def test_python_refusals_come_before_any_library_call(no_library):
    for fn, rows in ((polars_matmul.kmeans, X), (pm._kmeans, X), (pm._kmeans, col(X)), (pm._kmeans_labels, col(X))):
        with pytest.raises(ValueError, match="does not maximise a dot product"):
            fn(rows, 2, "dot")
        with pytest.raises(ValueError, match="Unknown metric"):
            fn(rows, 2, "manhattan")
        with pytest.raises(TypeError, match="cannot be converted to 'PyString'"):
            fn(rows, 2, 2)
        with pytest.raises(TypeError, match=r"compute='bf16' has no k-means"):
            fn(rows, 2, "cosine", compute="bf16")
        with pytest.raises(ValueError, match="n_clusters must be >= 1"):
            fn(rows, 0)
        with pytest.raises(ValueError, match=r"n_clusters \(7\) must be <= the rows of the column \(6\)"):
            fn(rows, 7)
        with pytest.raises(TypeError, match="cannot be interpreted as an integer"):
            fn(rows, 2.5)
        with pytest.raises(OverflowError):
            fn(rows, 2, "euclidean", -1)
        with pytest.raises(TypeError, match="cannot be interpreted as an integer"):
            fn(rows, 2, "euclidean", 2.0)
        with pytest.raises(ValueError, match=r"init has shape \(3, 4\)"):
            fn(rows, 2, init=np.zeros((3, 4), dtype=np.float32))
        with pytest.raises(ValueError, match=r"init has shape \(2, 5\)"):
            fn(rows, 2, init=np.zeros((2, 5), dtype=np.float32))
        with pytest.raises(TypeError, match="must hold floats"):
            fn(rows, 2, init=np.zeros((2, 4), dtype=np.int32))
        with pytest.raises(ValueError, match="holds 3 row ids, n_clusters is 2"):
            fn(rows, 2, init=np.array([0, 1, 2]))
        with pytest.raises(ValueError, match=r"row id 6: not a row of the column \(6 rows\)"):
            fn(rows, 2, init=np.array([0, 6]))
        with pytest.raises(ValueError, match="row id twice"):
            fn(rows, 2, init=np.array([3, 3]))
        with pytest.raises(TypeError, match="init must be"):
            fn(rows, 2, init="random")
        with pytest.raises(TypeError, match="seed must be an integer"):
            fn(rows, 2, seed=1.5)
    # Float32 only, in the style of the MaxSim refusals
    for bad in (X.astype(np.float64), X.astype(np.int8)):
        with pytest.raises(TypeError, match="k-means runs on Float32 columns"):
            polars_matmul.kmeans(bad, 2)
        with pytest.raises(TypeError, match="k-means runs on Float32 columns"):
            pm._kmeans(bad, 2)
    for dtype in (pa.float64(), pa.int8()):
        with pytest.raises(TypeError, match="k-means runs on Float32 columns"):
            pm._kmeans(col(X.astype(dtype.to_pandas_dtype()), dtype), 2)
    with pytest.raises(TypeError, match="2-D array"):
        polars_matmul.kmeans(np.zeros(4, dtype=np.float32), 2)
    with pytest.raises(RuntimeError, match="Empty series"):
        pm._kmeans(np.zeros((0, 4), dtype=np.float32), 1)


class StubCorpus:
    """Records the call; answers like a handle of its rows."""

    calls = []

    def __init__(self, c, compute="f32"):
        self.c, self.n, self.d = c, c.shape[0], c.shape[1]

    def acquire(self):
        return self

    def release(self):
        pass

    def close(self):
        pass

    def kmeans(self, init, metric, max_iter):
        StubCorpus.calls.append((np.array(init), metric, max_iter))
        labels = np.zeros(self.n, dtype=np.uint32)
        labels[-1] = _native.NO_GROUP
        return init, labels, np.zeros(self.n, dtype=np.float32), 1, True


@pytest.fixture
def stubbed(monkeypatch):
    StubCorpus.calls = []
    monkeypatch.setattr(_native, "DeviceCorpus", StubCorpus)
    monkeypatch.setattr(_native, "get_devices", lambda: [])
    monkeypatch.setattr(pm, "_devices_env_done", True)
    monkeypatch.setattr(pm, "_CACHE_ON", False)
    return monkeypatch


def test_init_forms_and_the_label_column(stubbed):
    x = np.arange(40, dtype=np.float32).reshape(10, 4)
    polars_matmul.kmeans(x, 3, seed=5)
    ids = np.sort(np.random.RandomState(5).choice(10, 3, replace=False))
    assert np.array_equal(StubCorpus.calls[-1][0], x[ids]) and StubCorpus.calls[-1][1:] == (_native.METRIC_EUCLIDEAN, 25)
    polars_matmul.kmeans(x, 3, "cosine", 7, init=np.array([9, 0, 4]))
    assert np.array_equal(StubCorpus.calls[-1][0], x[[9, 0, 4]]) and StubCorpus.calls[-1][1:] == (_native.METRIC_COSINE, 7)
    m = np.ones((3, 4), dtype=np.float64)
    pm._kmeans(col(x), 3, "l2", 0, init=m)
    assert StubCorpus.calls[-1][0].dtype == np.float32 and np.array_equal(StubCorpus.calls[-1][0], m)
    assert StubCorpus.calls[-1][1:] == (_native.METRIC_EUCLIDEAN, 0)
    out = pm._kmeans_labels(col(x), 3)
    assert out.type == pa.uint32() and out.to_pylist() == [0] * 9 + [None]


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

import polars_matmul
ns = registry["pmm"]
calls = []
polars_matmul._kmeans_labels = lambda s, *a: calls.append(["kmeans", s, *a]) or "labels"
out = {}
e = Expr(); ns(e).kmeans(8, "cosine", 3, init=None, seed=4)
fn, kw = e.calls[0]
out["kw"] = {"is_elementwise": kw["is_elementwise"], "dtype": kw["return_dtype"].name}
out["result"] = fn("batch")
out["call"] = calls[-1]
out["errors"] = []
for args, kwargs in ((("dot",), {}), (("euclidean",), {"compute": "bf16"})):
    try:
        ns(Expr()).kmeans(8, *args, **kwargs)
        out["errors"].append(None)
    except (TypeError, ValueError) as err:
        out["errors"].append(type(err).__name__ + ": " + str(err))
print(json.dumps(out))
'''


def test_namespace_method_against_the_stub_polars():
    pkg = os.path.join(ROOT, "polars-matmul_amd")
    r = subprocess.run([sys.executable, "-c", NS_SCRIPT % {"pkg": pkg}], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["kw"] == {"is_elementwise": False, "dtype": "UInt32"}
    assert out["result"] == "labels" and out["call"] == ["kmeans", "batch", 8, "cosine", 3, None, 4]
    assert out["errors"][0].startswith("ValueError") and "dot product" in out["errors"][0]
    assert out["errors"][1].startswith("TypeError") and "has no k-means" in out["errors"][1]


# ---- code generation (after tests/test_bits_cpu.py) ----
def test_kmeans_kernels_compile_without_scratch():
    from test_kernel_resources import scratch_by_kernel

    if not have_hipcc():
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kmeans.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_kmeans.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = scratch_by_kernel(asm)
    for want in ("kmeans_labels_kernel", "kmeans_sort_hist_kernel", "kmeans_scan_kernel", "kmeans_sort_scatter_kernel",
                 "kmeans_bounds_kernel", "kmeans_pieces_kernel", "kmeans_update_kernel", "kmeans_finish_kernel"):
        hits = {k: v for k, v in sc.items() if want in k}
        assert hits, f"{want} not in pmm_kmeans.hip's assembly: {sorted(sc)}"
        assert set(hits.values()) == {(0, 0)}, f"scratch (bytes, instructions): {hits}"
    assert len([k for k in sc if "kmeans_update_kernel" in k]) == 2  # euclidean and cosine
    # the update adds in f64 and holds no global atomic: its sums cannot depend on the launch geometry
    assert "v_add_f64" in asm and "global_atomic" not in asm
