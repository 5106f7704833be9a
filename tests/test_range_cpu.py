"""CPU side of range search (pmm_range_f32_corpus, ``DeviceCorpus.range``,
``within`` / ``_within`` / ``.pmm.within``): the C entry's argument checks,
which all come before the handle is read or a device touched; the Arrow
assembly from CSR arrays; the namespace against a stand-in ``polars`` in a
subprocess (as tests/test_namespace.py drives ``topk``); and the Float64 /
compute="bf16" refusals, before any library call."""
from __future__ import annotations

import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_entry_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    assert re.search(r"\bint pmm_range_f32_corpus\s*\(", text)
    assert "pmm_range_f32_corpus" in _native.EXPORTED_SYMBOLS
    assert _native.lib().pmm_range_f32_corpus.argtypes is not None


# A stand-in for a corpus handle: never read, because every call below fails an
# argument check first (the checks come before the handle is dereferenced).
_FAKE = ctypes.create_string_buffer(4096)
_Q = np.zeros((2, 4), dtype=np.float32)
_OFF = np.zeros(3, dtype=np.int64)
_IDX = np.zeros(8, dtype=np.uint32)
_SC = np.zeros(8, dtype=np.float32)


def _call(corpus=_FAKE, q=_Q, m=2, threshold=0.5, metric=_native.METRIC_COSINE, cap=8, offsets=_OFF, idx=_IDX,
          sc=_SC, total=True):
    tot = ctypes.c_int64(-7)
    p = lambda a: None if a is None else (ctypes.cast(a, ctypes.c_void_p) if a is _FAKE else _native.ptr(a))
    rc = _native.lib().pmm_range_f32_corpus(p(corpus), p(q), m, threshold, metric, cap, p(offsets), p(idx), p(sc),
                                            ctypes.byref(tot) if total else None)
    return rc, _native.last_error()


@pytest.mark.parametrize("bad", [
    dict(corpus=None), dict(q=None), dict(offsets=None), dict(total=False),
    dict(idx=None), dict(sc=None),  # (with cap > 0: the lists need their buffers)
    dict(threshold=float("nan")), dict(cap=-1), dict(m=-1), dict(metric=3), dict(metric=-1),
])
def test_argument_errors_come_before_any_device_call(bad):
    rc, msg = _call(**bad)
    assert rc == _native.PMM_ERR_ARG, (bad, rc, msg)
    assert msg, bad


def test_nan_threshold_message_names_the_threshold():
    rc, msg = _call(threshold=float("nan"))
    assert rc == _native.PMM_ERR_ARG and "NaN" in msg


# ---- _within's Arrow assembly ----
def test_csr_arrow_assembly_with_empty_rows():
    offsets = np.array([0, 2, 2, 5, 5], dtype=np.int64)
    idx = np.array([7, 3, 1, 0, 4], dtype=np.uint32)
    sc = np.array([0.75, 0.5, 1.0, -0.0, 0.25], dtype=np.float32)
    arr = pm._csr_arrow(offsets, idx, sc)
    assert arr.type == pa.large_list(pm._TOPK_STRUCT)
    assert len(arr) == 4
    got = arr.to_pylist()
    assert got[0] == [{"index": 7, "score": 0.75}, {"index": 3, "score": 0.5}]
    assert got[1] == [] and got[3] == []
    assert [e["index"] for e in got[2]] == [1, 0, 4]
    scores = arr.values.field("score")
    assert scores.type == pa.float64()
    # widened, not re-rounded: the f64 holds the f32's value (and -0.0 its sign)
    assert np.array_equal(scores.to_numpy().view(np.uint64), sc.astype(np.float64).view(np.uint64))
    assert arr.values.field("index").type == pa.uint32()


def test_csr_arrow_assembly_of_no_rows():
    arr = pm._csr_arrow(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    assert len(arr) == 0 and arr.type == pa.large_list(pm._TOPK_STRUCT)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library or of a device helper fails the test."""

    def boom(*a, **k):
        raise AssertionError("library call before the argument check")

    for name in ("lib", "topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str",
                 "device_count", "set_devices"):
        monkeypatch.setattr(_native, name, boom)
    return monkeypatch


def test_within_of_no_query_rows_is_an_empty_list_column(no_library):
    left = pa.array([], type=pa.list_(pa.float32()))
    right = pa.array([[1.0, 0.0]], type=pa.list_(pa.float32()))
    out = pm._within(left, right, 0.5, "cosine")
    assert len(out) == 0 and out.type == pa.large_list(pm._TOPK_STRUCT)


# ---- the refusals ----
C32 = np.zeros((6, 4), dtype=np.float32)
C64 = np.zeros((6, 4), dtype=np.float64)


def test_float64_columns_are_refused_with_the_cast(no_library):
    import polars_matmul

    for left, right in ((C64[:2], C64), (C32[:2], C64), (C64[:2], C32),
                        (pa.array([[1.0, 0.0]], type=pa.list_(pa.float64())),
                         pa.array([[1.0, 0.0]], type=pa.list_(pa.float32())))):
        with pytest.raises(TypeError, match=r"range search runs on Float32 columns.*cast") as ei:
            pm._within(left, right, 0.5, "cosine")
        assert "Float32" in str(ei.value)
    with pytest.raises(TypeError, match=r"range search runs on Float32 columns.*cast"):
        polars_matmul.within(C64[:2], C64, 0.5)


def test_bf16_compute_is_refused(no_library):
    import polars_matmul

    with pytest.raises(TypeError, match=r"range search runs on Float32 columns.*cast"):
        pm._within(C32[:2], C32, 0.5, "cosine", compute="bf16")
    with pytest.raises(TypeError, match=r"range search runs on Float32 columns.*cast"):
        polars_matmul.within(C32[:2], C32, 0.5, compute="bf16")
    with pytest.raises(ValueError, match="compute must be"):
        pm._within(C32[:2], C32, 0.5, "cosine", compute="fp8")


def test_threshold_and_metric_types(no_library):
    with pytest.raises(ValueError, match="NaN"):
        pm._within(C32[:2], C32, float("nan"), "cosine")
    with pytest.raises(TypeError, match="threshold must be a number"):
        pm._within(C32[:2], C32, "0.5", "cosine")
    with pytest.raises(TypeError, match="PyString"):
        pm._within(C32[:2], C32, 0.5, 0)


def test_within_takes_no_groups():
    with pytest.raises(TypeError):
        pm._within(C32[:2], C32, 0.5, "cosine", groups=(np.zeros(2), np.zeros(6)))


def test_subset_checks_come_before_any_library_call(no_library):
    with pytest.raises(ValueError, match="the corpus has 6"):
        pm._within(C32[:2], C32, 0.5, "cosine", subset=np.ones(5, bool))
    with pytest.raises(RuntimeError, match="Empty series"):
        pm._within(C32[:2], C32, 0.5, "cosine", subset=np.zeros(6, bool))


NAMESPACE_SCRIPT = r'''
import json, sys, types
sys.path.insert(0, %(pkg)r)
pl = types.ModuleType("polars")
pl.UInt32, pl.Float32, pl.Float64 = "u32", "f32", "f64"
pl.List = lambda inner: ("List", inner)
pl.Struct = lambda fields: ("Struct", tuple(fields.items()))
pl.Array = lambda inner, n: ("Array", inner, n)
class Expr:
    def __init__(self):
        self.calls = []
    def map_batches(self, fn, **kw):
        self.calls.append((fn, kw))
        return ("mapped", kw)
class Series:
    def __init__(self, values):
        self.values = values
    def __len__(self):
        return len(self.values)
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
calls = []
def rec(*args, **kw):
    calls.append((args, kw))
    return "within-result"
polars_matmul._within = rec
ns = registry["pmm"]
corpus = Series([[1.0, 0.0]] * 3)
mask = Series([True, False, True])
out = {}
e = Expr(); r = ns(e).within(corpus, 0.9)
fn, kw = e.calls[0]
out["mapped"] = r[0]
out["kw"] = [kw["is_elementwise"], kw["return_dtype"] == pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
             sorted(kw)]
out["r"] = fn("b0")
a, k2 = calls[-1]
out["default"] = [a[0], a[1] is corpus, list(a[2:]), k2]
e = Expr(); ns(e).within(corpus, 1.5, metric="euclidean", subset=mask); e.calls[0][0]("b1")
a, k2 = calls[-1]
out["subset"] = [a[0], a[1] is corpus, list(a[2:]), sorted(k2), k2.get("subset") is mask]
for name, args, kws in (("expr", (Expr(), 0.5), {}), ("subset_expr", (corpus, 0.5), {"subset": Expr()}),
                        ("bf16", (corpus, 0.5), {"compute": "bf16"}), ("by", (corpus, 0.5), {"by": "label"})):
    try:
        ns(Expr()).within(*args, **kws)
        out[name] = None
    except TypeError as err:
        out[name] = str(err)
print(json.dumps(out))
'''


def test_namespace_within_map_batches_contract():
    code = NAMESPACE_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mapped"] == "mapped"
    # the same map_batches arguments as topk: elementwise, List[Struct{index: u32, score: f64}]
    assert out["kw"] == [True, True, ["is_elementwise", "return_dtype"]]
    assert out["r"] == "within-result"
    assert out["default"] == ["b0", True, [0.9, "cosine"], {}]
    assert out["subset"] == ["b1", True, [1.5, "euclidean"], ["subset"], True]
    assert out["expr"].startswith("corpus must be a Polars Series, not an Expression.")
    assert out["subset_expr"].startswith("subset must be a Polars Series, not an Expression.")
    assert "range search runs on Float32 columns" in out["bf16"]
    assert out["by"] is not None  # by= / groups= is not accepted
