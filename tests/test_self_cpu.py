"""CPU side of self search (pmm_range_f32_self, pmm_topk_f32_self,
``within_self`` / ``topk_self`` and their Arrow and namespace forms): the C
entries' argument checks, which all come before the handle is read; the Python
entries' refusals, before any library call; the namespace against a stand-in
``polars`` in a subprocess; and the symmetry of the exact score, on the oracle."""
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

import self_cases as sc_
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_self_entries_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    for name in ("pmm_range_f32_self", "pmm_topk_f32_self", "pmm_range_self_plan"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _native.EXPORTED_SYMBOLS
        assert getattr(_native.lib(), name).argtypes is not None


# A stand-in for a corpus handle: never read, because every call below fails an
# argument check first.
_FAKE = ctypes.create_string_buffer(4096)
_OFF = np.zeros(8, dtype=np.int64)
_IDX = np.zeros(8, dtype=np.uint32)
_SC = np.zeros(8, dtype=np.float32)


def _p(a):
    return None if a is None else (ctypes.cast(a, ctypes.c_void_p) if a is _FAKE else _native.ptr(a))


def _range(corpus=_FAKE, threshold=0.5, metric=_native.METRIC_COSINE, cap=8, offsets=_OFF, idx=_IDX, sc=_SC,
           total=True):
    tot = ctypes.c_int64(-7)
    rc = _native.lib().pmm_range_f32_self(_p(corpus), threshold, metric, cap, _p(offsets), _p(idx), _p(sc),
                                          ctypes.byref(tot) if total else None)
    return rc, _native.last_error()


def _topk(corpus=_FAKE, k=2, metric=_native.METRIC_COSINE, idx=_IDX, sc=_SC):
    rc = _native.lib().pmm_topk_f32_self(_p(corpus), k, metric, _p(idx), _p(sc))
    return rc, _native.last_error()


@pytest.mark.parametrize("bad", [
    dict(corpus=None), dict(offsets=None), dict(total=False), dict(idx=None), dict(sc=None),
    dict(threshold=float("nan")), dict(cap=-1), dict(metric=3), dict(metric=-1),
])
def test_range_argument_errors_come_before_the_handle_is_read(bad):
    rc, msg = _range(**bad)
    assert rc == _native.PMM_ERR_ARG and msg, (bad, rc, msg)
    if "threshold" in bad:
        assert "NaN" in msg


@pytest.mark.parametrize("bad", [dict(corpus=None), dict(idx=None), dict(sc=None), dict(k=0), dict(k=-3),
                                 dict(metric=3)])
def test_topk_argument_errors_come_before_the_handle_is_read(bad):
    rc, msg = _topk(**bad)
    assert rc == _native.PMM_ERR_ARG and msg, (bad, rc, msg)


# ---- the Python entries' refusals ----
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library or of a device helper fails the test."""

    def boom(*a, **k):
        raise AssertionError("library call before the argument check")

    for name in ("lib", "topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str",
                 "device_count", "set_devices"):
        monkeypatch.setattr(_native, name, boom)
    return monkeypatch


C32 = np.zeros((6, 4), dtype=np.float32)
C64 = np.zeros((6, 4), dtype=np.float64)
I8 = np.zeros((6, 4), dtype=np.int8)
REFUSAL = r"self search runs on Float32 columns.*cast"


def test_other_dtypes_are_refused_with_the_cast(no_library):
    import polars_matmul

    for col in (C64, I8, pa.array([[1.0, 0.0]], type=pa.list_(pa.float64())),
                pa.array([[1, 0]], type=pa.list_(pa.int8()))):
        with pytest.raises(TypeError, match=REFUSAL):
            pm._within_self(col, 0.5, "cosine")
        with pytest.raises(TypeError, match=REFUSAL):
            pm._topk_self(col, 2, "cosine")
    for col in (C64, I8):
        with pytest.raises(TypeError, match=REFUSAL):
            polars_matmul.within_self(col, 0.5)
        with pytest.raises(TypeError, match=REFUSAL):
            polars_matmul.topk_self(col, 2)


def test_bf16_compute_is_refused(no_library):
    import polars_matmul

    with pytest.raises(TypeError, match=REFUSAL):
        polars_matmul.within_self(C32, 0.5, compute="bf16")
    with pytest.raises(TypeError, match=REFUSAL):
        polars_matmul.topk_self(C32, 2, compute="bf16")
    with pytest.raises(ValueError, match="compute must be"):
        polars_matmul.topk_self(C32, 2, compute="fp8")


def test_threshold_metric_and_shape(no_library):
    import polars_matmul

    with pytest.raises(ValueError, match="NaN"):
        pm._within_self(C32, float("nan"), "cosine")
    with pytest.raises(ValueError, match="NaN"):
        polars_matmul.within_self(C32, float("nan"))
    with pytest.raises(TypeError, match="threshold must be a number"):
        pm._within_self(C32, "0.5", "cosine")
    with pytest.raises(TypeError, match="PyString"):
        pm._within_self(C32, 0.5, 0)
    with pytest.raises(TypeError, match="PyString"):
        pm._topk_self(C32, 2, 0)
    for bad in (np.zeros(4, np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(TypeError, match="2-D"):
            polars_matmul.within_self(bad, 0.5)
        with pytest.raises(TypeError, match="2-D"):
            polars_matmul.topk_self(bad, 2)


def test_an_empty_column_is_an_empty_list_column(no_library):
    empty = pa.array([], type=pa.list_(pa.float32()))
    for out in (pm._within_self(empty, 0.5, "cosine"), pm._topk_self(empty, 3, "cosine")):
        assert len(out) == 0 and out.type == pa.large_list(pm._TOPK_STRUCT)


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
calls = []
polars_matmul._within_self = lambda *a, **k: calls.append(("within_self", a, k)) or "within-self-result"
polars_matmul._topk_self = lambda *a, **k: calls.append(("topk_self", a, k)) or "topk-self-result"
ns = registry["pmm"]
want_dtype = pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64}))
out = {}
column = object()
e = Expr(); r = ns(e).within_self(0.9)
fn, kw = e.calls[0]
out["within_kw"] = [r[0], kw["is_elementwise"], kw["return_dtype"] == want_dtype, sorted(kw)]
out["within_r"] = fn(column)
name, a, k2 = calls[-1]
out["within_call"] = [name, a[0] is column, list(a[1:]), k2]
e = Expr(); ns(e).within_self(1.5, metric="euclidean"); e.calls[0][0](column)
out["within_call2"] = [calls[-1][0], list(calls[-1][1][1:])]
e = Expr(); r = ns(e).topk_self(5)
fn, kw = e.calls[0]
out["topk_kw"] = [r[0], kw["is_elementwise"], kw["return_dtype"] == want_dtype, sorted(kw)]
out["topk_r"] = fn(column)
name, a, k2 = calls[-1]
out["topk_call"] = [name, a[0] is column, list(a[1:]), k2]
e = Expr(); ns(e).topk_self(k=3, metric="dot"); e.calls[0][0](column)
out["topk_call2"] = [calls[-1][0], list(calls[-1][1][1:])]
for meth, args in (("within_self", (0.5,)), ("topk_self", (2,))):
    try:
        getattr(ns(Expr()), meth)(*args, compute="bf16")
        out[meth + "_bf16"] = None
    except TypeError as err:
        out[meth + "_bf16"] = str(err)
print(json.dumps(out))
'''


def test_namespace_self_map_batches_contract():
    code = NAMESPACE_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    # a row's list depends on the whole column: not elementwise; the dtype is topk's
    assert out["within_kw"] == ["mapped", False, True, ["is_elementwise", "return_dtype"]]
    assert out["topk_kw"] == ["mapped", False, True, ["is_elementwise", "return_dtype"]]
    assert out["within_r"] == "within-self-result" and out["topk_r"] == "topk-self-result"
    # the column itself is the corpus: it is the one Series handed on
    assert out["within_call"] == ["within_self", True, [0.9, "cosine"], {}]
    assert out["within_call2"] == ["within_self", [1.5, "euclidean"]]
    assert out["topk_call"] == ["topk_self", True, [5, "cosine"], {}]
    assert out["topk_call2"] == ["topk_self", [3, "dot"]]
    assert "self search runs on Float32 columns" in out["within_self_bf16"]
    assert "self search runs on Float32 columns" in out["topk_self_bf16"]


# ---- symmetry: the dropped (j, i) has the kept (i, j)'s score bits ----
# exact_score joins the two norms by one commutative IEEE operation (cosine: their
# product, euclidean: the sum of the squared norms; dot reads none) and the chain
# multiplies the same pairs in the same K order, so it holds for all three
# metrics.  Checked on the oracle, which the device matches bit for bit.
@pytest.mark.parametrize("metric", [sc_.COS, sc_.DOT, sc_.EUC])
def test_scores_are_symmetric_on_the_oracle(metric):
    c = sc_.ragged_column(metric)
    n = c.shape[0]
    oi, osc = sc_.ranked_self(c, metric)
    s = np.empty((n, n), dtype=np.float32)
    s[np.arange(n)[:, None], oi.astype(np.int64)] = osc
    assert np.isfinite(s).all()
    assert np.array_equal(s.view(np.uint32), s.T.view(np.uint32)), sc_.NAME[metric]
