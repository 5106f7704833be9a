"""CPU side of duplicate groups (pmm_components_f32_self,
``duplicate_groups`` and its Arrow and namespace forms): the symbol in the
header and the binding tables; the C entry's argument checks, which come before
the handle is read; the Python entries' refusals, before any library call, with
self search's texts; the namespace against a stand-in ``polars`` in a
subprocess; and the truth helpers of tests/components_cases.py themselves."""
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

import components_cases as cc
import self_cases as sc_
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_components_entry_declared_and_bound():
    import polars_matmul

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    name = "pmm_components_f32_self"
    assert re.search(r"\bint %s\s*\(" % name, text)
    assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGS
    assert len(_native._SIGS[name][0]) == 6
    assert getattr(_native.lib(), name).argtypes is not None
    assert hasattr(_native.DeviceCorpus, "components_self")
    assert "duplicate_groups" in polars_matmul.__all__ and callable(polars_matmul.duplicate_groups)
    assert polars_matmul._duplicate_groups is pm._duplicate_groups


# A stand-in for a corpus handle: never read, because every call below fails an
# argument check first.
_FAKE = ctypes.create_string_buffer(4096)
_LAB = np.zeros(8, dtype=np.uint32)


def _components(corpus=_FAKE, threshold=0.5, metric=_native.METRIC_COSINE, components=True, pairs=True):
    nc, npairs = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _native.lib().pmm_components_f32_self(
        None if corpus is None else ctypes.cast(corpus, ctypes.c_void_p), threshold, metric, _native.ptr(_LAB),
        ctypes.byref(nc) if components else None, ctypes.byref(npairs) if pairs else None)
    return rc, _native.last_error(), nc.value, npairs.value


@pytest.mark.parametrize("bad", [dict(corpus=None), dict(components=False), dict(pairs=False),
                                 dict(threshold=float("nan")), dict(metric=3), dict(metric=-1)])
def test_argument_errors_come_before_the_handle_is_read(bad):
    rc, msg, nc, npairs = _components(**bad)
    assert rc == _native.PMM_ERR_ARG and msg, (bad, rc, msg)
    assert nc in (-7,) and npairs in (-7,)  # nothing written
    if "threshold" in bad:
        assert msg == "the range threshold is NaN"


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


def _raised(call):
    with pytest.raises(Exception) as ei:
        call()
    return type(ei.value), str(ei.value)


def test_other_dtypes_are_refused_with_self_searchs_text(no_library):
    import polars_matmul

    for col in (C64, I8, pa.array([[1.0, 0.0]], type=pa.list_(pa.float64())),
                pa.array([[1, 0]], type=pa.list_(pa.int8()))):
        with pytest.raises(TypeError, match=REFUSAL):
            pm._duplicate_groups(col, 0.5, "cosine")
        assert _raised(lambda: pm._duplicate_groups(col, 0.5, "cosine")) == \
            _raised(lambda: pm._within_self(col, 0.5, "cosine"))
    for col in (C64, I8):
        with pytest.raises(TypeError, match=REFUSAL):
            polars_matmul.duplicate_groups(col, 0.5)
        assert _raised(lambda: polars_matmul.duplicate_groups(col, 0.5)) == \
            _raised(lambda: polars_matmul.within_self(col, 0.5))


def test_compute_is_refused_as_self_search_refuses_it(no_library):
    import polars_matmul

    with pytest.raises(TypeError, match=REFUSAL):
        polars_matmul.duplicate_groups(C32, 0.5, compute="bf16")
    with pytest.raises(ValueError, match="compute must be"):
        polars_matmul.duplicate_groups(C32, 0.5, compute="fp8")
    for compute in ("bf16", "fp8"):
        assert _raised(lambda: polars_matmul.duplicate_groups(C32, 0.5, compute=compute)) == \
            _raised(lambda: polars_matmul.within_self(C32, 0.5, compute=compute))


def test_threshold_metric_and_shape(no_library):
    import polars_matmul

    with pytest.raises(ValueError, match="NaN"):
        pm._duplicate_groups(C32, float("nan"), "cosine")
    with pytest.raises(ValueError, match="NaN"):
        polars_matmul.duplicate_groups(C32, float("nan"))
    for bad in ("0.5", True, None):
        with pytest.raises(TypeError, match="threshold must be a number"):
            pm._duplicate_groups(C32, bad, "cosine")
        assert _raised(lambda: pm._duplicate_groups(C32, bad, "cosine")) == \
            _raised(lambda: pm._within_self(C32, bad, "cosine"))
    with pytest.raises(TypeError, match="PyString"):
        pm._duplicate_groups(C32, 0.5, 0)
    for bad in (np.zeros(4, np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(TypeError, match="2-D"):
            polars_matmul.duplicate_groups(bad, 0.5)


def test_an_empty_column_is_an_empty_uint32_column(no_library):
    out = pm._duplicate_groups(pa.array([], type=pa.list_(pa.float32())), 0.5, "cosine")
    assert len(out) == 0 and out.type == pa.uint32()


def test_an_empty_matrix_is_an_empty_uint32_vector(monkeypatch):
    import polars_matmul

    def boom(*a, **k):  # (the metric's name is looked up first, as within_self does: no device)
        raise AssertionError("a handle for an empty matrix")

    monkeypatch.setattr(_native, "DeviceCorpus", boom)
    out = polars_matmul.duplicate_groups(np.zeros((0, 4), np.float32), 0.5)
    assert out.shape == (0,) and out.dtype == np.uint32


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
polars_matmul._duplicate_groups = lambda *a, **k: calls.append(("duplicate_groups", a, k)) or "groups-result"
ns = registry["pmm"]
out = {}
column = object()
e = Expr(); r = ns(e).duplicate_groups(0.95)
fn, kw = e.calls[0]
out["kw"] = [r[0], kw["is_elementwise"], kw["return_dtype"], sorted(kw)]
out["r"] = fn(column)
name, a, k2 = calls[-1]
out["call"] = [name, a[0] is column, list(a[1:]), k2]
e = Expr(); ns(e).duplicate_groups(1.5, metric="euclidean"); e.calls[0][0](column)
out["call2"] = [calls[-1][0], list(calls[-1][1][1:])]
try:
    ns(Expr()).duplicate_groups(0.5, compute="bf16")
    out["bf16"] = None
except TypeError as err:
    out["bf16"] = str(err)
try:
    ns(Expr()).duplicate_groups(0.5, compute="fp8")
    out["fp8"] = None
except ValueError as err:
    out["fp8"] = str(err)
print(json.dumps(out))
'''


def test_namespace_map_batches_contract():
    code = NAMESPACE_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    # a row's label depends on the whole column: not elementwise; one UInt32 per row
    assert out["kw"] == ["mapped", False, "u32", ["is_elementwise", "return_dtype"]]
    assert out["r"] == "groups-result"
    # the column itself is the corpus: it is the one Series handed on
    assert out["call"] == ["duplicate_groups", True, [0.95, "cosine"], {}]
    assert out["call2"] == ["duplicate_groups", [1.5, "euclidean"]]
    assert "self search runs on Float32 columns" in out["bf16"]
    assert "compute must be" in out["fp8"]


# ---- the truth helpers ----
def _reachability(n, rows, cols):
    reach = np.eye(n, dtype=bool)
    reach[rows, cols] = reach[cols, rows] = True
    for _ in range(n):  # (boolean closure by repeated squaring until it stands)
        nxt = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
        if np.array_equal(nxt, reach):
            break
        reach = nxt
    return reach


@pytest.mark.parametrize("metric", [sc_.COS, sc_.DOT, sc_.EUC])
def test_components_truth_against_brute_force_reachability(metric):
    n = 40
    c = sc_.f32(np.random.RandomState(17 + metric).randn(n, 5))
    full = sc_.ranked_self(c, metric)
    s = np.sort(full[1][np.isfinite(full[1])])
    t = float(s[int(0.06 * s.size)] if metric == sc_.EUC else s[int(0.94 * s.size)])
    offsets, idx, _ = sc_.range_self_truth(full, t, metric)
    rows = np.repeat(np.arange(n), np.diff(offsets))
    reach = _reachability(n, rows, idx.astype(np.int64))
    want = reach.argmax(axis=1)  # the first True of a row: the smallest row it reaches
    labels, components, pairs = cc.components_truth(full, t, metric)
    assert labels.dtype == np.uint32 and np.array_equal(labels, want), (labels, want)
    assert components == np.unique(want).size and pairs == idx.size
    # the case is worth something: a component that is not a clique, and singletons
    sizes = np.bincount(want, minlength=n)
    big = int(sizes.argmax())
    members = np.flatnonzero(want == big)
    assert sizes[big] >= 3 and (sizes == 1).sum() >= 3 and 1 < components < n
    direct = np.zeros((n, n), dtype=bool)
    direct[rows, idx.astype(np.int64)] = True
    assert not (direct | direct.T)[np.ix_(members, members)][~np.eye(members.size, dtype=bool)].all()
    ids = np.arange(n) * 3 + 1
    mapped, c2, p2 = cc.components_truth(full, t, metric, ids=ids)
    assert np.array_equal(mapped, ids[want]) and (c2, p2) == (components, pairs)


def test_chain_column_is_what_it_says():
    n, d = 600, 16
    c, chains, isolated = cc.chain_column(n, d, 1)
    assert c.shape == (n, d) and c.dtype == np.float32
    assert [len(r) for r in chains] == list(cc.CHAIN_LENGTHS)
    members = np.concatenate(chains + [isolated])
    assert np.array_equal(np.sort(members), np.arange(n))
    full = sc_.ranked_self(c, sc_.EUC)
    offsets, idx, _ = sc_.range_self_truth(full, cc.CHAIN_THRESHOLD, sc_.EUC)
    rows = np.repeat(np.arange(n), np.diff(offsets))
    edges = set(zip(rows.tolist(), idx.astype(np.int64).tolist()))
    # exactly the links between consecutive points, nothing else
    want = set()
    for r in chains:
        want |= {(min(a, b), max(a, b)) for a, b in zip(r[:-1].tolist(), r[1:].tolist())}
    assert edges == want
    labels, components, pairs = cc.components_truth(full, cc.CHAIN_THRESHOLD, sc_.EUC)
    assert pairs == sum(L - 1 for L in cc.CHAIN_LENGTHS)
    assert components == len(chains) + isolated.size
    for r in chains:
        assert (labels[r] == r.min()).all()  # one component, its smallest row
        assert (min(r[0], r[-1]), max(r[0], r[-1])) not in edges or len(r) == 2  # the end points: no edge
        if len(r) >= 3:
            assert r.min() not in (r[0], r[-1])  # an interior point
            assert len({x // 128 for x in r.tolist()}) > 1  # links cross blocks and tiles
    assert np.array_equal(labels[isolated], isolated)
