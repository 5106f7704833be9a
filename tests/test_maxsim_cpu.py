"""CPU side of late-interaction search (pmm_topk_f32_maxsim, ``_topk_maxsim``,
``polars_matmul.topk_maxsim``, ``.pmm.topk_maxsim``): the header and bindings,
every refusal before any library call, the k clip, the ``candidates=None``
synthesis and its bound, the fallback's union and renumbering, the cached
path, the namespace (against a stand-in ``polars`` in a subprocess, as
tests/test_candidates_cpu.py) and the new kernels' resources (hipcc
cross-compiles gfx950 here)."""
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

import polars_matmul
from isa_util import CSRC, FLAGS, HIPCC, have_hipcc
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    for name, nargs in (("pmm_corpus_create_f32_docs", 6), ("pmm_corpus_docs", 4), ("pmm_topk_f32_maxsim", 11)):
        m = re.search(r"\bint %s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, f"{name} not declared in include/pmm.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _native.EXPORTED_SYMBOLS
        fn = getattr(_native.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    for method in ("multivector", "doc_offsets", "topk_maxsim"):
        assert hasattr(_native.DeviceCorpus, method)
    # the native limit on the padded dimension: one constant, stated in both headers
    internal = open(os.path.join(CSRC, "pmm_internal.h")).read()
    a = re.search(r"constexpr int kMaxsimMaxDp = (\d+);", internal)
    b = re.search(r"#define PMM_MAXSIM_MAX_DP (\d+)", text)
    assert a and b and a.group(1) == b.group(1) and int(a.group(1)) >= 256


def test_host_refusals_touch_no_device():
    L = _native.lib()
    assert L.pmm_topk_f32_maxsim(None, None, None, 0, None, None, 1, 0, None, None, None) == _native.PMM_ERR_ARG
    assert _native.last_error() == "null corpus"
    assert L.pmm_corpus_docs(None, None, None, 0) == _native.PMM_ERR_ARG
    assert L.pmm_corpus_create_f32_docs(None, 1, 1, None, 1, None) == _native.PMM_ERR_ARG
    # bad document bounds are refused naming the position, before any device call
    tok = np.zeros((4, 2), dtype=np.float32)
    import ctypes

    for offs, text in (([1, 4], "start at 0"), ([0, 2, 2, 4], "doc_offsets[2] = 2 follows 2"),
                       ([0, 3, 2, 4], "doc_offsets[2] = 2 follows 3"), ([0, 2, 3], "end at n_tokens")):
        o = np.array(offs, dtype=np.int64)
        h = ctypes.c_void_p()
        rc = L.pmm_corpus_create_f32_docs(_native.ptr(tok), 4, 2, _native.ptr(o), o.size - 1, ctypes.byref(h))
        assert rc == _native.PMM_ERR_ARG and text in _native.last_error() and not h.value


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library or of a device helper fails the test."""

    def boom(*a, **k):
        raise AssertionError("library call before the MaxSim checks")

    for name in ("lib", "topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str",
                 "device_count", "set_devices"):
        monkeypatch.setattr(_native, name, boom)
    return monkeypatch


def col(rows, d, ragged=False, dtype=pa.float32()):
    """A List column of token lists: rows = per-row lists of token vectors (None: a null row)."""
    inner = pa.list_(dtype) if ragged else pa.list_(dtype, d)
    return pa.array(rows, type=pa.large_list(inner))


Q = (np.zeros((3, 4), dtype=np.float32), np.array([0, 2, 3]))
D = (np.zeros((6, 4), dtype=np.float32), np.array([0, 1, 3, 6]))
GOOD = (np.array([0, 1, 2]), np.array([0, 2]))


def test_python_refusals_come_before_any_library_call(no_library):
    for fn in (pm._topk_maxsim, polars_matmul.topk_maxsim):
        with pytest.raises(ValueError, match="not a similarity"):
            fn(Q, D, 1, "euclidean", candidates=GOOD)
        with pytest.raises(ValueError, match="not a similarity"):
            fn(Q, D, 1, "l2")
        with pytest.raises(ValueError, match="Unknown metric"):
            fn(Q, D, 1, "manhattan")
        with pytest.raises(TypeError, match="MaxSim search runs on Float32 token columns"):
            fn((Q[0].astype(np.float64), Q[1]), D, 1, "cosine")
        with pytest.raises(TypeError, match="MaxSim search runs on Float32 token columns"):
            fn(Q, (D[0].astype(np.int8), D[1]), 1, "cosine")
        with pytest.raises(ValueError, match="document 1 is empty"):
            fn(Q, (D[0], np.array([0, 3, 3, 6])), 1, "cosine")
        with pytest.raises(ValueError, match="start at 0, not descend and end"):
            fn(Q, (D[0], np.array([0, 3, 5])), 1, "cosine")
        with pytest.raises(ValueError, match=r"row 1 hold the id 3: not a row of the corpus \(3 rows\)"):
            fn(Q, D, 1, "cosine", candidates=(np.array([0, 1, 2]), np.array([0, 3])))
        with pytest.raises(ValueError, match="hold 1 lists, the queries have 2 rows"):
            fn(Q, D, 1, "cosine", candidates=(np.array([0, 1]), np.array([0])))
        with pytest.raises(RuntimeError, match="Dimension mismatch"):
            fn((np.zeros((3, 5), dtype=np.float32), Q[1]), D, 1, "cosine", candidates=GOOD)
    with pytest.raises(TypeError, match=r"compute='bf16' has no MaxSim search"):
        pm._topk_maxsim(Q, D, 1, "cosine", compute="bf16")
    # Arrow columns
    tok = [[0.0] * 4]
    with pytest.raises(TypeError, match="hold double tokens"):
        pm._topk_maxsim(col([tok], 4, dtype=pa.float64()), col([tok], 4), 1, "cosine")
    with pytest.raises(TypeError, match="hold int8 tokens"):
        pm._topk_maxsim(col([tok], 4), col([[[0] * 4]], 4, dtype=pa.int8()), 1, "cosine")
    with pytest.raises(TypeError, match="List of Array"):
        pm._topk_maxsim(pa.array([[0.0] * 4], type=pa.list_(pa.float32())), col([tok], 4), 1, "cosine")
    with pytest.raises(ValueError, match="document 1 is null"):
        pm._topk_maxsim(col([tok], 4), col([tok, None], 4), 1, "cosine")
    with pytest.raises(ValueError, match="document 1 is empty"):
        pm._topk_maxsim(col([tok], 4), col([tok, []], 4), 1, "cosine")
    with pytest.raises(ValueError, match=r"token 2 has width 3, the first token has 4"):
        pm._topk_maxsim(col([tok], 4, True), col([tok * 2, [[0.0] * 3]], 4, True), 1, "cosine")
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        pm._topk_maxsim(col([[[0.0] * 5]], 5), col([tok], 4), 1, "cosine")


def test_token_columns_parse_to_tokens_and_offsets():
    rows = [[[1.0, 2.0], [3.0, 4.0]], None, [], [[5.0, 6.0]]]
    for ragged in (False, True):
        t, o, arr = pm._token_lists(col(rows, 2, ragged), "the queries", False)
        assert t.dtype == np.float32 and t.tolist() == [[1, 2], [3, 4], [5, 6]] and o.tolist() == [0, 2, 2, 2, 3]
        assert isinstance(arr, pa.Array)
        t, o, _ = pm._token_lists(col(rows, 2, ragged).slice(3), "the queries", False)
        assert t.tolist() == [[5, 6]] and o.tolist() == [0, 1]
    t, o, arr = pm._token_lists((np.ones((3, 2), dtype=np.float32), np.array([0, 3], dtype=np.int32)), "q", True)
    assert arr is None and o.dtype == np.int64 and t.shape == (3, 2)


# ---- the executor's two routes (stub handles) ----
def maxsim_dot(qt, dt):
    return np.float32((qt @ dt.T).max(axis=1).sum()) if qt.shape[0] else np.float32(0)


class StubCorpus:
    """Records multivector / topk_maxsim calls; answers by a NumPy MaxSim (dot)."""

    calls: list = []
    made: list = []
    shards = 1
    nbytes = 0

    def __init__(self, tokens, offsets):
        self.tokens, self.offsets = np.array(tokens), np.array(offsets)

    @classmethod
    def multivector(cls, tokens, offsets):
        self = cls(tokens, offsets)
        StubCorpus.made.append(self)
        return self

    def acquire(self):
        return self

    def release(self):
        pass

    def close(self):
        pass

    def topk_maxsim(self, qt, qo, co, ci, k, metric):
        StubCorpus.calls.append((self, np.array(qt), np.array(qo), np.array(co), np.array(ci), k, metric))
        m = qo.size - 1
        idx = np.full((m, k), 0xFFFFFFFF, dtype=np.uint32)
        sc = np.zeros((m, k), dtype=np.float32)
        lens = np.zeros(m, dtype=np.uint32)
        for i in range(m):
            S = ci[co[i]:co[i + 1]]
            if qo[i + 1] == qo[i]:
                continue
            v = np.array([maxsim_dot(qt[qo[i]:qo[i + 1]], self.tokens[self.offsets[c]:self.offsets[c + 1]]) for c in S])
            order = np.lexsort((S, -v.astype(np.float64)))[:k]
            lens[i] = order.size
            idx[i, :order.size], sc[i, :order.size] = S[order], v[order]
        return idx, sc, lens


@pytest.fixture
def stubbed(monkeypatch):
    StubCorpus.calls, StubCorpus.made = [], []
    monkeypatch.setattr(_native, "DeviceCorpus", StubCorpus)
    monkeypatch.setattr(_native, "get_devices", lambda: [])
    monkeypatch.setattr(pm, "_devices_env_done", True)
    return monkeypatch


def problem(nd=40, m=5, d=4, seed=3):
    rs = np.random.RandomState(seed)
    do = np.concatenate([[0], np.cumsum(rs.randint(1, 6, size=nd))]).astype(np.int64)
    qo = np.concatenate([[0], np.cumsum(rs.randint(0, 4, size=m))]).astype(np.int64)
    return rs.randn(qo[-1], d).astype(np.float32), qo, rs.randn(do[-1], d).astype(np.float32), do


def test_k_clips_and_empty_lists_need_no_device(stubbed):
    qt, qo, dt, do = problem()
    out = pm._topk_maxsim((qt, qo), (dt, do), 100, "dot",
                          candidates=pa.array([[7, 2, 2], None, [9], [], [1, 0, 3]], type=pa.list_(pa.int64())))
    assert StubCorpus.calls[-1][5] == 3  # k = the longest normalised list
    assert out.type == pa.large_list(pm._TOPK_STRUCT) and [len(r) for r in out.to_pylist()] == [
        min(2, 2) if qo[1] > qo[0] else 0, 0, 1 if qo[3] > qo[2] else 0, 0, 3 if qo[5] > qo[4] else 0]
    n_calls = len(StubCorpus.calls)
    out = pm._topk_maxsim((qt, qo), (dt, do), 5, "dot", candidates=pa.array([None] * 5, type=pa.list_(pa.int64())))
    assert out.to_pylist() == [[]] * 5 and len(StubCorpus.calls) == n_calls
    gi, gs = polars_matmul.topk_maxsim((qt, qo), (dt, do), 5, "dot", candidates=(np.zeros(6, np.int64), np.zeros(0, np.int64)))
    assert gi.shape == (5, 0) and gs.shape == (5, 0) and len(StubCorpus.calls) == n_calls
    gi, gs = polars_matmul.topk_maxsim((qt, qo), (dt, do), 0, "dot")
    assert gi.shape == (5, 0) and len(StubCorpus.calls) == n_calls
    # no query rows: an empty column, no device
    out = pm._topk_maxsim((np.zeros((0, 4), np.float32), np.zeros(1, np.int64)), (dt, do), 5, "dot")
    assert len(out) == 0 and len(StubCorpus.calls) == n_calls


def test_candidates_none_lists_every_document_up_to_the_bound(stubbed):
    qt, qo, dt, do = problem()
    gi, gs = polars_matmul.topk_maxsim((qt, qo), (dt, do), 1000, "dot")
    _, _, _, co, ci, k, metric = StubCorpus.calls[-1]
    assert k == 40 and metric == _native.METRIC_DOT
    assert co.tolist() == (np.arange(6) * 40).tolist() and ci.tolist() == list(range(40)) * 5
    assert gi.shape == (5, 40)
    live = np.diff(qo) > 0
    assert (gi[~live] == 0xFFFFFFFF).all() and np.isnan(gs[~live]).all() and not np.isnan(gs[live]).any()
    stubbed.setattr(pm, "_MAXSIM_SYNTH_MAX", 5 * 40 - 1)
    n_calls = len(StubCorpus.calls)
    with pytest.raises(ValueError, match="give candidates="):
        polars_matmul.topk_maxsim((qt, qo), (dt, do), 3, "dot")
    assert len(StubCorpus.calls) == n_calls and pm._MAXSIM_SYNTH_MAX == 199
    stubbed.undo()
    assert pm._MAXSIM_SYNTH_MAX == 1 << 24


def test_fallback_searches_the_union_with_renumbered_lists(stubbed):
    qt, qo, dt, do = problem(nd=300, m=9)
    rs = np.random.RandomState(8)
    rows = [np.sort(rs.choice(300, size=rs.randint(0, 12), replace=False)) for _ in range(9)]
    co = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    ci = np.concatenate(rows).astype(np.uint32)
    # numpy pairs are not cacheable: the fallback
    gi, gs = polars_matmul.topk_maxsim((qt, qo), (dt, do), 5, "dot", candidates=(co, ci))
    (handle, _, _, offs, local, k, _), = StubCorpus.calls
    U = np.array(sorted(set(ci.tolist())), dtype=np.uint32)
    assert len(StubCorpus.made) == 1 and k == 5 and np.array_equal(offs, co)
    # the union's documents, whole and in order, and the lists by their place in it
    assert np.array_equal(np.diff(handle.offsets), np.diff(do)[U])
    assert np.array_equal(handle.tokens, np.concatenate([dt[do[c]:do[c + 1]] for c in U]))
    assert np.array_equal(U[local], ci) and np.array_equal(local, np.searchsorted(U, ci))
    # mapped back: what the whole column's handle returns
    wi, ws, wl = StubCorpus(dt, do).topk_maxsim(qt, qo, co, ci, 5, 1)
    assert np.array_equal(gi, wi)
    used = np.arange(5)[None, :] < wl[:, None].astype(np.int64)
    assert np.array_equal(gs[used], ws[used].astype(np.float64)) and np.isnan(gs[~used]).all()


def test_cached_handle_is_searched_with_the_lists_as_they_are(stubbed):
    nd, d = 1 << 15, 8
    dt = np.zeros((2 * nd, d), dtype=np.float32)  # 2 MiB: above the caching floor
    dt[:, 0] = np.arange(2 * nd)
    docs = pa.LargeListArray.from_arrays(pa.array(np.arange(nd + 1, dtype=np.int64) * 2),
                                         pa.FixedSizeListArray.from_arrays(pa.array(dt.reshape(-1)), d))
    q = col([[[1.0] + [0.0] * 7], [[1.0] + [0.0] * 7] * 2], d)
    stubbed.setattr(_native, "device_memory", lambda: (1 << 40, 1 << 40))
    stubbed.setattr(_native, "corpus_device_bytes", lambda n, d, dt, c="f32": n * d * 4)
    stubbed.setattr(pm, "_CACHE_ON", True)
    stubbed.setattr(pm, "_cache", type(pm._cache)())
    out = pm._topk_maxsim(q, docs, 2, "dot", candidates=(np.array([0, 3, 4]), np.array([70, 9, 4000, 5])))
    (handle, _, qo, co, ci, k, _), = StubCorpus.calls
    assert handle.tokens.shape == dt.shape and handle.offsets.size == nd + 1 and len(StubCorpus.made) == 1
    assert qo.tolist() == [0, 1, 3] and co.tolist() == [0, 3, 4] and ci.tolist() == [9, 70, 4000, 5] and k == 2
    assert len(pm._cache) == 1
    assert [[e["index"] for e in row] for row in out.to_pylist()] == [[4000, 70], [5]]
    assert out.to_pylist()[1][0]["score"] == 2 * 11.0
    pm._topk_maxsim(q, docs, 2, "dot", candidates=(np.array([0, 1, 1]), np.array([3])))
    assert StubCorpus.calls[-1][0] is handle and len(StubCorpus.made) == 1


# ---- the namespace ----
NAMESPACE_SCRIPT = r'''
import json, sys, types
sys.path.insert(0, %(pkg)r)
pl = types.ModuleType("polars")
pl.UInt32, pl.Float32, pl.Float64 = "u32", "f32", "f64"
pl.List = lambda inner: ("List", inner)
pl.Struct = lambda fields: ("Struct", tuple(fields.items()))
pl.Array = lambda inner, n: ("Array", inner, n)
class Expr:
    def __init__(self, name="expr", fields=None):
        self.name, self.fields, self.calls = name, fields, []
    def alias(self, name):
        e = Expr(name); e.source = self
        return e
    def map_batches(self, fn, **kw):
        self.calls.append((fn, kw))
        return ("mapped", self, kw)
class Series:
    def __init__(self, values):
        self.values = values
    def __len__(self):
        return len(self.values)
class Batch:
    struct = types.SimpleNamespace(field=lambda name: ("field", name))
registry = {}
def register_expr_namespace(name):
    def deco(cls):
        registry[name] = cls
        return cls
    return deco
pl.Expr, pl.Series = Expr, Series
pl.col = lambda name: Expr("col:" + name)
pl.struct = lambda *exprs: Expr("struct", list(exprs))
pl.api = types.SimpleNamespace(register_expr_namespace=register_expr_namespace)
sys.modules["polars"] = pl

import polars_matmul
calls = []
def rec(*args, **kw):
    calls.append((args, kw))
    return "maxsim-result"
polars_matmul._topk_maxsim = rec
ns = registry["pmm"]
docs = Series([[[1.0, 0.0]]] * 3)
out = {}
tok = Expr("tok")
tag, packed, kw = ns(tok).topk_maxsim(docs, 5, "dot", candidates="hits")
out["packed"] = [packed.name, [f.name for f in packed.fields], packed.fields[0].source is tok,
                 packed.fields[1].source.name, kw["is_elementwise"], tok.calls]
out["r"] = packed.calls[0][0](Batch)
a, k = calls[-1]
out["call"] = [list(a[0]), a[1] is docs, list(a[2:]), sorted(k), list(k["candidates"])]
an_expr = Expr("an-expr")
tag, packed, kw = ns(Expr("tok")).topk_maxsim(docs, 5, candidates=an_expr)
out["expr"] = packed.fields[1].source is an_expr
e = Expr(); ns(e).topk_maxsim(docs, 5); e.calls[0][0]("b1")
a, k = calls[-1]
out["default"] = [a[0], a[1] is docs, list(a[2:]), k]
try:
    ns(Expr()).topk_maxsim(Expr("docs"), 5)
    out["expr_docs"] = None
except TypeError as err:
    out["expr_docs"] = str(err)
print(json.dumps(out))
'''


def test_namespace_packs_the_lists_and_forwards_the_keyword_only_when_given():
    code = NAMESPACE_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["packed"] == ["struct", ["tokens", "candidates"], True, "col:hits", True, []]
    assert out["r"] == "maxsim-result"
    assert out["call"] == [["field", "tokens"], True, [5, "dot"], ["candidates"], ["field", "candidates"]]
    assert out["expr"] is True
    assert out["default"] == ["b1", True, [5, "cosine"], {}]
    assert "must be a Polars Series" in out["expr_docs"]


# ---- the kernels ----
@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_maxsim_kernels_compile_without_scratch():
    from test_kernel_resources import scratch_by_kernel

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "maxsim.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_maxsim.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = scratch_by_kernel(asm)
    for want, count in (("maxsim_score_kernel", 2), ("maxsim_decode_kernel", 1)):
        hits = {k: v for k, v in sc.items() if want in k}
        assert len(hits) == count, f"{want}: {sorted(sc)}"
        assert set(hits.values()) == {(0, 0)}, f"scratch (bytes, instructions): {hits}"
    for name in (k for k in sc if "maxsim_score_kernel" in k):
        func = asm.split(f"{name}:")[1].split("s_endpgm")[0]
        # 16-byte gathers through LDS into the f32 MFMA, two accumulator blocks
        assert func.count("global_load_dwordx4") >= 8 and "ds_write_b128" in func and "ds_read_b128" in func
        assert func.count("v_mfma_f32_32x32x2_f32") >= 32
