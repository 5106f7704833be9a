"""CPU side of candidate search (pmm_topk_f32_candidates, ``candidates=``): the
list normaliser, every refusal before any library call, the k clip, the
fallback's union and renumbering against a NumPy restatement, the namespace
packing the lists into a struct (against a stand-in ``polars`` in a subprocess,
as tests/test_grouped_cpu.py), the header, and the new kernels' resources
(hipcc cross-compiles gfx950 here)."""
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


def test_entry_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    m = re.search(r"\bint pmm_topk_f32_candidates\s*\(([^;]*)\)\s*;", text)
    assert m, "pmm_topk_f32_candidates not declared in include/pmm.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[3].startswith("const int64_t *cand_offsets") and args[4] == "const uint32_t *cand_ids"
    assert "pmm_topk_f32_candidates" in _native.EXPORTED_SYMBOLS
    fn = _native.lib().pmm_topk_f32_candidates
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    assert hasattr(_native.DeviceCorpus, "topk_candidates")


def test_host_refusals_touch_no_device():
    # null corpus, and nothing else is reachable without a handle
    L = _native.lib()
    assert L.pmm_topk_f32_candidates(None, None, 0, None, None, 1, 0, None, None, None) == _native.PMM_ERR_ARG
    assert _native.last_error() == "null corpus"


# ---- the normaliser ----
def test_unsorted_duplicate_and_null_lists():
    arr = pa.array([[5, 1, 1, 3], None, [], [2, 0, 2]], type=pa.list_(pa.int32()))
    c = pm._check_candidates(arr, 4, 7)
    assert c.offsets.dtype == np.int64 and c.ids.dtype == np.uint32
    assert c.offsets.tolist() == [0, 3, 3, 3, 5] and c.ids.tolist() == [1, 3, 5, 0, 2] and c.maxlen == 3
    # already ascending lists pass through as they are
    c = pm._check_candidates(pa.array([[0, 6], [3]], type=pa.list_(pa.uint8())), 2, 7)
    assert c.offsets.tolist() == [0, 2, 3] and c.ids.tolist() == [0, 6, 3]


def test_large_list_sliced_and_offsets_pair_input():
    arr = pa.array([[9, 9], [4, 2], None, [6, 6, 0]], type=pa.large_list(pa.uint64())).slice(1)
    c = pm._check_candidates(arr, 3, 7)
    assert c.offsets.tolist() == [0, 2, 2, 4] and c.ids.tolist() == [2, 4, 0, 6]
    c = pm._check_candidates((np.array([0, 2, 2, 5]), np.array([3, 0, 6, 6, 1], dtype=np.int16)), 3, 7)
    assert c.offsets.tolist() == [0, 2, 2, 4] and c.ids.tolist() == [0, 3, 1, 6]
    c = pm._check_candidates((np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.uint32)), 2, 7)
    assert c.maxlen == 0 and c.ids.size == 0
    ch = pa.chunked_array([pa.array([[1]], type=pa.list_(pa.int64())), pa.array([[0, 1]], type=pa.list_(pa.int64()))])
    assert pm._check_candidates(ch, 2, 2).ids.tolist() == [1, 0, 1]


def test_normaliser_equals_a_per_row_restatement():
    rs = np.random.RandomState(4)
    m, n = 200, 50
    rows = [rs.randint(0, n, size=rs.randint(0, 30)).tolist() for _ in range(m)]
    c = pm._check_candidates(pa.array(rows, type=pa.large_list(pa.int64())), m, n)
    want = [sorted(set(r)) for r in rows]
    assert c.offsets.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want])]).tolist()
    assert c.ids.tolist() == [x for r in want for x in r]
    assert c.maxlen == max(len(r) for r in want)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library or of a device helper fails the test."""

    def boom(*a, **k):
        raise AssertionError("library call before the candidates check")

    for name in ("lib", "topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str",
                 "device_count", "set_devices"):
        monkeypatch.setattr(_native, name, boom)
    return monkeypatch


Q = np.zeros((2, 4), dtype=np.float32)
C = np.zeros((6, 4), dtype=np.float32)
GOOD = (np.array([0, 1, 2]), np.array([0, 5]))


def test_wrong_lists_raise_before_any_library_call(no_library):
    with pytest.raises(ValueError, match="hold 3 lists, the queries have 2 rows"):
        pm._topk(Q, C, 1, "cosine", candidates=pa.array([[0], [1], [2]], type=pa.list_(pa.int64())))
    with pytest.raises(ValueError, match="hold 1 lists, the queries have 2 rows"):
        pm._topk(Q, C, 1, "cosine", candidates=(np.array([0, 1]), np.array([0])))
    with pytest.raises(ValueError, match=r"row 1 hold the id null"):
        pm._topk(Q, C, 1, "cosine", candidates=pa.array([[0], [1, None]], type=pa.list_(pa.int64())))
    with pytest.raises(ValueError, match=r"row 0 hold the id -1"):
        pm._topk(Q, C, 1, "cosine", candidates=pa.array([[2, -1], [1]], type=pa.list_(pa.int64())))
    with pytest.raises(ValueError, match=r"row 1 hold the id 6: not a row of the corpus \(6 rows\)"):
        pm._topk(Q, C, 1, "cosine", candidates=(np.array([0, 1, 2]), np.array([0, 6])))
    with pytest.raises(ValueError, match="start at 0"):
        pm._topk(Q, C, 1, "cosine", candidates=(np.array([1, 1, 2]), np.array([0, 5])))
    with pytest.raises(TypeError, match="List of integer row ids"):
        pm._topk(Q, C, 1, "cosine", candidates=pa.array([[0.5], [1.0]]))
    with pytest.raises(TypeError, match="List of integer row ids"):
        pm._topk(Q, C, 1, "cosine", candidates=pa.array([0, 1]))
    with pytest.raises(TypeError, match="pair"):
        pm._topk(Q, C, 1, "cosine", candidates=3)


def test_combinations_raise_before_any_library_call(no_library):
    with pytest.raises(ValueError, match="cannot be combined with subset= or groups="):
        pm._topk(Q, C, 1, "cosine", candidates=GOOD, subset=np.ones(6, bool))
    with pytest.raises(ValueError, match="cannot be combined with subset= or groups="):
        pm._topk(Q, C, 1, "cosine", candidates=GOOD, groups=(np.arange(2), np.arange(6)))
    with pytest.raises(ValueError, match="cannot be combined"):
        polars_matmul.topk(Q, C, 1, candidates=GOOD, subset=np.ones(6, bool))


def test_other_columns_raise_type_errors_before_any_library_call(no_library):
    advice = r"cast the embeddings first, e\.g\. pl\.col\('embedding'\)\.cast\(pl\.List\(pl\.Float32\)\)"
    with pytest.raises(TypeError, match=r"candidate search runs on Float32 columns \(compute=\"bf16\" has no candidate "
                                        r"search\); " + advice):
        pm._topk(Q, C, 1, "cosine", compute="bf16", candidates=GOOD)
    for q, c in ((Q.astype(np.float64), C), (Q, C.astype(np.float64)), (Q.astype(np.int8), C.astype(np.int8))):
        with pytest.raises(TypeError, match=r"candidate search runs on Float32 columns \(got a column of another "
                                            r"type\); " + advice):
            pm._topk(q, c, 1, "cosine", candidates=GOOD)  # (int8 does not take the f64 route silently)
        with pytest.raises(TypeError, match="candidate search runs on Float32 columns"):
            polars_matmul.topk(q, c, 1, candidates=GOOD)
    with pytest.raises(TypeError, match="candidate search runs on Float32 columns"):
        polars_matmul.topk(Q, C, 1, compute="bf16", candidates=GOOD)


# ---- the k clip, the empty case, the executor's two routes (stub handles) ----
class StubCorpus:
    """Records topk_candidates calls; answers with each list's first k ids."""

    calls: list = []
    shards = 1
    nbytes = 0

    def __init__(self, c, compute="f32"):
        self.c = np.array(c)

    def acquire(self):
        return self

    def release(self):
        pass

    def close(self):
        pass

    def topk_candidates(self, q, offsets, ids, k, metric):
        StubCorpus.calls.append((self, np.array(q), np.array(offsets), np.array(ids), k, metric))
        m = q.shape[0]
        idx = np.full((m, k), 0xFFFFFFFF, dtype=np.uint32)
        sc = np.zeros((m, k), dtype=np.float32)
        lens = np.minimum(np.diff(offsets), k).astype(np.uint32)
        for i in range(m):
            idx[i, :lens[i]] = ids[offsets[i]:offsets[i] + lens[i]]
            sc[i, :lens[i]] = self.c[idx[i, :lens[i]], 0]
        return idx, sc, lens


@pytest.fixture
def stubbed(monkeypatch):
    StubCorpus.calls = []
    monkeypatch.setattr(_native, "DeviceCorpus", StubCorpus)
    monkeypatch.setattr(_native, "get_devices", lambda: [])
    monkeypatch.setattr(_native, "metric_from_str", lambda s: 0)
    monkeypatch.setattr(pm, "_devices_env_done", True)
    return monkeypatch


def test_k_clips_to_the_longest_list_and_empty_lists_need_no_device(stubbed):
    c = np.arange(40, dtype=np.float32).reshape(10, 4)
    q = np.zeros((3, 4), dtype=np.float32)
    out = pm._topk(q, c, 100, "cosine", candidates=pa.array([[7, 2, 2], None, [9]], type=pa.list_(pa.int64())))
    assert StubCorpus.calls[-1][4] == 2  # k = the longest normalised list
    assert out.type == pa.large_list(pm._TOPK_STRUCT)
    assert [[e["index"] for e in row] for row in out.to_pylist()] == [[2, 7], [], [9]]
    n_calls = len(StubCorpus.calls)
    out = pm._topk(q, c, 5, "cosine", candidates=pa.array([None, [], None], type=pa.list_(pa.int64())))
    assert out.to_pylist() == [[], [], []] and len(StubCorpus.calls) == n_calls
    gi, gs = polars_matmul.topk(q, c, 5, candidates=(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64)))
    assert gi.shape == (3, 0) and gs.shape == (3, 0) and len(StubCorpus.calls) == n_calls
    gi, gs = polars_matmul.topk(q, c, 5, candidates=(np.array([0, 2, 2, 3]), np.array([2, 7, 9])))
    assert gi.tolist() == [[2, 7], [0xFFFFFFFF] * 2, [9, 0xFFFFFFFF]]
    assert np.isnan(gs[1]).all() and np.isnan(gs[2, 1]) and gs[0].tolist() == [8.0, 28.0]


def test_fallback_searches_the_union_with_renumbered_lists(stubbed):
    rs = np.random.RandomState(8)
    n, m, d = 500, 23, 4
    c = rs.randn(n, d).astype(np.float32)
    q = rs.randn(m, d).astype(np.float32)
    rows = [np.sort(rs.choice(n, size=rs.randint(0, 12), replace=False)) for _ in range(m)]
    offsets = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    ids = np.concatenate(rows).astype(np.uint32)
    cand = pm._Candidates(offsets, ids)
    # a numpy corpus is not cacheable: the fallback
    idx, sc, lens = pm._topk_candidates(q, c, None, c, cand, 5, 0)
    (handle, _, offs, local, k, _), = StubCorpus.calls
    # the NumPy restatement: the sorted union, the lists by searchsorted, the result mapped back
    U = np.array(sorted(set(ids.tolist())), dtype=np.uint32)
    assert np.array_equal(handle.c, c[U]) and k == 5 and np.array_equal(offs, offsets)
    assert np.array_equal(local, np.array([U.tolist().index(x) for x in ids.tolist()], dtype=np.uint32))
    assert np.array_equal(U[local], ids) and np.all(np.diff(U.astype(np.int64)) > 0)
    for i in range(m):
        assert idx[i, :lens[i]].tolist() == rows[i][:5].tolist()  # parent numbering, order kept
        assert (idx[i, lens[i]:] == 0xFFFFFFFF).all()
        assert np.array_equal(sc[i, :lens[i]], c[rows[i][:5], 0])
    u2, l2 = pm._candidates_union(cand)
    assert np.array_equal(u2, U) and np.array_equal(l2, local)


def test_cached_handle_is_searched_with_the_lists_as_they_are(stubbed):
    c = np.zeros((1 << 16, 8), dtype=np.float32)  # 2 MiB: above the caching floor
    c[:, 0] = np.arange(1 << 16)
    corpus = pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1)), 8)
    q = np.zeros((2, 8), dtype=np.float32)
    stubbed.setattr(_native, "device_memory", lambda: (1 << 40, 1 << 40))
    stubbed.setattr(pm, "_CACHE_ON", True)
    stubbed.setattr(pm, "_cache", type(pm._cache)())
    out = pm._topk(q, corpus, 2, "dot", candidates=(np.array([0, 3, 4]), np.array([70, 9, 4000, 5])))
    (handle, _, offs, ids, k, _), = StubCorpus.calls
    assert handle.c.shape == c.shape and ids.tolist() == [9, 70, 4000, 5] and k == 2 and len(pm._cache) == 1
    assert [[e["index"] for e in row] for row in out.to_pylist()] == [[9, 70], [5]]
    # a second call finds the handle again
    pm._topk(q, corpus, 2, "dot", candidates=(np.array([0, 1, 1]), np.array([3])))
    assert StubCorpus.calls[-1][0] is handle


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
    return "topk-result"
polars_matmul._topk = rec
ns = registry["pmm"]
corpus = Series([[1.0, 0.0]] * 3)
out = {}
emb = Expr("emb")
tag, packed, kw = ns(emb).topk(corpus, 5, "cosine", candidates="hits")
out["packed"] = [packed.name, [f.name for f in packed.fields], packed.fields[0].source is emb,
                 packed.fields[1].source.name, kw["is_elementwise"], emb.calls]
out["r"] = packed.calls[0][0](Batch)
a, k = calls[-1]
out["call"] = [list(a[0]), a[1] is corpus, list(a[2:]), sorted(k), list(k["candidates"])]
an_expr = Expr("an-expr")
tag, packed, kw = ns(Expr("emb")).topk(corpus, 5, "dot", candidates=an_expr)
out["expr"] = packed.fields[1].source is an_expr
e = Expr(); ns(e).topk(corpus, 5, "cosine"); e.calls[0][0]("b1")
a, k = calls[-1]
out["default"] = [a[0], a[1] is corpus, list(a[2:]), k]
e = Expr(); ns(e).topk(corpus, 5, "cosine", subset=Series([True])); e.calls[0][0]("b2")
out["subset_only"] = sorted(calls[-1][1])
for name, kwargs in (("with_by", {"by": "category", "corpus_by": Series(["a"] * 3)}), ("with_subset", {"subset": Series([True])})):
    try:
        ns(Expr()).topk(corpus, 5, "cosine", candidates="hits", **kwargs)
        out[name] = None
    except ValueError as err:
        out[name] = str(err)
print(json.dumps(out))
'''


def test_namespace_packs_the_lists_and_forwards_the_keyword_only_when_given():
    code = NAMESPACE_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["packed"] == ["struct", ["embedding", "candidates"], True, "col:hits", True, []]
    assert out["r"] == "topk-result"
    assert out["call"] == [["field", "embedding"], True, [5, "cosine"], ["candidates"], ["field", "candidates"]]
    assert out["expr"] is True
    # without the keyword the calls are what they were: four positional arguments, no candidates=
    assert out["default"] == ["b1", True, [5, "cosine"], {}]
    assert out["subset_only"] == ["subset"]
    assert "cannot be combined" in out["with_by"] and "cannot be combined" in out["with_subset"]


# ---- the kernels ----
@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_candidate_kernels_use_no_scratch_and_gather_wide():
    from test_kernel_resources import scratch_by_kernel

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "candidates.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_candidates.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = scratch_by_kernel(asm)
    for want, count in (("cand_score_kernel", 3), ("cand_merge_kernel", 1), ("cand_decode_kernel", 1)):
        hits = {k: v for k, v in sc.items() if want in k}
        assert len(hits) == count, f"{want}: {sorted(sc)}"
        assert set(hits.values()) == {(0, 0)}, f"scratch (bytes, instructions): {hits}"
    for name in (k for k in sc if "cand_score_kernel" in k):
        body = asm.split(f".amdhsa_kernel {name}")[1].split(".end_amdhsa_kernel")[0]
        vgpr = [int(l.split()[1]) for l in body.splitlines() if l.strip().startswith(".amdhsa_next_free_vgpr")]
        assert vgpr and vgpr[0] <= 128, (name, vgpr)  # four workgroups per CU, as the LDS tile allows
        func = asm.split(f"{name}:")[1].split("s_endpgm")[0]
        # 16-byte gathers through LDS and back, the query row by scalar loads, no workgroup barrier
        assert func.count("global_load_dwordx4") >= 16 and "ds_write_b128" in func and "ds_read_b128" in func
        assert "s_load_dwordx16" in func or "s_load_dwordx8" in func
        assert "s_barrier" not in func
