"""CPU side of grouped search (partitioned corpus handles, ``groups=``): the
host-only partition plan against numpy's stable sort, the label encoding and
its checks before any library call, the namespace packing ``by`` into a
struct (against a stand-in ``polars`` in a subprocess, as
tests/test_namespace.py), and the new kernels' resources (hipcc
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

from isa_util import CSRC, FLAGS, HIPCC, have_hipcc
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = _native.NO_GROUP
NAMES = ("pmm_partition_plan", "pmm_corpus_partition", "pmm_corpus_groups", "pmm_topk_f32_grouped",
         "pmm_topk_f64_grouped")


def test_grouped_entries_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", text), f"{name} not declared in include/pmm.h"
        assert name in _native.EXPORTED_SYMBOLS, f"{name} not in EXPORTED_SYMBOLS"
        assert getattr(_native.lib(), name).argtypes is not None, f"{name} has no argtypes"


def test_partitioned_handle_bytes_helper():
    for dt, comp in ((np.float32, "f32"), (np.float64, "f32"), (np.float32, "bf16")):
        assert (_native.partitioned_device_bytes(1000, 37, 8, dt, comp)
                == _native.subset_device_bytes(1000, 37, dt, comp) + 8 * 9)


# ---- pmm_partition_plan: host only ----
def reference_plan(labels, G):
    labels = np.asarray(labels, dtype=np.uint32)
    keep = np.flatnonzero(labels != NONE)
    perm = keep[np.argsort(labels[keep], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels[keep], minlength=G))])
    return perm.astype(np.uint32), offsets.astype(np.int64)


@pytest.mark.parametrize("n,G,none_every", [(1, 1, 0), (1037, 8, 0), (1037, 8, 5), (4096, 1, 3), (777, 300, 7)])
def test_partition_plan_equals_a_stable_sort(n, G, none_every):
    rs = np.random.RandomState(n + G)
    labels = rs.randint(0, G, size=n).astype(np.uint32)
    if none_every:
        labels[::none_every] = NONE
    perm, offsets = _native.partition_plan(labels, G)
    wperm, woff = reference_plan(labels, G)
    assert np.array_equal(perm, wperm) and np.array_equal(offsets, woff)
    assert perm.size == int((labels != NONE).sum()) == offsets[-1]
    for g in range(G):  # strictly ascending inside every group, every row of the group's label
        seg = perm[offsets[g]:offsets[g + 1]]
        assert np.all(np.diff(seg.astype(np.int64)) > 0) and np.all(labels[seg] == g)


def test_partition_plan_empty_groups_and_all_dropped():
    labels = np.array([5, 5, 2, NONE, 2, 5], dtype=np.uint32)
    perm, offsets = _native.partition_plan(labels, 7)
    assert perm.tolist() == [2, 4, 0, 1, 5]
    assert offsets.tolist() == [0, 0, 0, 2, 2, 2, 5, 5]
    perm, offsets = _native.partition_plan(np.full(4, NONE, dtype=np.uint32), 3)
    assert perm.size == 0 and offsets.tolist() == [0, 0, 0, 0]
    perm, offsets = _native.partition_plan(np.zeros(0, dtype=np.uint32), 2)
    assert perm.size == 0 and offsets.tolist() == [0, 0, 0]


def test_partition_plan_refuses_a_label_that_is_no_group():
    for labels, G, where in (([0, 1, 2], 2, "labels[2]"), ([7], 1, "labels[0]"), ([0, 0xFFFFFFFE], 4, "labels[1]")):
        with pytest.raises(_native.PmmError) as ei:
            _native.partition_plan(np.array(labels, dtype=np.uint32), G)
        assert ei.value.code == _native.PMM_ERR_ARG and where in str(ei.value), str(ei.value)


# ---- the label encoding of groups= ----
def test_string_labels_nulls_and_unseen_labels():
    right = pa.array(["b", "a", None, "b", "c", "a"])
    left = pa.array(["a", "zz", None, "c", "b"])
    g = pm._check_groups((left, right), 5, 6)
    assert g.G == 3 and g.clabels.dtype == np.uint32 and g.qlabels.dtype == np.uint32
    assert g.clabels.tolist() == [0, 1, NONE, 0, 2, 1]  # first-seen order: b, a, c
    assert g.qlabels.tolist() == [1, NONE, NONE, 2, 0]
    assert g.sizes.tolist() == [2, 2, 1] and g.searched_max() == 2
    assert g.key == pm._arrow_key(right) and g.keep is right
    # (string against large_string: the same labels)
    g2 = pm._check_groups((pa.array(["a"], type=pa.large_string()), right), 1, 6)
    assert g2.qlabels.tolist() == [1]


def test_integer_and_categorical_labels():
    right = np.array([10, -3, 10, 7], dtype=np.int64)
    left = np.array([7, 10, 99], dtype=np.int64)
    g = pm._check_groups((left, right), 3, 4)
    assert g.clabels.tolist() == [0, 1, 0, 2] and g.qlabels.tolist() == [2, 0, NONE] and g.key is None
    cat = pa.array(["x", "y", "x"]).dictionary_encode()
    g = pm._check_groups((pa.array(["y", "x"]), cat), 2, 3)
    assert g.clabels.tolist() == [0, 1, 0] and g.qlabels.tolist() == [1, 0]
    none = pm._check_groups((np.array([5]), np.array([1, 2])), 1, 2)
    assert none.searched_max() == 0


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library or of a device helper fails the test."""

    def boom(*a, **k):
        raise AssertionError("library call before the label check")

    for name in ("lib", "topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str",
                 "device_count", "set_devices"):
        monkeypatch.setattr(_native, name, boom)
    return monkeypatch


Q = np.zeros((2, 4), dtype=np.float32)
C = np.zeros((6, 4), dtype=np.float32)


def test_mismatched_label_types_raise_before_any_library_call(no_library):
    for left, right in ((np.array([1, 2]), pa.array(["a"] * 6)), (pa.array(["a", "b"]), np.arange(6)),
                        (np.array([1, 2], dtype=np.int32), np.arange(6, dtype=np.int64))):
        with pytest.raises(TypeError, match="one type"):
            pm._topk(Q, C, 1, "cosine", groups=(left, right))
    with pytest.raises(TypeError, match="hashable"):
        pm._topk(Q, C, 1, "cosine", groups=(np.zeros(2), np.zeros(6)))
    with pytest.raises(TypeError, match="pair"):
        pm._topk(Q, C, 1, "cosine", groups=np.arange(6))


def test_wrong_label_lengths_raise_before_any_library_call(no_library):
    with pytest.raises(ValueError, match="the queries have 2"):
        pm._topk(Q, C, 1, "cosine", groups=(np.arange(3), np.arange(6)))
    with pytest.raises(ValueError, match="the corpus has 6"):
        pm._topk(Q, C, 1, "cosine", groups=(np.arange(2), np.arange(5)))


def test_groups_with_subset_raises_before_any_library_call(no_library):
    with pytest.raises(ValueError, match="cannot be combined"):
        pm._topk(Q, C, 1, "cosine", groups=(np.arange(2), np.arange(6)), subset=np.ones(6, bool))
    import polars_matmul

    with pytest.raises(ValueError, match="cannot be combined"):
        polars_matmul.topk(Q, C, 1, groups=(np.arange(2), np.arange(6)), subset=np.ones(6, bool))


def test_ragged_lists_hold_no_padding():
    idx = np.array([[4, 9, 0xFFFFFFFF], [0xFFFFFFFF] * 3, [1, 2, 3]], dtype=np.uint32)
    sc = np.array([[0.5, 0.25, 0.0], [0.0] * 3, [3.0, 2.0, 1.0]], dtype=np.float32)
    out = pm._ragged_topk_arrow(idx, sc, np.array([2, 0, 3], dtype=np.uint32))
    assert out.type == pa.large_list(pm._TOPK_STRUCT)
    assert out.offsets.to_pylist() == [0, 2, 2, 5]
    assert out.values.field("index").to_pylist() == [4, 9, 1, 2, 3]
    assert out.values.field("score").to_pylist() == [0.5, 0.25, 3.0, 2.0, 1.0]


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
    """A struct batch: .struct.field(name) gives ("field", name)."""
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
labels = Series(["a", "b", "a"])
out = {}
emb = Expr("emb")
tag, packed, kw = ns(emb).topk(corpus, 5, "cosine", by="category", corpus_by=labels)
out["packed"] = [packed.name, [f.name for f in packed.fields], packed.fields[0].source is emb,
                 packed.fields[1].source.name, kw["is_elementwise"], emb.calls]
out["r"] = packed.calls[0][0](Batch)
a, k = calls[-1]
out["call"] = [list(a[0]), a[1] is corpus, list(a[2:]), sorted(k), list(k["groups"][0]), k["groups"][1] is labels]
by_expr = Expr("an-expr")
tag, packed, kw = ns(Expr("emb")).topk(corpus, 5, "dot", compute="bf16", by=by_expr, corpus_by=labels)
packed.calls[0][0](Batch)
a, k = calls[-1]
out["expr_by"] = [packed.fields[1].source is by_expr, sorted(k), k["compute"]]
e = Expr(); ns(e).topk(corpus, 5, "cosine"); e.calls[0][0]("b1")
a, k = calls[-1]
out["default"] = [a[0], a[1] is corpus, list(a[2:]), k]
for name, kwargs in (("only_by", {"by": "category"}), ("only_corpus_by", {"corpus_by": labels})):
    try:
        ns(Expr()).topk(corpus, 5, "cosine", **kwargs)
        out[name] = None
    except ValueError as err:
        out[name] = str(err)
try:
    ns(Expr()).topk(corpus, 5, "cosine", by="category", corpus_by=Expr())
    out["expr"] = None
except TypeError as err:
    out["expr"] = str(err)
print(json.dumps(out))
'''


def test_namespace_packs_by_into_a_struct_and_forwards_groups():
    code = NAMESPACE_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    # pl.struct(embedding, by) is what is mapped, elementwise; the embedding expression itself is not
    assert out["packed"] == ["struct", ["embedding", "by"], True, "col:category", True, []]
    assert out["r"] == "topk-result"
    assert out["call"] == [["field", "embedding"], True, [5, "cosine"], ["groups"], ["field", "by"], True]
    assert out["expr_by"] == [True, ["compute", "groups"], "bf16"]
    # the default call is still the reference's: four positional arguments, no keywords
    assert out["default"] == ["b1", True, [5, "cosine"], {}]
    assert "go together" in out["only_by"] and "go together" in out["only_corpus_by"]
    assert out["expr"].startswith("corpus_by must be a Polars Series, not an Expression.")


# ---- the kernels ----
@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_grouped_kernels_use_no_scratch():
    # the grouped kernel keeps 16 query rows, the chunk buffers and every row's
    # candidates in LDS and four chunks of loads in registers; 16 waves of 1024
    # threads leave 128 VGPRs per lane
    from test_kernel_resources import scratch_by_kernel

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "grouped.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_grouped.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = scratch_by_kernel(asm)
    for want, count in (("grouped_topk_f32_kernel", 3), ("grouped_scatter_kernel", 2), ("grouped_pad_kernel", 2)):
        hits = {k: v for k, v in sc.items() if want in k}
        assert len(hits) == count, f"{want}: {sorted(sc)}"
        assert set(hits.values()) == {(0, 0)}, f"scratch (bytes, instructions): {hits}"
    for name in sc:
        body = asm.split(f".amdhsa_kernel {name}")[1].split(".end_amdhsa_kernel")[0]
        vgpr = [int(l.split()[1]) for l in body.splitlines() if l.strip().startswith(".amdhsa_next_free_vgpr")]
        assert vgpr and vgpr[0] <= 128, (name, vgpr)
    assert "v_mfma_f32_16x16x4_f32" in asm or "v_mfma_f32_16x16x4f32" in asm
