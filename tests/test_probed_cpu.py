"""CPU side of probed search (``pmm_topk_f32_probed``, ``groups=`` with a list
of labels per query row): the host-only probe plan against a NumPy
restatement, the refusals and the label encoding before any library call, the
host fallback's per-row merge against the oracle on the union of the probed
groups, and the new kernels' resources (hipcc cross-compiles gfx950 here)."""
from __future__ import annotations

import os
import re
import subprocess
import tempfile

import numpy as np
import pyarrow as pa
import pytest

import oracle
from isa_util import CSRC, FLAGS, HIPCC, have_hipcc
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = _native.NO_GROUP
NAMES = ("pmm_probe_plan", "pmm_topk_f32_probed")


def test_probed_entries_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmm.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", text), f"{name} not declared in include/pmm.h"
        assert name in _native.EXPORTED_SYMBOLS, f"{name} not in EXPORTED_SYMBOLS"
        assert getattr(_native.lib(), name).argtypes is not None, f"{name} has no argtypes"
    assert callable(_native.DeviceCorpus.topk_probed) and callable(_native.probe_plan)


# ---- pmm_probe_plan: host only ----
def reference_plan(po, pl, goff, k):
    """The plan restated: per row the distinct labels with a non-empty
    segment, the (row, label) slots stably sorted by label, every row's slot
    numbers ascending by label, min(k, rows of the union)."""
    m = len(po) - 1
    sizes = np.diff(goff)
    per_row = []
    for i in range(m):
        ls = [int(x) for x in pl[po[i]:po[i + 1]] if x != NONE]
        per_row.append(sorted({x for x in ls if sizes[x] > 0}))
    slots = sorted((l, i) for i, ls in enumerate(per_row) for l in ls)
    number = {s: j for j, s in enumerate(slots)}
    row_offsets = np.concatenate([[0], np.cumsum([len(ls) for ls in per_row])]).astype(np.int64)
    row_slots = [number[(l, i)] for i, ls in enumerate(per_row) for l in ls]
    out_len = [min(k, int(sum(sizes[l] for l in ls))) for ls in per_row]
    return ([i for _, i in slots], [l for l, _ in slots], row_offsets, row_slots, out_len)


def assert_plan(po, pl, goff, k):
    got = _native.probe_plan(po, pl, goff, k)
    want = reference_plan(np.asarray(po), np.asarray(pl, dtype=np.uint32), np.asarray(goff), k)
    for g, w, name in zip(got, want, ("slot_row", "slot_label", "row_offsets", "row_slots", "out_len")):
        assert np.array_equal(g, np.asarray(w, dtype=g.dtype)), (name, g, w)
    return got


def test_probe_plan_small_cases_by_hand():
    goff = [0, 3, 3, 10, 11]  # group 1 is empty
    # row 0: a repeat; row 1: no list; row 2: the none label and the empty group; row 3: unsorted labels
    pl = [2, 0, 2, NONE, 1, 3, 3, 2, 0]
    po = [0, 3, 3, 6, 9]
    slot_row, slot_label, row_offsets, row_slots, out_len = assert_plan(po, pl, goff, 5)
    assert slot_label.tolist() == [0, 0, 2, 2, 3, 3] and slot_row.tolist() == [0, 3, 0, 3, 2, 3]  # stable: rows ascend
    assert row_offsets.tolist() == [0, 2, 2, 3, 6] and row_slots.tolist() == [0, 2, 4, 1, 3, 5]
    assert out_len.tolist() == [5, 0, 1, 5]
    assert assert_plan(po, pl, goff, 200)[4].tolist() == [10, 0, 1, 11]
    assert assert_plan(po, pl, goff, 0)[4].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("m,G,pmax,seed", [(1, 1, 1, 0), (37, 8, 8, 1), (500, 64, 5, 2), (300, 1000, 40, 3)])
def test_probe_plan_equals_the_restatement(m, G, pmax, seed):
    rs = np.random.RandomState(seed)
    sizes = rs.randint(0, 4, size=G) * rs.randint(1, 300, size=G)  # about a quarter of the groups are empty
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lens = rs.randint(0, pmax + 1, size=m)
    po = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pl = rs.randint(0, G, size=int(po[-1])).astype(np.uint32)  # with replacement: repeats
    pl[rs.rand(pl.size) < 0.1] = NONE
    assert_plan(po, pl, goff, 10)


def test_probe_plan_refuses_a_label_that_is_no_group_and_names_the_row():
    with pytest.raises(_native.PmmError) as ei:
        _native.probe_plan([0, 1, 3], [0, 1, 2], [0, 5, 9], 3)
    assert ei.value.code == _native.PMM_ERR_ARG
    assert "probe_labels[2] = 2" in str(ei.value) and "query row 1" in str(ei.value)


def test_probe_plan_refuses_more_than_2_31_list_entries():
    m = 1 << 17
    po = np.arange(m + 1, dtype=np.int64) * 128
    pl = np.tile(np.arange(128, dtype=np.uint32), m)
    goff = np.arange(129, dtype=np.int64)
    assert _native.probe_plan(po, pl, goff, 128)[0].size == m * 128  # 2^24 slots x 128 = 2^31: the last size served
    with pytest.raises(_native.PmmError) as ei:
        _native.probe_plan(po, pl, goff, 129)
    assert ei.value.code == _native.PMM_ERR_UNSUPPORTED and "split the call" in str(ei.value)


def test_probe_offsets_are_checked_in_python():
    for po in ([0, 2], [1, 2, 3], [0, 2, 1], [0, 1, 2]):
        with pytest.raises(ValueError, match="probe_offsets"):
            _native._probe_lists(po, [0, 0, 0], 2)


# ---- the label encoding and its checks: before any library call ----
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library or of a device helper fails the test."""

    def boom(*a, **k):
        raise AssertionError("library call before the label check")

    for name in ("lib", "topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str",
                 "device_count", "set_devices"):
        monkeypatch.setattr(_native, name, boom)
    return monkeypatch


Q = np.zeros((3, 4), dtype=np.float32)
C = np.zeros((6, 4), dtype=np.float32)


def test_list_labels_are_encoded_against_the_right_side(no_library):
    right = pa.array(["b", "a", None, "b", "c", "a"])
    left = pa.array([["a", "zz", None, "b"], None, []], type=pa.list_(pa.string()))
    for arr in (left, left.cast(pa.large_list(pa.string()))):
        g = pm._check_groups((arr, right), 3, 6)
        assert g.G == 3 and g.clabels.tolist() == [0, 1, NONE, 0, 2, 1]
        assert g.probe_offsets.tolist() == [0, 4, 4, 4]  # a null and an empty list are empty
        assert g.qlabels.tolist() == [1, NONE, NONE, 0]  # an unseen label and a null element match nothing
        assert g.probe_pairs().tolist() == [[0, 0], [1, 0]] and g.searched_max() == 4
    fixed = pa.FixedSizeListArray.from_arrays(pa.array([1, 2, 2, 2, 7, 7], type=pa.int64()), 2)
    g = pm._check_groups((fixed, np.array([2, 2, 1, 5, 5, 5])), 3, 6)
    assert g.probe_offsets.tolist() == [0, 2, 4, 6] and g.qlabels.tolist() == [1, 0, 0, 0, NONE, NONE]
    assert g.probe_pairs().tolist() == [[0, 0], [0, 1], [1, 0]] and g.searched_max() == 3
    sliced = left.cast(pa.large_list(pa.string())).slice(1, 2)  # offsets that do not start at 0
    assert pm._check_groups((sliced, right), 2, 6).probe_offsets.tolist() == [0, 0, 0]


def test_a_label_matrix_is_one_list_per_row(no_library):
    mat = np.array([[3, 3], [1, 9], [1, 3]], dtype=np.int64)
    g = pm._check_groups((mat, np.array([1, 3, 3, 3, 4, 4])), 3, 6)
    assert g.probe_offsets.tolist() == [0, 2, 4, 6] and g.qlabels.tolist() == [1, 1, 0, NONE, 0, 1]
    assert g.searched_max() == 4
    plain = pm._check_groups((np.array([3, 1, 9]), np.array([1, 3, 3, 3, 4, 4])), 3, 6)
    assert plain.probe_offsets is None and plain.qlabels.tolist() == [1, 0, NONE]


def test_probed_refusals_come_before_any_library_call(no_library):
    right = np.arange(6)
    with pytest.raises(ValueError, match="the queries have 3"):
        pm._topk(Q, C, 1, "cosine", groups=(np.zeros((2, 2), dtype=np.int64), right))
    with pytest.raises(TypeError, match="one type"):
        pm._topk(Q, C, 1, "cosine", groups=(pa.array([["a"], [], []]), right))
    with pytest.raises(TypeError, match="integers"):
        pm._topk(Q, C, 1, "cosine", groups=(np.zeros((3, 2)), right))
    with pytest.raises(ValueError, match="cannot be combined"):
        pm._topk(Q, C, 1, "cosine", groups=(np.zeros((3, 2), dtype=np.int64), right), subset=np.ones(6, bool))


# ---- the device call, against a stand-in handle ----
def test_the_device_path_passes_offsets_and_flat_labels(monkeypatch):
    calls = []

    class Handle:
        def topk_probed(self, q, po, pl, k, metric):
            calls.append((q.shape, po.tolist(), pl.tolist(), k, metric))
            m = q.shape[0]
            return (np.full((m, k), 7, np.uint32), np.ones((m, k), np.float32), np.full(m, k, np.uint32))

        def release(self):
            calls.append("release")

    monkeypatch.setattr(pm, "_partitioned_handle", lambda c, original, rv, grp, compute: (Handle(), False))
    monkeypatch.setattr(pm, "_reaccount_cache", lambda dc: calls.append("reaccount"))
    grp = pm._check_groups((np.array([[0, 1], [1, 1]]), np.array([0, 1, 1, 0, 1, 1])), 2, 6)
    idx, sc, lens = pm._topk_grouped(Q[:2], C, None, C, grp, 3, _native.METRIC_DOT, "f32")
    assert calls == [((2, 4), [0, 2, 4], [0, 1, 1, 1], 3, _native.METRIC_DOT), "reaccount", "release"]
    assert idx.shape == (2, 3) and lens.tolist() == [3, 3]
    # k past the entry's limit, Float64 rows: never the handle
    monkeypatch.setattr(pm, "_partitioned_handle", lambda *a: (_ for _ in ()).throw(AssertionError("handle")))
    monkeypatch.setattr(_native, "topk_host", lambda q, c, k, metric, compute=0: (
        np.tile(np.arange(k, dtype=np.uint32), (q.shape[0], 1)), np.zeros((q.shape[0], k), q.dtype)))
    assert pm._topk_probed(np.zeros((2, 4)), np.zeros((6, 4)), None, None, grp, 3, 0, "f32")[2].tolist() == [3, 3]
    big = pm._check_groups((np.zeros((1, 1), dtype=np.int64), np.zeros(200, dtype=np.int64)), 1, 200)
    out = pm._topk_probed(np.zeros((1, 4), np.float32), np.zeros((200, 4), np.float32), None, None, big, 129, 0, "f32")
    assert out[2].tolist() == [129]


# ---- the fallback's merge against the oracle on unions ----
ORACLE_METRIC = {_native.METRIC_COSINE: oracle.COSINE, _native.METRIC_DOT: oracle.DOT,
                 _native.METRIC_EUCLIDEAN: oracle.EUCLIDEAN}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("metric", sorted(ORACLE_METRIC))
def test_fallback_merge_equals_the_oracle_on_the_union(monkeypatch, metric):
    """The per-label searches are the oracle's (no device here); the merge by
    (score, corpus row) must then give the oracle's list on the union --
    duplicates across groups (ties to the lower corpus row, which lies in the
    higher group), a zero row (signed zero scores) and a NaN row included."""
    m, n, d, k, G = 9, 120, 8, 7, 4
    rs = np.random.RandomState(5 + metric)
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    cl = (3 - np.arange(n) % G).astype(np.int64)  # row 0 in group 3, row 3 in group 0
    c[13] = c[22] = c[40] = c[3]  # equal rows in groups 0, 2, 1, 3
    c[50], c[51] = 0.0, np.nan
    q[0], q[1] = c[3], -c[3]
    probes = [[0, 1, 2, 3], [3, 0], [2], [], [1, 1, 2], [0, 1, 2, 3], [3], [0, 2], [1, 3]]
    po = np.concatenate([[0], np.cumsum([len(p) for p in probes])])
    left = pa.ListArray.from_arrays(pa.array(po, type=pa.int32()), pa.array(sum(probes, []), type=pa.int64()))

    def oracle_host(qq, cc, kk, metric_id, compute=0):
        oi, osc = oracle.topk(qq, cc, kk, ORACLE_METRIC[metric_id])
        return np.asarray(oi).astype(np.uint32), np.asarray(osc, dtype=np.float32)

    monkeypatch.setattr(_native, "topk_host", oracle_host)
    monkeypatch.setattr(pm, "_partitioned_handle", lambda *a: (None, False))
    grp = pm._check_groups((left, cl), m, n)
    idx, sc, lens = pm._topk_probed(q, c, None, None, grp, k, metric, "f32")
    for i, p in enumerate(probes):
        ids = np.flatnonzero(np.isin(cl, p))
        kk = min(k, ids.size)
        assert lens[i] == kk
        if kk:
            oi, osc = oracle_host(q[i:i + 1], np.ascontiguousarray(c[ids]), kk, metric)
            assert np.array_equal(idx[i, :kk], ids[oi[0]]), (i, idx[i], ids[oi[0]])
            assert same_bits(sc[i, :kk], osc[0]), (i, sc[i], osc[0])
        assert np.all(idx[i, kk:] == 0xFFFFFFFF) and not np.any(sc[i, kk:].view(np.uint8))
    if metric == _native.METRIC_COSINE:
        assert idx[0, :4].tolist() == [3, 13, 22, 40]  # one score, four groups: ascending corpus row


# ---- the kernels ----
@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_probed_kernels_use_no_scratch():
    # pmm_probed.hip holds the merge (two instantiations) and the grouped
    # kernel's row-table variant (three); the latter within the 128 VGPRs that
    # 16 waves of 1024 threads leave
    from test_kernel_resources import scratch_by_kernel

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "probed.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_probed.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = scratch_by_kernel(asm)
    for want, count in (("grouped_topk_f32_kernel", 3), ("probe_merge_f32_kernel", 2)):
        hits = {k: v for k, v in sc.items() if want in k}
        assert len(hits) == count, f"{want}: {sorted(sc)}"
        assert set(hits.values()) == {(0, 0)}, f"scratch (bytes, instructions): {hits}"
    for name in sc:
        body = asm.split(f".amdhsa_kernel {name}")[1].split(".end_amdhsa_kernel")[0]
        vgpr = [int(l.split()[1]) for l in body.splitlines() if l.strip().startswith(".amdhsa_next_free_vgpr")]
        assert vgpr and vgpr[0] <= 128, (name, vgpr)
    assert "global_atomic" not in asm and "buffer_atomic" not in asm
