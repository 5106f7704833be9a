"""Bit rows without a GPU (DESIGN.md §4d "Bit rows"): the packing definition on
special values, the restatement the GPU tests compare with and its tie rule,
the boundary (header, exports, workspace and handle byte formulas), the dtype
and shape refusals, the Arrow extraction, the untouched UInt8 route of
``.pmm.topk``, the namespace methods against a stand-in ``polars`` and the
resource report of pmm_bits.hip compiled for gfx950."""
from __future__ import annotations

import ctypes
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
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pmm.h")


# ---------------------------------------------------------------------------
# The restatement (shared with tests/test_gpu_bits.py)
# ---------------------------------------------------------------------------
def hamming_truth(q, c, k):
    """(indices uint32 (m, k), distances float64 (m, k)): the bits unpacked,
    integer distances, a stable sort by distance -- ties keep the lower index."""
    qb = np.unpackbits(q, axis=1, bitorder="little").astype(np.int32)
    cb = np.unpackbits(c, axis=1, bitorder="little").astype(np.int32)
    dist = qb.sum(1)[:, None] + cb.sum(1)[None, :] - 2 * (qb @ cb.T)
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return order.astype(np.uint32), np.take_along_axis(dist, order, 1).astype(np.float64)


def special_rows(d):
    """Rows of d floats that walk through every special value at every bit position."""
    tiny = np.float32(1e-45)  # the least subnormal
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny, 1.0, -1.0, np.float32(1e-40), -np.float32(1e-40),
                     3.4e38, -3.4e38], dtype=np.float32)
    rows = np.stack([np.roll(np.resize(vals, d + len(vals)), s)[:d] for s in range(len(vals))])
    return np.ascontiguousarray(rows, dtype=np.float32)


WANT_BIT = {"0.0": 0, "-0.0": 0, "nan": 0, "inf": 1, "-inf": 0, "1e-45": 1, "-1e-45": 0, "1.0": 1, "-1.0": 0}


def test_pack_sign_special_values_one_by_one():
    for text, bit in WANT_BIT.items():
        x = np.array([[float(text)]], dtype=np.float32)
        assert polars_matmul.pack_sign(x).tolist() == [[bit]], text
    assert np.float32(1e-45) > 0 and np.float32(1e-45) < np.finfo(np.float32).tiny  # (a subnormal)


@pytest.mark.parametrize("d", [1, 7, 8, 9, 63, 64, 65, 1000])
def test_pack_sign_bit_order_and_zero_tail(d):
    x = special_rows(d)
    p = polars_matmul.pack_sign(x)
    w = -(-d // 8)
    assert p.dtype == np.uint8 and p.shape == (x.shape[0], w)
    for r in range(x.shape[0]):
        for j in range(8 * w):
            want = 1 if (j < d and x[r, j] > 0) else 0  # NaN > 0 is False
            assert (int(p[r, j >> 3]) >> (j & 7)) & 1 == want, (r, j)
    one = np.zeros((1, d), np.float32)
    one[0, d - 1] = 2.0  # the last element alone: bit (d - 1) & 7 of the last byte
    last = polars_matmul.pack_sign(one)
    assert last[0, -1] == 1 << ((d - 1) & 7) and not last[0, :-1].any()


def test_restatement_tie_rule_by_hand():
    c = np.array([[0b0000_0001], [0b0000_0010], [0b0000_0000], [0b0000_0011], [0b0000_0010]], np.uint8)
    q = np.array([[0b0000_0010], [0b1111_1111]], np.uint8)
    idx, dist = hamming_truth(q, c, 4)
    # row 0: distances 2 0 1 1 0 -> 1, 4 (tie: lower first), then 2, 3 (tie)
    assert idx[0].tolist() == [1, 4, 2, 3] and dist[0].tolist() == [0.0, 0.0, 1.0, 1.0]
    # row 1: distances 7 7 8 6 7 -> 3, then 0, 1, 4 (a three-way tie, the k-th place included)
    assert idx[1].tolist() == [3, 0, 1, 4] and dist[1].tolist() == [6.0, 7.0, 7.0, 7.0]


# ---------------------------------------------------------------------------
# The boundary
# ---------------------------------------------------------------------------
BITS_SYMBOLS = ("pmm_pack_sign_device", "pmm_corpus_create_bits", "pmm_corpus_sign_bits", "pmm_corpus_bits_rows", "pmm_topk_bits",
                "pmm_topk_bits_corpus", "pmm_topk_bits_workspace_bytes", "pmm_topk_bits_device")


def test_bits_header_symbols_are_bound_and_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(pmm_\w+)\s*\(", text, flags=re.M))
    assert set(BITS_SYMBOLS) <= declared
    assert re.search(r"^#define PMM_DTYPE_BITS 4$", text, flags=re.M) and _native.DTYPE_BITS == 4
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in BITS_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name


def al256(x):
    return (x + 255) & ~255


def native_bytes(m, n, w, k, cap=None):
    """route_bits' native layout restated (pmm_capi.hip)."""
    p2 = 64
    while p2 < 4 * min(k, 1024) + 256:
        p2 *= 2
    cap = cap or min(4096, max(1024, p2))
    mc = max(1, min(m, (1 << 30) // (cap * 16)))
    dp = -(-w // 16) * 16
    return (al256(4) + al256(4 * m) + al256(4 * n) + 4 * al256(4 * mc) + al256(4 * m) + al256(m * dp) + al256(4 * m)
            + al256(mc * cap * 16))


def test_workspace_bytes_follow_the_route(monkeypatch):
    ws = _native.bits_workspace_bytes
    monkeypatch.delenv("PMM_BITS_CAP", raising=False)
    m, n = 70, 3001
    for w, k in ((1, 1), (32, 100), (96, 1000), (8192, 1024), (129, 1024)):
        assert ws(m, n, w, k) == native_bytes(m, n, w, k), (w, k)
    assert ws(1 << 20, 1000, 32, 1024) == native_bytes(1 << 20, 1000, 32, 1024)  # several passes of mc rows
    # past k = 1024: both sides expanded to f64 next to the f64 path's own workspace
    for w, k in ((32, 1025), (7, 3001)):
        dp64 = -(-8 * w // 16) * 16
        assert ws(m, n, w, k) > al256(m * dp64 * 8) + al256(n * dp64 * 8), (w, k)
    # one decision per call: the environment is read when the route is planned
    monkeypatch.setenv("PMM_BITS_CAP", "64")
    assert ws(m, n, 32, 10) == native_bytes(m, n, 32, 10, cap=64) < native_bytes(m, n, 32, 10)
    assert ws(m, n, 32, 64) == native_bytes(m, n, 32, 64)  # (no room for a chunk beside k entries: ignored)
    monkeypatch.setenv("PMM_BITS_CAP", "100")  # not a power of two: ignored
    assert ws(m, n, 32, 10) == native_bytes(m, n, 32, 10)
    # refused or empty problems need nothing
    assert ws(0, n, 32, 10) == ws(m, n, 8193, 10) == ws(m, n, 32, 0) == 0


def test_handle_byte_formula():
    assert _native.bits_device_bytes(1000, 96) == 1000 * 96 + 4000
    assert _native.bits_device_bytes(10, 1) == 10 * 16 + 40
    assert _native.bits_device_bytes(7, 17) == 7 * 32 + 28
    # a 1M x 1024 corpus: 1/32 of the f32 handle's rows, under an eighth of the int8 handle
    n, d = 1 << 20, 1024
    assert _native.bits_device_bytes(n, d // 8) == n * 128 + 4 * n
    assert 30 * _native.bits_device_bytes(n, d // 8) < _native.corpus_device_bytes(n, d, np.float32)
    assert 7 * _native.bits_device_bytes(n, d // 8) < _native.corpus_device_bytes(n, d, np.int8)


# ---------------------------------------------------------------------------
# Refusals (each before the library is called)
# ---------------------------------------------------------------------------
def test_dtype_and_shape_refusals():
    u8 = np.zeros((2, 4), np.uint8)
    for bad in (np.zeros((2, 4), np.int8), np.zeros((2, 4), np.float32), np.zeros((2, 4), bool)):
        with pytest.raises(TypeError, match="UInt8 columns of packed bits"):
            polars_matmul.topk_hamming(bad, u8, 1)
        with pytest.raises(TypeError, match="UInt8 columns of packed bits"):
            pm._topk_hamming(u8, bad, 1)
        with pytest.raises(TypeError, match="2-D uint8 array of packed bits"):
            _native.topk_bits_host(bad, u8, 1)
        with pytest.raises(TypeError, match="DeviceCorpus.bits takes a 2-D uint8 array"):
            _native.DeviceCorpus.bits(bad)
    with pytest.raises(TypeError, match="UInt8 columns of packed bits"):
        pm._topk_hamming(pa.array([[1.0, 2.0]], type=pa.list_(pa.float32())), u8, 1)
    with pytest.raises(TypeError, match="2-D"):
        polars_matmul.topk_hamming(np.zeros(4, np.uint8), u8, 1)
    with pytest.raises(TypeError, match="2-D uint8 array"):
        _native.DeviceCorpus.bits(np.zeros(4, np.uint8))
    text = "Dimension mismatch: left has 4 dimensional vectors, right has 5 dimensional vectors"
    with pytest.raises(RuntimeError, match=text):
        polars_matmul.topk_hamming(u8, np.zeros((3, 5), np.uint8), 1)
    with pytest.raises(RuntimeError, match=text):
        pm._topk_hamming(u8, np.zeros((3, 5), np.uint8), 1)
    with pytest.raises(TypeError, match="sign_bits takes a Float32 column"):
        pm._sign_bits(np.zeros((2, 4), np.float64))
    with pytest.raises(TypeError, match="2-D"):
        polars_matmul.pack_sign(np.zeros(4, np.float32))
    # the empty cases never reach a device
    idx, sc = polars_matmul.topk_hamming(u8, np.zeros((3, 4), np.uint8), 0)
    assert idx.shape == (2, 0) and idx.dtype == np.uint32 and sc.shape == (2, 0) and sc.dtype == np.float64
    out = pm._topk_hamming(pa.array([], type=pa.list_(pa.uint8())), u8, 3)
    assert len(out) == 0 and out.type == pa.large_list(pa.struct([("index", pa.uint32()), ("score", pa.float64())]))


def test_the_bit_handle_refuses_other_queries():
    # (DeviceCorpus.topk on a bit corpus passes its queries through this check before the library is called)
    for bad in (np.zeros((1, 3), np.int8), np.zeros((1, 3), np.float32), np.zeros((1, 4), np.uint8), np.zeros(3, np.uint8)):
        with pytest.raises(TypeError, match="a bit corpus takes a 2-D uint8 array of packed bits of 3 bytes a row"):
            _native._bit_rows(bad, "a bit corpus", 3)
    ok = np.zeros((2, 3), np.uint8)[:, ::1]
    assert _native._bit_rows(ok, "a bit corpus", 3).flags.c_contiguous


# ---------------------------------------------------------------------------
# Extraction and routing, the device calls stubbed
# ---------------------------------------------------------------------------
def test_bit_extraction_borrows_array_children_and_zeroes_nulls():
    vals = pa.array(np.arange(200, 212, dtype=np.uint8))
    arr = pa.FixedSizeListArray.from_arrays(vals, 4)
    m = pm._series_to_matrix(arr, np.uint8)
    assert m.dtype == np.uint8 and m.shape == (3, 4)
    assert m.ctypes.data == vals.buffers()[1].address  # zero-copy
    rows = pa.array([[1, 2, 3], None, [255, None, 6]], type=pa.list_(pa.uint8(), 3))
    m = pm._series_to_matrix(rows, np.uint8)
    assert m.dtype == np.uint8 and m.tolist() == [[1, 2, 3], [0, 0, 0], [255, 0, 6]]
    assert pm._is_u8(arr) and pm._is_u8(np.zeros((1, 1), np.uint8))
    assert not pm._is_u8(pa.array([[1]], type=pa.list_(pa.int8()))) and not pm._is_u8(np.zeros((1, 1), np.int8))


@pytest.fixture
def recorded(monkeypatch):
    seen = []

    def fake(name):
        def run(q, c, k, *a, **kw):
            seen.append((name, q.dtype.name, c.dtype.name, q.shape, c.shape, k))
            return np.zeros((q.shape[0], k), np.uint32), np.zeros((q.shape[0], k), np.float64)
        return run

    for name in ("topk_host", "topk_i8_host", "topk_bits_host"):
        monkeypatch.setattr(_native, name, fake(name))
    monkeypatch.setattr(pm, "_cached_corpus", lambda *a, **k: None)
    monkeypatch.setattr(pm, "_apply_devices_env", lambda: None)
    monkeypatch.setattr(_native, "get_devices", lambda: [])
    return seen


def test_uint8_columns_on_topk_keep_the_f64_route_and_hamming_takes_the_bits(recorded):
    q = pa.array([[1, 2, 3], [0, 0, 1]], type=pa.list_(pa.uint8()))
    c = pa.array([[1, 2, 3], [200, 127, 0], [4, None, 6]], type=pa.list_(pa.uint8(), 3))
    pm._topk(q, c, 2, "euclidean")
    polars_matmul.topk(np.zeros((2, 3), np.uint8), np.zeros((4, 3), np.uint8), 2, "euclidean")
    assert [r[:3] for r in recorded] == [("topk_host", "float64", "float64")] * 2  # read as numbers, widened
    del recorded[:]
    out = pm._topk_hamming(q, c, 5)  # k clips to n
    assert recorded == [("topk_bits_host", "uint8", "uint8", (2, 3), (3, 3), 3)]
    assert out.type == pa.large_list(pa.struct([("index", pa.uint32()), ("score", pa.float64())])) and len(out) == 2
    assert [len(r) for r in out.to_pylist()] == [3, 3]
    idx, sc = polars_matmul.topk_hamming(np.zeros((2, 3), np.uint8), np.zeros((4, 3), np.uint8), 9)
    assert recorded[-1] == ("topk_bits_host", "uint8", "uint8", (2, 3), (4, 3), 4) and idx.shape == sc.shape == (2, 4)


def test_sign_bits_column_is_pack_sign_of_the_rows():
    x = special_rows(19)
    col = pa.FixedSizeListArray.from_arrays(pa.array(x.reshape(-1)), 19)
    out = pm._sign_bits(col)
    assert out.type == pa.list_(pa.uint8(), 3)
    got = np.asarray(out.values.to_numpy()).reshape(len(x), 3)
    assert np.array_equal(got, polars_matmul.pack_sign(x))
    ragged = pa.array([[1.0, -1.0, 2.0], None], type=pa.list_(pa.float32()))
    assert pm._sign_bits(ragged).to_pylist() == [[0b101], [0]]
    assert np.array_equal(np.asarray(pm._sign_bits(x).values.to_numpy()).reshape(len(x), 3), polars_matmul.pack_sign(x))


# ---------------------------------------------------------------------------
# The namespace methods against a stand-in polars (tests/test_namespace.py's)
# ---------------------------------------------------------------------------
NS_SCRIPT = r'''
import json, sys, types
sys.path.insert(0, %(pkg)r)
pl = types.ModuleType("polars")
class _DT:
    def __init__(self, name, *args):
        self.name, self.args = name, args
    def __eq__(self, o):
        return isinstance(o, _DT) and (self.name, self.args) == (o.name, o.args)
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
ns = registry["pmm"]
calls = []
polars_matmul._topk_hamming = lambda s, c, k: calls.append(("topk_hamming", s, len(c), k)) or "hamming-result"
polars_matmul._sign_bits = lambda s: calls.append(("sign_bits", s)) or "bits-result"
out = {}
e = Expr(); ns(e).topk_hamming(Series([[1, 2]] * 3), 40)
fn, kw = e.calls[0]
out["hamming_kw"] = {"is_elementwise": kw["is_elementwise"],
                     "dtype_ok": kw["return_dtype"] == pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64}))}
out["hamming_result"] = fn("batch")
out["hamming_call"] = list(calls[-1])
try:
    ns(Expr()).topk_hamming(Expr(), 1)
    out["expr_error"] = None
except TypeError as err:
    out["expr_error"] = str(err)
e = Expr(); ns(e).sign_bits()
fn, kw = e.calls[0]
out["sign_kw"] = {"is_elementwise": kw["is_elementwise"], "has_dtype": "return_dtype" in kw}
out["sign_result"] = fn("b2")
out["sign_call"] = list(calls[-1])
print(json.dumps(out))
'''


def test_namespace_methods_against_the_stub_polars():
    pkg = os.path.join(ROOT, "polars-matmul_amd")
    r = subprocess.run([sys.executable, "-c", NS_SCRIPT % {"pkg": pkg}], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["hamming_kw"] == {"is_elementwise": True, "dtype_ok": True}
    assert out["hamming_result"] == "hamming-result" and out["hamming_call"] == ["topk_hamming", "batch", 3, 40]
    assert out["expr_error"] and "must be a Polars Series" in out["expr_error"]
    assert out["sign_kw"] == {"is_elementwise": True, "has_dtype": False}
    assert out["sign_result"] == "bits-result" and out["sign_call"] == ["sign_bits", "b2"]


# ---------------------------------------------------------------------------
# Code generation (after tests/test_kernel_resources_range.py)
# ---------------------------------------------------------------------------
def test_bit_kernels_use_no_scratch():
    from isa_util import CSRC, FLAGS, HIPCC, have_hipcc
    from test_kernel_resources import scratch_by_kernel

    if not have_hipcc():
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bits.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_bits.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = scratch_by_kernel(asm)
    for want in ("pack_sign_kernel", "bits_popcount_kernel", "gemm_bits_topk_kernel", "bits_finish_kernel",
                 "bits_gather_kernel", "bits_widen_kernel", "bits_square_kernel"):
        hits = {k: v for k, v in sc.items() if want in k}
        assert hits, f"{want} not in pmm_bits.hip's assembly: {sorted(sc)}"
        assert set(hits.values()) == {(0, 0)}, f"scratch (bytes, instructions): {hits}"
    assert "v_mfma_i32_16x16x64_i8" in asm
