"""The int8 route (DESIGN.md §4d "Int8 rows") without a GPU: the cosine key's error bound
restated in NumPy, the header against the exports, the workspace size against
the route, and the dtype routing of ``_topk`` with the device calls stubbed."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import polars_matmul
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pmm.h")

EPS = 2.0 ** -21          # kI8CosEps (pmm_internal.h)
DERIVED = 5.001 * 2.0 ** -24  # five f32 roundings of a value of magnitude <= 1 (DESIGN.md §4d "Int8 rows")


# ---------------------------------------------------------------------------
# The bound.  The kernel's key is a = f32(dot) * (fq * fc) in f32, with
# fq = f32(1 / sqrt(Sq)) from f64; the exact score is the oracle's
# dot / (sqrt(Sq) * sqrt(Sc)) in f64.  |a - s| <= 5.001 * 2^-24 |s| + 2^-50.
# ---------------------------------------------------------------------------
def factor(S):
    S = np.asarray(S, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(S > 0, 1.0 / np.sqrt(S), 0.0).astype(np.float32)


def approx_and_exact(q, c):
    qi, ci = q.astype(np.int64), c.astype(np.int64)
    dot = qi @ ci.T
    Sq, Sc = (qi * qi).sum(1), (ci * ci).sum(1)
    a = dot.astype(np.float32) * (factor(Sq)[:, None] * factor(Sc)[None, :])  # f32 throughout
    assert a.dtype == np.float32
    qn, cn = np.sqrt(Sq.astype(np.float64)), np.sqrt(Sc.astype(np.float64))
    den = qn[:, None] * cn[None, :]
    ok = (qn[:, None] > 1e-10) & (cn[None, :] > 1e-10)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(ok, dot.astype(np.float64) / den, 0.0)
    return a.astype(np.float64), s


def adversarial(d, rs):
    rows = [np.full(d, 127), np.full(d, -128), np.full(d, -127), np.zeros(d, int)]
    alt = np.where(np.arange(d) % 2 == 0, 127, -128)
    rows += [alt, -alt.clip(-127, 127), np.where(np.arange(d) % 2 == 0, 1, -1)]
    for pos, v in ((0, 1), (d - 1, -128), (d // 2, 127), (0, -1)):  # one non-zero element
        e = np.zeros(d, int)
        e[pos] = v
        rows.append(e)
    # near-orthogonal pairs: dot = +-1 against large norms
    h = np.where(rs.rand(d) < 0.5, 127, -128)
    g = h.copy()
    g[1::2] = -g[1::2].clip(-127, 127)
    rows += [h, g]
    rows += list(rs.randint(-128, 128, size=(24, d)))
    rows += list(rs.randint(-1, 2, size=(8, d)))
    return np.array(rows, dtype=np.int8)


@pytest.mark.parametrize("d", (1, 2, 37, 64, 257, 768, 1536, 2048, 65535))
def test_cosine_key_error_bound(d):
    rs = np.random.RandomState(d)
    x = adversarial(d, rs)
    a, s = approx_and_exact(x, x)
    err = np.abs(a - s)
    assert np.all(err <= DERIVED * np.abs(s) + 2.0 ** -50), float(err.max())
    assert float(err.max()) < EPS and float(np.abs(s).max()) <= 1.0 + 2.0 ** -50
    assert np.all(a[s == 0.0] == 0.0)  # a zero row or an orthogonal pair: the key is exactly 0


def test_band_keeps_every_member_of_the_exact_topk():
    """The kernel's rule on the NumPy restatement: with a_k the k-th best key,
    every entry of the exact top k (f64 score, then lower index) has a key at
    or above f32(a_k - 2 eps)."""
    rs = np.random.RandomState(3)
    base = rs.randint(-3, 4, size=(60, 48)).astype(np.int8)
    c = base[rs.randint(0, 60, size=800)]          # many equal rows
    c[::7] = np.clip(c[::7].astype(int) * 2, -128, 127)  # and their multiples: equal cosines from other integers
    q = rs.randint(-3, 4, size=(16, 48)).astype(np.int8)
    a, s = approx_and_exact(q, c)
    for k in (1, 10, 100):
        for i in range(q.shape[0]):
            order = np.lexsort((np.arange(c.shape[0]), -s[i]))[:k]
            a_k = np.sort(a[i])[::-1][k - 1]
            thr = np.float32(np.float32(a_k) - np.float32(2 * EPS))
            assert np.all(a[i][order] >= thr), (k, i)


def test_euclidean_and_dot_keys_are_exact():
    """Distinct squared distances below 2^32 have distinct f64 square roots, so
    the integer key orders as the f64 score does; the largest one fits in u32."""
    assert 255 * 255 * 65535 < 2 ** 32 and 128 * 128 * 65535 < 2 ** 31
    top = np.arange(2 ** 32 - 4096, 2 ** 32, dtype=np.float64)
    assert np.all(np.diff(np.sqrt(top)) > 0)
    low = np.arange(0, 1 << 16, dtype=np.float64)
    assert np.all(np.diff(np.sqrt(low)) > 0)


# ---------------------------------------------------------------------------
# The boundary
# ---------------------------------------------------------------------------
I8_SYMBOLS = ("pmm_corpus_create_i8", "pmm_topk_i8", "pmm_topk_i8_corpus", "pmm_topk_i8_device",
              "pmm_topk_i8_workspace_bytes")


def test_int8_header_symbols_are_bound_and_exported():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(pmm_\w*i8\w*)\s*\(", text, flags=re.M)))
    assert declared == sorted(I8_SYMBOLS)
    assert re.search(r"^#define PMM_DTYPE_I8 3$", text, flags=re.M) and _native.DTYPE_I8 == 3
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name


def al256(x):
    return (x + 255) & ~255


def native_bytes(m, n, k, cap=None):
    """route_i8's native layout restated (pmm_capi.hip)."""
    p2 = 64
    while p2 < 4 * min(k, 1024) + 256:
        p2 *= 2
    cap = cap or min(4096, max(1024, p2))
    mc = max(1, min(m, (1 << 30) // (cap * 16)))
    return (256 + 2 * al256(4 * m) + 2 * al256(4 * n) + 4 * al256(4 * mc) + al256(4 * m) + al256(mc * cap * 16))


def test_workspace_bytes_follow_the_route(monkeypatch):
    ws = _native.i8_workspace_bytes
    monkeypatch.delenv("PMM_I8_CAP", raising=False)
    m, n = 70, 3001
    for d, k in ((1, 1), (768, 100), (1536, 1000), (2048, 1024), (1985, 1024)):  # the last pads to 2048: still native
        assert ws(m, n, d, k, 0) == native_bytes(m, n, k), (d, k)
    assert ws(1 << 20, 1000, 64, 1024, 0) == native_bytes(1 << 20, 1000, 1024)  # several passes of mc rows
    # past either limit: both sides widened to f64 next to the f64 path's own workspace
    for d, k in ((2049, 10), (4096, 10), (64, 1025), (2048, 3001)):
        dp64 = -(-d // 16) * 16
        assert ws(m, n, d, k, 0) > al256(m * dp64 * 8) + al256(n * dp64 * 8), (d, k)
    assert ws(m, n, 2049, 10, 0) > ws(m, n, 2048, 10, 0)
    # one decision per call: the environment is read when the route is planned
    monkeypatch.setenv("PMM_I8_CAP", "64")
    assert ws(m, n, 64, 10, 0) == native_bytes(m, n, 10, cap=64) < native_bytes(m, n, 10)
    monkeypatch.setenv("PMM_I8_CAP", "100")  # not a power of two: ignored
    assert ws(m, n, 64, 10, 0) == native_bytes(m, n, 10)
    # refused or empty problems need nothing
    assert ws(0, n, 64, 10, 0) == ws(m, n, 65536, 10, 0) == ws(m, n, 64, 0, 0) == 0


def test_int8_corpus_device_bytes():
    assert _native.corpus_device_bytes(1000, 768, np.int8) == 1000 * 768 + 8000
    assert _native.corpus_device_bytes(10, 1, np.int8) == 10 * 64 + 80
    # a 1M x 768 column: under a sixth of the f64 handle it took before
    assert 6 * _native.corpus_device_bytes(1 << 20, 768, np.int8) < _native.corpus_device_bytes(1 << 20, 768, np.float64)
    assert 6 * _native.corpus_device_bytes(1 << 20, 256, np.int8) < _native.corpus_device_bytes(1 << 20, 256, np.float64)


# ---------------------------------------------------------------------------
# Routing by dtype, the device calls stubbed
# ---------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def fake(name):
        def run(q, c, k, metric, compute=_native.COMPUTE_F32):
            seen.append((name, q.dtype.name, c.dtype.name, compute))
            return np.zeros((q.shape[0], k), np.uint32), np.zeros((q.shape[0], k), np.float64)
        return run

    monkeypatch.setattr(_native, "topk_i8_host", fake("i8"))
    monkeypatch.setattr(_native, "topk_host", fake("host"))
    monkeypatch.setattr(pm, "_cached_corpus", lambda *a, **k: None)
    monkeypatch.setattr(pm, "_apply_devices_env", lambda: None)
    monkeypatch.setattr(_native, "get_devices", lambda: [])
    monkeypatch.setattr(pm, "_topk_subset", lambda q, c, *a: (seen.append(("subset", q.dtype.name, c.dtype.name, 0)),
                                                              (np.zeros((q.shape[0], a[3]), np.uint32),
                                                               np.zeros((q.shape[0], a[3]), np.float64)))[1])
    return seen


def col(rows, t, fixed=False):
    return pa.array(rows, type=pa.list_(t, len(rows[0])) if fixed else pa.list_(t))


Q = [[1, -2, 3], [0, 0, 1]]
C = [[1, 2, 3], [-128, 127, 0], [4, None, 6]]


@pytest.mark.parametrize("fixed", (False, True))
def test_int8_columns_take_the_int8_entry(calls, fixed):
    out = pm._topk(col(Q, pa.int8(), fixed), col(C, pa.int8(), fixed), 2, "cosine")
    assert calls == [("i8", "int8", "int8", _native.COMPUTE_F32)]
    assert out.type == pa.large_list(pa.struct([("index", pa.uint32()), ("score", pa.float64())]))


def test_int8_matrices_take_the_int8_entry(calls):
    q, c = np.array(Q, np.int8), np.array([[1, 2, 3], [4, 5, 6]], np.int8)
    pm._topk(q, c, 2, "dot")
    polars_matmul.topk(q, c, 2, "dot")
    assert calls == [("i8", "int8", "int8", _native.COMPUTE_F32)] * 2


@pytest.mark.parametrize("lt,rt", [(pa.int8(), pa.float32()), (pa.float64(), pa.int8()), (pa.uint8(), pa.uint8()),
                                   (pa.int16(), pa.int16()), (pa.int8(), pa.int16()), (pa.int8(), pa.uint8()),
                                   (pa.int64(), pa.int8())])
def test_other_integer_and_mixed_columns_keep_the_f64_route(calls, lt, rt):
    q = [[1, 2, 3], [0, 0, 1]]  # (values every one of these types holds)
    c = [[1, 2, 3], [100, 127, 0], [4, None, 6]]
    pm._topk(col(q, lt), col(c, rt), 2, "cosine")
    assert calls == [("host", "float64", "float64", _native.COMPUTE_F32)]


def test_int8_with_bf16_subset_groups_or_a_device_list_keeps_today_s_route(calls, monkeypatch):
    q8, c8 = col(Q, pa.int8()), col(C, pa.int8())
    pm._topk(q8, c8, 2, "cosine", compute="bf16")
    assert calls.pop() == ("host", "float32", "float32", _native.COMPUTE_BF16)
    pm._topk(q8, c8, 2, "cosine", subset=np.array([0, 2]))
    assert calls.pop() == ("subset", "float64", "float64", 0)
    monkeypatch.setattr(pm, "_topk_grouped", lambda q, c, *a: (calls.append(("grouped", q.dtype.name, c.dtype.name, 0)),
                                                               (np.zeros((2, 1), np.uint32), np.zeros((2, 1), np.float64),
                                                                np.ones(2, np.uint32)))[1])
    pm._topk(q8, c8, 1, "cosine", groups=(np.array([0, 1]), np.array([0, 1, 1])))
    assert calls.pop() == ("grouped", "float64", "float64", 0)
    qm, cm = np.array(Q, np.int8), np.array([[1, 2, 3], [4, 5, 6]], np.int8)
    polars_matmul.topk(qm, cm, 1, "dot", compute="bf16")
    assert calls.pop() == ("host", "float32", "float32", _native.COMPUTE_BF16)
    monkeypatch.setattr(_native, "get_devices", lambda: [0, 1])
    pm._topk(q8, c8, 2, "cosine")
    polars_matmul.topk(qm, cm, 1, "dot")
    assert calls == [("host", "float64", "float64", _native.COMPUTE_F32)] * 2


def test_int8_extraction_borrows_array_children_and_zeroes_nulls():
    vals = pa.array(np.arange(-6, 6, dtype=np.int8))
    arr = pa.FixedSizeListArray.from_arrays(vals, 4)
    m = pm._series_to_matrix(arr, np.int8)
    assert m.dtype == np.int8 and m.shape == (3, 4)
    assert m.ctypes.data == vals.buffers()[1].address  # zero-copy
    m = pm._series_to_matrix(col(C, pa.int8()), np.int8)
    assert m.dtype == np.int8 and m.tolist() == [[1, 2, 3], [-128, 127, 0], [4, 0, 6]]
    assert pm._is_i8(arr) and not pm._is_i8(col(C, pa.uint8()) if False else pa.array([[1]], type=pa.list_(pa.uint8())))


def test_the_int8_handle_refuses_other_queries():
    # (the check comes before the library is called)
    dc = _native.DeviceCorpus.__new__(_native.DeviceCorpus)
    dc.dtype, dc.d = np.dtype(np.int8), 3
    with pytest.raises(TypeError, match="int8 queries"):
        dc.topk(np.zeros((1, 3), np.float32), 1, 0)
    dc._h = None  # (nothing to free)
    dc._lock, dc._refs, dc._closing = __import__("threading").Lock(), 0, True
