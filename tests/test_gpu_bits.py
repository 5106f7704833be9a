"""Bit rows on the GPU (DESIGN.md §4d "Bit rows"): every list -- indices and
f64 score bits -- against the NumPy restatement of tests/test_bits_cpu.py
(bits unpacked, integer distances, stable sort by (distance, index)); the
device packing against ``pack_sign`` byte for byte."""
from __future__ import annotations

import os

import numpy as np
import pytest

import polars_matmul
from polars_matmul import _native
from polars_matmul import _polars_matmul as pm
from test_bits_cpu import hamming_truth, special_rows

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F, 0x01)


@pytest.fixture
def env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    assert _native.device_count() > 0, "no HIP device visible"
    return monkeypatch


def bit_rows(rs, rows, w):
    return np.ascontiguousarray(rs.randint(0, 256, size=(rows, w)).astype(np.uint8))


def assert_lists(got, want, label):
    gi, gs = got
    wi, ws = want
    assert gi.dtype == np.uint32 and gs.dtype == np.float64 and gi.shape == wi.shape and gs.shape == ws.shape, label
    if not np.array_equal(gs.view(np.uint64), ws.view(np.uint64)):
        bad = np.argwhere(gs.view(np.uint64) != ws.view(np.uint64))[0]
        raise AssertionError(f"{label}: score at {tuple(bad)} is {gs[tuple(bad)]!r}, not {ws[tuple(bad)]!r}")
    if not np.array_equal(gi, wi):
        bad = np.argwhere(gi != wi)[0]
        raise AssertionError(f"{label}: index at {tuple(bad)} is {gi[tuple(bad)]}, not {wi[tuple(bad)]}")


# ---------------------------------------------------------------------------
# Shapes at the kernel's edges.  m: the 128-row tile; n: the 128-column tile
# and the chunk boundaries; w: the 8-byte K step (w % 8), the 16-byte staging
# group (w % 16) and several groups; k: one, a list, the buffer (1024), n.
# chunk_schedule (pmm_capi.hip) for k = 10: cap = 1024, first chunk s0 = 512,
# growth g = floor((1024 - 10) / (10 + 23 + sqrt(529 + 460))) = 15, so the
# chunks end at 512, 512 + 15 * 512 = 8192, ...: n = 9000 is past the second
# boundary.  For k = 100: g = 4, boundaries 512 and 2560 -- n = 3000 is past it.
# ---------------------------------------------------------------------------
SHAPES = [
    # (m, n, w, k)
    (1, 1, 1, 1), (1, 127, 7, 10), (1, 3000, 8, 100), (1, 129, 384, 129),
    (70, 1, 9, 1), (70, 127, 1, 127), (70, 129, 96, 100), (70, 3000, 129, 1024), (70, 3000, 7, 10),
    (129, 127, 8, 1), (129, 129, 129, 10), (129, 3000, 96, 100), (129, 3000, 9, 3000), (129, 1, 384, 1),
    (257, 127, 96, 127), (257, 129, 9, 129), (257, 3000, 384, 10), (257, 3000, 1, 100), (257, 3000, 8, 1024),
    (257, 129, 7, 1), (1, 3000, 96, 1024), (70, 129, 8, 10), (129, 127, 384, 100), (257, 1, 129, 1),
    (70, 9000, 96, 10), (129, 9000, 9, 10),  # past the second chunk boundary of k = 10 (8192)
    (33, 3000, 17, 100), (33, 3000, 16, 100), (33, 3000, 15, 100), (33, 3000, 33, 100),  # around the staging group
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_at_the_kernel_edges(env, shape):
    m, n, w, k = shape
    rs = np.random.RandomState(m + 3 * n + 7 * w + k)
    q, c = bit_rows(rs, m, w), bit_rows(rs, n, w)
    assert_lists(_native.topk_bits_host(q, c, k), hamming_truth(q, c, k), f"host entry {shape}")


# ---------------------------------------------------------------------------
# Ties
# ---------------------------------------------------------------------------
def tie_corpus(rs, w=12):
    """3000 rows drawn from 40 patterns: every place of a list is tied many ways."""
    patterns = bit_rows(rs, 40, w)
    return np.ascontiguousarray(patterns[rs.randint(0, 40, size=3000)]), patterns


@pytest.mark.parametrize("k", [1, 10, 100, 1024])
def test_forty_patterns_tie_at_every_place(env, k):
    rs = np.random.RandomState(40 + k)
    c, patterns = tie_corpus(rs)
    q = np.ascontiguousarray(np.concatenate([patterns[:20], bit_rows(rs, 50, 12)]))  # (20 rows at distance 0 of many)
    want = hamming_truth(q, c, k)
    assert want[1][0, 0] == 0.0
    assert_lists(_native.topk_bits_host(q, c, k), want, f"tie corpus k={k}")


def test_identical_rows_zero_and_ones_rows(env):
    rs = np.random.RandomState(5)
    row = bit_rows(rs, 1, 24)
    c = np.ascontiguousarray(np.repeat(row, 700, axis=0))
    q = np.ascontiguousarray(np.concatenate([row, ~row, np.zeros((1, 24), np.uint8), np.full((1, 24), 255, np.uint8),
                                             bit_rows(rs, 3, 24)]))
    got = _native.topk_bits_host(q, c, 100)
    assert_lists(got, hamming_truth(q, c, 100), "identical rows")
    assert got[0][0].tolist() == list(range(100)) and got[1][0].tolist() == [0.0] * 100
    assert got[1][1].tolist() == [192.0] * 100  # the complement: every bit differs
    c2 = np.ascontiguousarray(np.concatenate([np.zeros((300, 24), np.uint8), np.full((300, 24), 255, np.uint8),
                                              bit_rows(rs, 400, 24)]))
    assert_lists(_native.topk_bits_host(q, c2, 350), hamming_truth(q, c2, 350), "all-zero and all-ones rows")


def test_one_byte_rows_have_nine_distances(env):
    rs = np.random.RandomState(9)
    q, c = np.arange(256, dtype=np.uint8)[:, None].copy(), bit_rows(rs, 3000, 1)
    got = _native.topk_bits_host(q, c, 100)
    assert_lists(got, hamming_truth(q, c, 100), "w = 1")
    assert set(np.unique(got[1])) <= set(float(x) for x in range(9))


# ---------------------------------------------------------------------------
# Routes
# ---------------------------------------------------------------------------
def test_forced_overflow_returns_the_same_lists(env):
    rs = np.random.RandomState(64)
    c, patterns = tie_corpus(rs)
    q = np.ascontiguousarray(np.concatenate([patterns[:30], bit_rows(rs, 40, 12)]))
    # ascending quality: every later chunk beats the buffer of a far query, so 64-entry buffers overflow
    far = hamming_truth(q[:1], c, 3000)[0][0][::-1]
    c = np.ascontiguousarray(c[far])
    want = hamming_truth(q, c, 10)
    clean = _native.topk_bits_host(q, c, 10)
    assert_lists(clean, want, "clean")
    env.setenv("PMM_BITS_CAP", "64")
    _native.timing_enable(True)
    try:
        _native.timing_reset()
        got = _native.topk_bits_host(q, c, 10)
        assert _native.timing_read("bits_gather")[1] >= 1, "no row overflowed: the re-run did not happen"
    finally:
        _native.timing_enable(False)
        _native.timing_reset()
    assert_lists(got, want, "PMM_BITS_CAP=64")


def test_widened_route_past_k_1024(env):
    rs = np.random.RandomState(1500)
    q, (c, _) = bit_rows(rs, 33, 12), tie_corpus(rs)
    assert_lists(_native.topk_bits_host(q, c, 1500), hamming_truth(q, c, 1500), "k = 1500 on the tie corpus")
    q, c = bit_rows(rs, 33, 9), bit_rows(rs, 3000, 9)
    assert_lists(_native.topk_bits_host(q, c, 1500), hamming_truth(q, c, 1500), "k = 1500")


def device_call(q, c, k, fill=0, ld_extra=0):
    import torch

    dev = torch.device("cuda:0")
    (m, w), n = q.shape, c.shape[0]
    ld = -(-w // 16) * 16 + ld_extra
    tq = torch.zeros((m, ld), dtype=torch.uint8, device=dev)
    tc = torch.zeros((n, ld), dtype=torch.uint8, device=dev)
    tq[:, :w], tc[:, :w] = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)
    wb = _native.bits_workspace_bytes(m, n, w, k)
    assert wb > 0
    ws = torch.full((wb + 256,), fill, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    oi = torch.full((m, k), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    osc = torch.full((m, k), 123.0, dtype=torch.float64, device=dev)
    _native.topk_bits_device(tq.data_ptr(), ld, m, tc.data_ptr(), ld, n, w, k, oi.data_ptr(), osc.data_ptr(),
                             workspace=ws.data_ptr() + off, workspace_bytes=wb,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy().view(np.uint32), osc.cpu().numpy()


@pytest.mark.parametrize("shape", [(70, 3000, 96, 100), (33, 1037, 9, 10), (33, 3000, 12, 1500)],
                         ids=["native", "odd width", "widened"])
def test_host_handle_and_device_entries_agree(env, shape):
    m, n, w, k = shape
    rs = np.random.RandomState(m + n + w)
    q, c = bit_rows(rs, m, w), bit_rows(rs, n, w)
    want = hamming_truth(q, c, k)
    assert_lists(_native.topk_bits_host(q, c, k), want, "host entry")
    dc = _native.DeviceCorpus.bits(c)
    try:
        assert dc.nbytes == _native.bits_device_bytes(n, w) == n * (-(-w // 16) * 16) + 4 * n
        assert_lists(dc.topk(q, k), want, "handle entry")
    finally:
        dc.close()
    assert_lists(device_call(q, c, k), want, "device entry, a workspace of exactly the stated bytes")
    assert_lists(device_call(q, c, k, ld_extra=32), want, "device entry, wider strides")


def test_other_entries_refuse_a_bit_handle(env):
    rs = np.random.RandomState(2)
    dc = _native.DeviceCorpus.bits(bit_rows(rs, 50, 4))
    try:
        with pytest.raises(_native.PmmError, match="pmm_topk_bits_corpus"):
            _native.check(_native.lib().pmm_topk_f32_corpus(dc._h, None, 1, 1, 0, None, None))
        with pytest.raises(_native.PmmError, match="no subsets"):
            dc.subset(np.array([0, 1], np.uint32))
        with pytest.raises(_native.PmmError, match="f32 handle"):
            dc.sign_bits()
    finally:
        dc.close()


# ---------------------------------------------------------------------------
# Packing
# ---------------------------------------------------------------------------
def device_pack(x, ld_extra=0, shift=0):
    """pmm_pack_sign_device of x held at row stride d + ld_extra, `shift` floats into an allocation."""
    import torch

    rows, d = x.shape
    ldx = d + ld_extra
    buf = torch.full((rows * ldx + shift + 8,), 7.0, dtype=torch.float32, device="cuda:0")  # (slack columns > 0)
    view = buf[shift:shift + rows * ldx].view(rows, ldx)
    view[:, :d] = torch.from_numpy(x).to("cuda:0")
    w = -(-d // 8)
    ld_out = -(-w // 8) * 8
    out = torch.full((rows, ld_out), 0xEE, dtype=torch.uint8, device="cuda:0")
    _native.pack_sign_device(view.data_ptr(), ldx, rows, d, out.data_ptr(), ld_out,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not got[:, w:].any(), "the bytes between w and roundup(w, 8) are not zero"
    return view.data_ptr(), got[:, :w]


@pytest.mark.parametrize("d", [1, 63, 64, 65, 768, 1000, 5000])
def test_device_packing_equals_pack_sign(env, d):
    rs = np.random.RandomState(d)
    x = np.ascontiguousarray(np.concatenate([special_rows(d), rs.randn(70, d).astype(np.float32)]))
    want = polars_matmul.pack_sign(x)
    assert np.array_equal(device_pack(x)[1], want), "tight rows"
    assert np.array_equal(device_pack(x, ld_extra=5)[1], want), "a source stride above d"
    ptr, got = device_pack(x, ld_extra=3, shift=1)
    assert ptr % 16 != 0 and ptr % 4 == 0
    assert np.array_equal(got, want), "a source that is 4-byte but not 16-byte aligned"


def test_sign_bits_handle_equals_the_uploaded_one(env):
    rs = np.random.RandomState(77)
    n, d, k = 3001, 100, 50
    c = np.ascontiguousarray(np.concatenate([special_rows(d), rs.randn(n - 13, d).astype(np.float32)]))
    q = polars_matmul.pack_sign(rs.randn(70, d).astype(np.float32))
    packed = polars_matmul.pack_sign(c)
    want = hamming_truth(q, packed, k)
    f32 = _native.DeviceCorpus(c)
    up = _native.DeviceCorpus.bits(packed)
    try:
        sb = f32.sign_bits()
        try:
            assert sb.n == n and sb.d == 13 and sb.nbytes == up.nbytes == _native.bits_device_bytes(n, 13)
            assert_lists(sb.topk(q, k), want, "sign_bits handle")
            assert_lists(up.topk(q, k), want, "uploaded handle")
        finally:
            sb.close()
        sel = np.flatnonzero(rs.rand(n) < 0.3).astype(np.uint32)
        sub = f32.subset(sel)
        try:
            sbs = sub.sign_bits()
            try:
                assert sbs.n == sel.size and sbs.nbytes == _native.bits_device_bytes(sel.size, 13) + 4 * sel.size
                wi, wsc = hamming_truth(q, packed[sel], k)
                assert_lists(sbs.topk(q, k), (sel[wi], wsc), "sign_bits of a subset: the parent's row numbers")
            finally:
                sbs.close()
        finally:
            sub.close()
    finally:
        up.close()
        f32.close()


# ---------------------------------------------------------------------------
# End to end: sign bits, Hamming 4 k, exact re-rank of the candidates
# ---------------------------------------------------------------------------
def test_two_stage_search_plumbing(env):
    import pyarrow as pa

    rs = np.random.RandomState(4)
    m, n, d, k = 40, 3000, 96, 10
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    qb, cb = pm._sign_bits(q), pm._sign_bits(c)
    assert qb.type == pa.list_(pa.uint8(), 12)
    first = pm._topk_hamming(qb, cb, 4 * k)
    ids = np.asarray(first.values.field("index").to_numpy()).reshape(m, 4 * k)
    wi, wsc = hamming_truth(polars_matmul.pack_sign(q), polars_matmul.pack_sign(c), 4 * k)
    assert np.array_equal(ids, wi)
    assert np.array_equal(np.asarray(first.values.field("score").to_numpy()).reshape(m, 4 * k), wsc)
    offsets = np.arange(m + 1, dtype=np.int64) * (4 * k)
    got = polars_matmul.topk(q, c, k, "cosine", candidates=(offsets, ids.reshape(-1)))
    want = polars_matmul.topk(q, c, k, "cosine", candidates=(offsets, wi.reshape(-1)))
    assert got[0].shape == (m, k) and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))


# ---------------------------------------------------------------------------
# Poisoned scratch (tests/test_gpu_dirty_scratch.py's setting)
# ---------------------------------------------------------------------------
def test_native_and_overflow_routes_on_poisoned_scratch(env):
    rs = np.random.RandomState(11)
    q, c = bit_rows(rs, 70, 20), bit_rows(rs, 3001, 20)
    want = hamming_truth(q, c, 100)
    for fill in POISONS:  # a caller's workspace filled with the poison
        assert_lists(device_call(q, c, 100, fill=fill), want, f"native, workspace filled with {fill:#04x}")
    c2, patterns = tie_corpus(rs)
    q2 = np.ascontiguousarray(np.concatenate([patterns[:30], bit_rows(rs, 40, 12)]))
    c2 = np.ascontiguousarray(c2[hamming_truth(q2[:1], c2, 3000)[0][0][::-1]])
    want2 = hamming_truth(q2, c2, 10)
    env.setenv("PMM_BITS_CAP", "64")
    for fill in POISONS:
        assert_lists(device_call(q2, c2, 10, fill=fill), want2, f"overflow re-run, workspace filled with {fill:#04x}")
    try:
        for text in ("0xFF", "127", "0x01"):  # the host entry with the thread's arena filled
            env.setenv("PMM_ARENA_POISON", text)
            assert_lists(_native.topk_bits_host(q2, c2, 10), want2, f"overflow re-run, arena filled with {text}")
            env.delenv("PMM_BITS_CAP")
            assert_lists(_native.topk_bits_host(q, c, 100), want, f"native, arena filled with {text}")
            env.setenv("PMM_BITS_CAP", "64")
    finally:
        env.delenv("PMM_ARENA_POISON", raising=False)


# ---------------------------------------------------------------------------
# Guard bands and slack (tests/test_gpu_dirty_scratch.py section C's setting):
# outputs and workspace between pattern bands that are checked after the call,
# the packed operands inside taller, wider tensors whose every free byte is
# 0xFF -- rows before and after, and the stride slack past the zero padding.
# ---------------------------------------------------------------------------
GUARD, PATTERN = 4096, 0xA5


class Banded:
    """`nbytes` of device memory between two bands of at least GUARD pattern bytes, the inner
    pointer aligned to `align`."""

    def __init__(self, nbytes, align=256, fill=0x5A):
        import torch

        self.t = torch.full((nbytes + 2 * GUARD + align,), PATTERN, dtype=torch.uint8, device="cuda:0")
        self.lo = GUARD + (-(self.t.data_ptr() + GUARD)) % align
        self.hi = self.lo + nbytes
        self.ptr = self.t.data_ptr() + self.lo
        self.t[self.lo:self.hi] = fill

    def inner(self, dtype, shape):
        return self.t[self.lo:self.hi].cpu().numpy().view(dtype).reshape(shape)

    def check(self, label):
        import torch

        assert bool(torch.all(self.t[:self.lo] == PATTERN)), f"{label}: bytes before the buffer were written"
        assert bool(torch.all(self.t[self.hi:] == PATTERN)), f"{label}: bytes behind the buffer were written"


def framed_bit_rows(a):
    """a's packed rows inside a taller, wider tensor: 64 rows of 0xFF before and after, a row
    stride 48 bytes above roundup(w, 16), bytes w .. roundup(w, 16) - 1 zero (the padding the
    entry asks for), every byte past them 0xFF.  (tensor, pointer to row 0, stride)."""
    import torch

    rows, w = a.shape
    dp = -(-w // 16) * 16
    ld = dp + 48
    t = torch.full((rows + 128, ld), 0xFF, dtype=torch.uint8, device="cuda:0")
    t[64:64 + rows, :dp] = 0
    t[64:64 + rows, :w] = torch.from_numpy(a).to("cuda:0")
    return t, t[64].data_ptr(), ld


def guarded_call(q, c, k, fill):
    """pmm_topk_bits_device with banded outputs and a banded workspace of exactly the stated
    bytes filled with `fill`, framed operands; the bands are checked."""
    import torch

    (m, w), n = q.shape, c.shape[0]
    (hq, pq, ldq), (hc, pc, ldc) = framed_bit_rows(q), framed_bit_rows(c)
    wb = _native.bits_workspace_bytes(m, n, w, k)
    oi, osc, ws = Banded(m * k * 4), Banded(m * k * 8), Banded(wb, fill=fill)
    _native.topk_bits_device(pq, ldq, m, pc, ldc, n, w, k, oi.ptr, osc.ptr, workspace=ws.ptr, workspace_bytes=wb,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for name, b in (("indices", oi), ("scores", osc), ("workspace", ws)):
        b.check(f"{name}, workspace filled with {fill:#04x}")
    del hq, hc
    return oi.inner(np.uint32, (m, k)), osc.inner(np.float64, (m, k))


@pytest.mark.parametrize("route", ["native", "overflow", "widened"])
def test_routes_inside_guard_bands_and_dirty_slack(env, route):
    rs = np.random.RandomState(len(route))
    if route == "overflow":
        c, patterns = tie_corpus(rs, w=13)
        q = np.ascontiguousarray(np.concatenate([patterns[:30], bit_rows(rs, 40, 13)]))
        c = np.ascontiguousarray(c[hamming_truth(q[:1], c, 3000)[0][0][::-1]])  # (test_forced_overflow's order)
        k = 10
        env.setenv("PMM_BITS_CAP", "64")
    else:
        q, c = bit_rows(rs, 70, 21), bit_rows(rs, 3001, 21)  # (w no multiple of 8 or 16)
        k = 100 if route == "native" else 1100
    want = hamming_truth(q, c, k)
    _native.timing_enable(True)
    try:
        for fill in (0,) + POISONS:
            _native.timing_reset()
            assert_lists(guarded_call(q, c, k, fill), want, f"{route}, workspace filled with {fill:#04x}")
            if route == "overflow":
                assert _native.timing_read("bits_gather")[1] >= 1, "no row overflowed: the re-run did not happen"
    finally:
        _native.timing_enable(False)
        _native.timing_reset()


@pytest.mark.parametrize("d", [1, 63, 64, 65, 1000, 5000])
def test_device_packing_inside_guard_bands(env, d):
    """The packed rows between guard bands at the least stride the entry takes and at a wider
    one (whose slack must stay untouched); the f32 rows inside NaN rows with NaN behind column d."""
    import torch

    rs = np.random.RandomState(d + 1)
    x = np.ascontiguousarray(np.concatenate([special_rows(d), rs.randn(40, d).astype(np.float32)]))
    rows, w = x.shape[0], -(-d // 8)
    w8 = -(-w // 8) * 8
    want = polars_matmul.pack_sign(x)
    ldx = d + 7
    t = torch.full((rows + 8, ldx), float("nan"), dtype=torch.float32, device="cuda:0")
    t[4:4 + rows, :d] = torch.from_numpy(x).to("cuda:0")
    for ld_out in (w8, w8 + 24):
        out = Banded(rows * ld_out, fill=0x5A)
        _native.pack_sign_device(t[4].data_ptr(), ldx, rows, d, out.ptr, ld_out,
                                 stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.check(f"pack d={d} ld_out={ld_out}")
        got = out.inner(np.uint8, (rows, ld_out))
        assert np.array_equal(got[:, :w], want), f"d={d} ld_out={ld_out}"
        assert not got[:, w:w8].any() and np.all(got[:, w8:] == 0x5A), f"d={d} ld_out={ld_out}: bytes past the row"


# ---------------------------------------------------------------------------
# The corpus cache: key mode "bits" and the device-packed column
# ---------------------------------------------------------------------------
def test_cached_bit_handle_and_device_packed_column(env):
    import pyarrow as pa

    pm.clear_corpus_cache()
    rs = np.random.RandomState(21)
    n, d, m, k = 40000, 256, 20, 50  # (40000 x 32 bytes of bits and 40000 x 1 KiB of f32: both above the cache's 1 MiB)
    x = rs.randn(n, d).astype(np.float32)
    x[:13, :19] = special_rows(19)
    col = pa.FixedSizeListArray.from_arrays(pa.array(x.reshape(-1)), d)
    packed = polars_matmul.pack_sign(x)
    try:
        # not cached yet: the NumPy form
        host = pm._sign_bits(col)
        assert len(pm._cache) == 0
        pm._topk(x[:m], col, 5, "cosine")  # the column becomes a cached f32 handle ...
        assert len(pm._cache) == 1
        dev = pm._sign_bits(col)           # ... and is packed on the device from it
        assert dev.type == host.type == pa.list_(pa.uint8(), 32)
        for name, got in (("host", host), ("device", dev)):
            assert np.array_equal(np.asarray(got.values.to_numpy()).reshape(n, 32), packed), name
        _native.timing_enable(True)
        _native.timing_reset()
        pm._sign_bits(col)
        assert _native.timing_read("pack_sign")[1] == 1, "the cached column was not packed on the device"
        # the bit column as a cached bit handle: created once, searched twice
        q = polars_matmul.pack_sign(rs.randn(m, d).astype(np.float32))
        want = hamming_truth(q, packed, k)
        for call in (1, 2):
            _native.timing_reset()
            out = pm._topk_hamming(q, dev, k)
            assert len(pm._cache) == 2 and any(key[-1] == "bits" for key in pm._cache)
            # (the corpus' popcounts at the handle's creation, the queries' per call)
            assert _native.timing_read("bits_popcount")[1] == (2 if call == 1 else 1)
            got = (np.asarray(out.values.field("index").to_numpy()).reshape(m, k),
                   np.asarray(out.values.field("score").to_numpy()).reshape(m, k))
            assert_lists(got, want, f"cached bit handle, call {call}")
    finally:
        _native.timing_enable(False)
        _native.timing_reset()
        pm.clear_corpus_cache()
