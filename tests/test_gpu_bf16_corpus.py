"""GPU tests of the bf16 device-resident corpus: the one-pass round-and-norm
kernel (pmm_round_bf16_device) against independent references, the handle
(pmm_corpus_create_bf16 / pmm_topk_bf16_corpus) against the host entry it must
equal bit for bit, its launches, sharding, typing and lifetime, and
``_topk(..., compute="bf16")`` through the corpus cache."""
from __future__ import annotations

import ctypes
import itertools
import threading

import numpy as np
import pytest

from parity import check_topk, dot_scale, round_bf16
from polars_matmul import _native

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
METRIC_NAMES = {COS: "cosine", DOT: "dot", EUC: "euclidean"}
BF16 = _native.COMPUTE_BF16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_f32(got, want, label):
    """Bit equality, any NaN matching any NaN (a NaN's payload is not part of the contract)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{label}: NaN positions differ"
    bad = (bits(got) != bits(want)) & ~gn
    assert not bad.any(), f"{label}: rows {np.nonzero(bad)[0][:5]} got {got[bad][:5]} want {want[bad][:5]}"


def assert_same_lists(a, b, label):
    (ia, sa), (ib, sb) = a, b
    assert np.array_equal(ia, ib), f"{label}: indices differ in {int(np.sum(np.any(ia != ib, axis=1)))} rows"
    assert np.array_equal(bits(sa), bits(sb)), f"{label}: score bits differ"


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 3.4e38], dtype=np.float32)
# exactly halfway between two bf16 numbers: down to the even 0x3F80, up to the even 0x3F82
HALFWAY = np.array([0x3F808000, 0x3F818000], dtype=np.uint32).view(np.float32)


def kernel_input(rows, d, seed):
    rs = np.random.RandomState(seed)
    a = rs.randn(rows, d + 5).astype(np.float32)  # source stride d + 5: the last 5 columns are not part of the rows
    if rows > 1:
        a[rows // 2, :] = 0.0  # an all-zero row (the zero-norm rule)
    vals = np.concatenate([SPECIALS, HALFWAY])
    for i, v in enumerate(vals):  # spread over rows and columns, never on the zero row unless rows == 1
        r = (3 * i + 1) % rows
        if rows > 1 and r == rows // 2:
            r = (r + 1) % rows
        a[r, (5 * i) % d] = v
    return a


def run_round(a, d, ldo, want=(True, True, True, True)):
    """pmm_round_bf16_device on a (rows, d + 5) f32 matrix; returns the 0xFF-prefilled output and the four
    arrays (None where skipped), plus the references."""
    import torch

    dev = torch.device("cuda:0")
    rows, ld = a.shape
    ta = torch.from_numpy(a).to(dev)
    out = torch.full((rows, ldo), -1, dtype=torch.int16, device=dev)  # 0xFFFF: unwritten padding shows
    arrs = [torch.full((rows,), 12345.0, dtype=torch.float32, device=dev) for _ in range(4)]
    ptrs = [t.data_ptr() if w else 0 for t, w in zip(arrs, want)]
    st = torch.cuda.current_stream().cuda_stream
    _native.round_bf16_device(ta.data_ptr(), ld, rows, d, out.data_ptr(), ldo, norm=ptrs[0], inv_norm=ptrs[1],
                              sq=ptrs[2], sq_factor=ptrs[3], stream=st)
    # references: torch's RNE rounding; the parent's norms kernel on the rounded rows widened exactly
    ref_rows = torch.zeros((rows, ldo), dtype=torch.int16, device=dev)
    rounded = ta[:, :d].to(torch.bfloat16)
    ref_rows[:, :d] = rounded.view(torch.int16)
    wide = torch.zeros((rows, ldo), dtype=torch.float32, device=dev)
    wide[:, :d] = rounded.to(torch.float32)
    rn = torch.empty((rows,), dtype=torch.float32, device=dev)
    rsq = torch.empty((rows,), dtype=torch.float32, device=dev)
    _native.norms_device(wide.data_ptr(), ldo, rows, d, False, rn.data_ptr(), stream=st)
    _native.norms_device(wide.data_ptr(), ldo, rows, d, True, rsq.data_ptr(), stream=st)
    torch.cuda.synchronize()
    rn, rsq = rn.cpu().numpy(), rsq.cpu().numpy()
    with np.errstate(all="ignore"):
        rinv = np.where(rn > np.float32(1e-6), np.float32(1.0) / rn, np.float32(0.0)).astype(np.float32)
        rfac = (rsq * np.float32(1.0 - 2.0 ** -18)).astype(np.float32)
    got = [t.cpu().numpy() for t in arrs]
    return out.cpu().numpy(), got, ref_rows.cpu().numpy(), [rn, rinv, rsq, rfac]


def check_round(a, d, ldo, want=(True, True, True, True), label=""):
    out, got, ref_rows, refs = run_round(a, d, ldo, want)
    assert np.array_equal(out.view(np.uint16), ref_rows.view(np.uint16)), (
        f"{label}: bf16 rows differ at {np.argwhere(out != ref_rows)[:4].tolist()}")
    for name, g, r, w in zip(("norm", "inv_norm", "sq", "sq_factor"), got, refs, want):
        if w:
            assert_same_f32(g, r, f"{label} {name}")
        else:
            assert np.all(g == np.float32(12345.0)), f"{label}: skipped array {name} was written"


@pytest.mark.parametrize("d", [1, 7, 8, 9, 37, 128, 129, 700, 1024, 1500])
def test_round_kernel_matches_references(d):
    assert _native.device_count() > 0, "no HIP device visible"
    for rows in (1, 33, 257):
        check_round(kernel_input(rows, d, 1000 * d + rows), d, -(-d // 128) * 128, label=f"d={d} rows={rows}")


def test_round_kernel_output_stride_roundup_8():
    for d in (9, 129, 700):
        check_round(kernel_input(33, d, d), d, -(-d // 8) * 8, label=f"d={d} ldo=roundup(d, 8)")


def test_round_kernel_vector_loads_when_source_is_aligned():
    # (the other cases' stride d + 5 takes the scalar loads; 16-byte-aligned rows take the 16-byte ones)
    for d in (7, 123, 251, 763):
        a = kernel_input(33, d, 7 * d)
        assert (a.shape[1] % 4) == 0
        check_round(a, d, -(-d // 128) * 128, label=f"aligned d={d}")


def test_round_kernel_null_outputs():
    a = kernel_input(33, 37, 5)
    for want in itertools.product((True, False), repeat=4):
        check_round(a, 37, 128, want, label=f"outputs {want}")


def test_round_kernel_argument_errors():
    import torch

    t = torch.zeros(64 * 16, dtype=torch.float32, device="cuda:0")
    o = torch.zeros(64 * 128, dtype=torch.int16, device="cuda:0")
    for ld, d, ldo, off in ((16, 16, 12, 0), (16, 16, 8, 0), (8, 16, 16, 0), (16, 16, 16, 2)):
        with pytest.raises(_native.PmmError) as ei:
            _native.round_bf16_device(t.data_ptr(), ld, 4, d, o.data_ptr() + off, ldo)
        assert ei.value.code == _native.PMM_ERR_ARG


# ---------------------------------------------------------------------------
# 2. handle == host entry, bit for bit
# ---------------------------------------------------------------------------
SHAPES = [
    ("small", 70, 5000, 96, 10),
    ("wave-specialised", 130, 16384, 256, 100),
    ("one-wave k=500", 70, 5000, 96, 500),
    ("widened d=1024", 33, 3000, 1024, 100),
    ("widened k=1000", 33, 3000, 96, 1000),
    ("k = n, d = 1", 3, 5, 1, 5),
]
_data = {}


def data(m, n, d):
    if (m, n, d) not in _data:
        rs = np.random.RandomState(m + n + d)
        _data[(m, n, d)] = (rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32))
    return _data[(m, n, d)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_handle_equals_host_bf16(shape):
    label, m, n, d, k = shape
    assert _native.device_count() > 0, "no HIP device visible"
    q, c = data(m, n, d)
    dc = _native.DeviceCorpus(c, compute="bf16")
    try:
        assert dc.nbytes == n * (-(-d // 128) * 128) * 2 + 16 * n
        for metric in (COS, DOT, EUC):
            got = dc.topk(q, k, metric)
            assert got[1].dtype == np.float32
            assert_same_lists(got, _native.topk_host(q, c, k, metric, compute=BF16), f"{label} {METRIC_NAMES[metric]}")
            if label in ("small", "wave-specialised"):
                # and against the rounded rows' truth, so the test does not rest on the library alone
                from golden.make_golden import truth_scores

                qb, cb = round_bf16(q), round_bf16(c)
                scale = dot_scale(qb, cb) if metric == DOT else None
                check_topk(got[0], got[1], truth_scores(qb, cb, METRIC_NAMES[metric]), metric != EUC, rtol=1e-5,
                           atol=1e-5, scale=scale, label=label)
    finally:
        dc.close()


def test_handle_equals_host_zero_row_and_ties():
    rs = np.random.RandomState(11)
    q = rs.randn(40, 64).astype(np.float32)
    c = rs.randn(2000, 64).astype(np.float32)
    c[5] = 0.0
    c[7] = c[3]
    c[100] = c[3]
    c[1999] = c[1998]
    q[2] = 0.0
    q[4] = c[3]
    dc = _native.DeviceCorpus(c, compute="bf16")
    try:
        for metric in (COS, DOT, EUC):
            got = dc.topk(q, 20, metric)
            assert_same_lists(got, _native.topk_host(q, c, 20, metric, compute=BF16), METRIC_NAMES[metric])
        # ties break to the lower index: row 3 and its copies lead query 4's cosine list in index order
        idx, _ = dc.topk(q, 3, COS)
        assert idx[4].tolist() == [3, 7, 100]
    finally:
        dc.close()


# ---------------------------------------------------------------------------
# 3. no corpus work per call
# ---------------------------------------------------------------------------
def launches():
    """(round_norms_bf16 launches, norms_bf16 launches): pmm_timing_read matches substrings, and the
    second name is one of the first."""
    r = _native.timing_read("round_norms_bf16")[1]
    return r, _native.timing_read("norms_bf16")[1] - r


@pytest.mark.parametrize("metric", [COS, DOT])
def test_handle_call_launches_no_corpus_work(metric):
    q, c = data(70, 5000, 96)
    dc = _native.DeviceCorpus(c, compute="bf16")
    _native.timing_enable(True)
    try:
        _native.timing_reset()
        dc.topk(q, 10, metric)
        assert launches() == (1, 0)
        assert _native.timing_read("f32_to_bf16")[1] == 0
        # the host entry, for contrast, norms both operands every call (none for dot)
        _native.timing_reset()
        _native.topk_host(q, c, 10, metric, compute=BF16)
        assert launches() == (0, 0 if metric == DOT else 1)
        # creation: one pass per shard
        _native.timing_reset()
        _native.DeviceCorpus(c, compute="bf16").close()
        assert launches() == (1, 0)
    finally:
        _native.timing_reset()
        _native.timing_enable(False)
        dc.close()


# ---------------------------------------------------------------------------
# 4. sharded handles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("devs, m, n, d, k", [([0, 0, 0], 70, 5000, 96, 10), ([0] * 8, 70, 5000, 96, 10),
                                              ([0] * 8, 31, 101, 96, 64)],
                         ids=["3 shards", "8 shards", "8 shards shorter than k"])
def test_sharded_handle(devs, m, n, d, k):
    q, c = data(m, n, d)
    one = _native.DeviceCorpus(c, compute="bf16")
    dc = None
    try:
        _native.set_devices(devs)
        dc = _native.DeviceCorpus(c, compute="bf16")
        assert dc.shards == len(devs) and one.shards == 1
        for metric in (COS, DOT, EUC):
            got = dc.topk(q, k, metric)
            # the same per-shard routes as the host entry under the same list
            assert_same_lists(got, _native.topk_host(q, c, k, metric, compute=BF16), METRIC_NAMES[metric])
            # pmm.h's rule for sharded bf16 against one device
            ref = one.topk(q, k, metric)
            assert np.mean(got[0] == ref[0]) > 0.99
    finally:
        _native.set_devices([])
        one.close()
        if dc is not None:
            dc.close()


def test_sharded_handle_refuses_k_above_1024():
    q, c = data(8, 2000, 32)
    dc = None
    try:
        _native.set_devices([0, 0])
        dc = _native.DeviceCorpus(c, compute="bf16")
        with pytest.raises(_native.PmmError) as ei:
            dc.topk(q, 1025, COS)
        assert ei.value.code == _native.PMM_ERR_UNSUPPORTED
        assert "a device-sharded corpus supports k <= 1024" in str(ei.value)
    finally:
        _native.set_devices([])
        if dc is not None:
            dc.close()


# ---------------------------------------------------------------------------
# 5. typing and lifetime
# ---------------------------------------------------------------------------
def test_handle_type_checks():
    q, c = data(8, 2000, 32)
    lib = _native.lib()
    hb = _native.DeviceCorpus(c, compute="bf16")
    h32 = _native.DeviceCorpus(c)
    h64 = _native.DeviceCorpus(c.astype(np.float64))
    try:
        assert hb.device_dtype == _native.DTYPE_BF16 == 2
        assert h32.device_dtype == _native.DTYPE_F32 and h64.device_dtype == _native.DTYPE_F64
        n, d, dev = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(-1)
        _native.check(lib.pmm_corpus_info(hb._h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(dev)))
        assert (n.value, d.value, dev.value) == (2000, 32, 0)
        idx = np.empty((8, 4), dtype=np.uint32)
        sc = np.empty((8, 4), dtype=np.float64)
        q64 = q.astype(np.float64)
        wrong = [(lib.pmm_topk_f32_corpus, hb, q, "pmm_topk_bf16_corpus"),
                 (lib.pmm_topk_f64_corpus, hb, q64, "pmm_topk_bf16_corpus"),
                 (lib.pmm_topk_bf16_corpus, h32, q, "pmm_topk_f32_corpus"),
                 (lib.pmm_topk_bf16_corpus, h64, q, "pmm_topk_f64_corpus"),
                 (lib.pmm_topk_f32_corpus, h64, q, "pmm_topk_f64_corpus"),
                 (lib.pmm_topk_f64_corpus, h32, q64, "pmm_topk_f32_corpus")]
        for fn, h, qq, right in wrong:
            rc = fn(h._h, _native.ptr(qq), 8, 4, COS, _native.ptr(idx), _native.ptr(sc))
            assert rc == _native.PMM_ERR_ARG and _native.last_error().endswith(f"use {right}")
    finally:
        for h in (hb, h32, h64):
            h.close()


def test_create_argument_errors_are_the_f32_creators():
    lib = _native.lib()
    c = np.zeros((4, 4), dtype=np.float32)
    for n, d in ((0, 4), (4, 0), (-1, 4)):
        texts = []
        for create in (lib.pmm_corpus_create_f32, lib.pmm_corpus_create_bf16):
            h = ctypes.c_void_p()
            assert create(_native.ptr(c), n, d, ctypes.byref(h)) == _native.PMM_ERR_ARG
            texts.append(_native.last_error())
        assert texts[0] == texts[1]


def test_handle_lifetime_and_threads():
    q, c = data(70, 5000, 96)
    dc = _native.DeviceCorpus(c, compute="bf16")
    serial = dc.topk(q, 10, COS)
    # two threads searching one handle return the serial result
    res = [None, None]

    def search(i):
        res[i] = [dc.topk(q, 10, COS) for _ in range(4)]

    ts = [threading.Thread(target=search, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r in res:
        for got in r:
            assert_same_lists(got, serial, "threaded")
    # close while another thread searches: the search in flight finishes, later ones are refused
    started = threading.Event()
    done, errors = [], []

    def searcher():
        for _ in range(50):
            try:
                done.append(dc.topk(q, 10, COS))
            except RuntimeError as e:
                errors.append(str(e))
                break
            finally:
                started.set()

    t = threading.Thread(target=searcher)
    t.start()
    started.wait()
    dc.close()
    t.join()
    assert dc.closed
    assert done and all(e == "DeviceCorpus is closed" for e in errors)
    for got in done:
        assert_same_lists(got, serial, "closed while searching")
    with pytest.raises(RuntimeError):
        dc.topk(q, 10, COS)
    dc.close()  # idempotent


# ---------------------------------------------------------------------------
# 6. through _topk and the corpus cache
# ---------------------------------------------------------------------------
def lists_of(out, m, k):
    vals = out.values
    return (vals.field("index").to_numpy().reshape(m, k), vals.field("score").to_numpy().reshape(m, k))


def test_topk_compute_bf16_through_the_cache():
    import pyarrow as pa

    import polars_matmul
    from polars_matmul import _polars_matmul as pm

    m, n, d, k = 50, 4096, 96, 10  # corpus 1.5 MB: the cache engages
    q, c = data(m, n, d)
    arr = pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1), type=pa.float32()), d)
    arr64 = pa.FixedSizeListArray.from_arrays(pa.array(c.astype(np.float64).reshape(-1), type=pa.float64()), d)
    pm.clear_corpus_cache()
    _native.timing_enable(True)
    try:
        f32_before = lists_of(pm._topk(q, arr, k, "cosine"), m, k)
        pm.clear_corpus_cache()
        for metric in ("cosine", "dot", "euclidean"):
            want = polars_matmul.topk(q, c, k, metric, compute="bf16")
            _native.timing_reset()
            got = lists_of(pm._topk(q, arr, k, metric, compute="bf16"), m, k)
            assert got[1].dtype == np.float64
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), metric
            assert len(pm._cache) == 1
            # first call: the handle's pass and the queries'; afterwards the queries' alone
            assert launches() == (2 if metric == "cosine" else 1, 0)
        # an f32 search of the same array: its own entry, the result it gave before
        f32_after = lists_of(pm._topk(q, arr, k, "cosine"), m, k)
        assert len(pm._cache) == 2
        assert np.array_equal(f32_after[0], f32_before[0]) and np.array_equal(f32_after[1], f32_before[1])
        # Float64 columns: read as f32
        want = polars_matmul.topk(q, c, k, "cosine", compute="bf16")
        got = lists_of(pm._topk(q.astype(np.float64), arr64, k, "cosine", compute="bf16"), m, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert len(pm._cache) == 3
        assert sorted(v[1].compute for v in pm._cache.values()) == ["bf16", "bf16", "f32"]
    finally:
        _native.timing_reset()
        _native.timing_enable(False)
        pm.clear_corpus_cache()
