"""Every route on hostile scratch and inside guard bands ("Workspace regions").

The value tests pin what a call returns; this module pins what it may start
from and what it may touch.

A. The device API in a caller's workspace filled with a poison byte.
B. The host entries and the handles with PMM_ARENA_POISON, which fills the
   thread's whole arena slot with that byte before the call uses it.
C. The device API with its outputs and workspace between guard bands and its
   operands inside taller, wider tensors whose every free element is NaN.

The assertion is always the same: indices and score bits equal those of the
same call on clean scratch (a zeroed workspace, the knob unset, tightly
allocated operands), compared as raw bits with no tolerance; once per case
family the clean result is also compared with the oracle, so that the two
cannot agree on a wrong answer.  bf16 results are compared clean against
poisoned only (their lists are deterministic: selection is a total order).

Poison bytes: 0xFF (u32 4294967295, f32 NaN: a threshold at its maximum, an
index that looks like the empty slot), 0x7F (u32 2.1e9, f32 3.4e38: a huge
composite key), 0x01 (u32 1.7e7, f32 a tiny denormal: a plausible count).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
from polars_matmul import _native

pytestmark = pytest.mark.gpu

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
METRICS = (COS, DOT, EUC)
F32, BF16 = _native.COMPUTE_F32, _native.COMPUTE_BF16
POISONS = (0xFF, 0x7F, 0x01)
# the knob takes decimal and 0x.. values: both spellings are used
POISON_TEXT = {0xFF: "0xFF", 0x7F: "127", 0x01: "0x01"}
GUARD = 4096      # bytes of pattern on each side of an output or a workspace
PATTERN = 0xA5
EMPTY_IDX, EMPTY_SCORE = 0xFFFFFFFF, 0x7FC00000


@pytest.fixture
def env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    assert _native.device_count() > 0, "no HIP device visible"
    return monkeypatch


@pytest.fixture
def device_list():
    yield
    _native.set_devices([])


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def assert_same(got, want, label):
    """Tuples of arrays: same shapes, same dtypes, the same bytes."""
    assert len(got) == len(want), label
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{label}: output {j} is {g.dtype}{g.shape}, not {w.dtype}{w.shape}"
        if not np.array_equal(raw(g), raw(w)):
            bad = np.flatnonzero(g.reshape(-1).view(f"u{g.dtype.itemsize}") != w.reshape(-1).view(f"u{w.dtype.itemsize}"))
            raise AssertionError(f"{label}: output {j} differs in {bad.size} of {g.size} entries, first at {bad[0]}: "
                                 f"{g.reshape(-1)[bad[0]]!r} != {w.reshape(-1)[bad[0]]!r}")


def assert_oracle(got, q, c, k, metric, label):
    """(idx, scores) against oracle.topk: the same indices and the same score bits."""
    oi, osc = oracle.topk(q, c, k, metric)
    idx, sc = got
    assert_same((np.asarray(idx).view(np.uint32), np.asarray(sc)),
                (np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(np.asarray(sc).dtype)), f"{label} vs oracle")


def randn(rs, rows, d, dtype=np.float32):
    return np.ascontiguousarray(rs.randn(rows, d).astype(dtype))


def roundup(x, a):
    return -(-x // a) * a


# ---------------------------------------------------------------------------
# A. A caller's workspace, device API
# ---------------------------------------------------------------------------
def device_lists(q, c, k, metric, compute, fills, ld=None):
    """One device-API call per entry of `fills` in a caller's workspace of exactly
    workspace_bytes(...) filled with that byte: [(idx u32, score bits u32), ...]."""
    import torch

    dev = torch.device("cuda:0")
    (m, d), n = q.shape, c.shape[0]
    dt = torch.bfloat16 if compute == BF16 else torch.float32
    ld = ld or roundup(d, 128 if compute == BF16 else 32)
    tq = torch.zeros((m, ld), dtype=dt, device=dev)
    tc = torch.zeros((n, ld), dtype=dt, device=dev)
    tq[:, :d] = torch.from_numpy(q).to(dev).to(dt)
    tc[:, :d] = torch.from_numpy(c).to(dev).to(dt)
    wb = _native.workspace_bytes(m, n, d, k, metric, compute)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    fn = _native.topk_bf16_device if compute == BF16 else _native.topk_device
    out = []
    for fill in fills:
        ws.fill_(fill)
        # (outputs that a call left unwritten would not pass for lists)
        oi = torch.full((m, k), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        osc = torch.full((m, k), 123.0, dtype=torch.float32, device=dev)
        fn(tq.data_ptr(), ld, m, tc.data_ptr(), ld, n, d, k, metric, oi.data_ptr(), osc.data_ptr(),
           workspace=ws.data_ptr(), workspace_bytes=wb, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.append((oi.cpu().numpy().view(np.uint32), osc.cpu().numpy().view(np.uint32)))
    return out


def poisoned_workspace(q, c, k, metric, compute, label, ld=None, exact=True):
    """Clean against the three poisons; the clean f32 lists against the oracle.  Returns the clean lists."""
    runs = device_lists(q, c, k, metric, compute, (0,) + POISONS, ld)
    for fill, got in zip(POISONS, runs[1:]):
        assert_same(got, runs[0], f"{label}, workspace filled with {fill:#04x}")
    if compute == F32 and exact:
        idx, bits_ = runs[0]
        assert_oracle((idx, bits_.view(np.float32)), q, c, k, metric, label)
    return runs[0]


# (label, m, n, d, k, metric, compute, environment)
# The first twelve are tests/test_workspace_routes.py's RUNS; the rest are the knobs and
# shapes that change which initialisation runs.
SCREEN_ON, SCREEN_OFF = {"PMM_F32_SCREEN": "1"}, {"PMM_F32_SCREEN": "0"}
BUDGET_KNOB = "PMM_MATERIALISE_BUDGET"
WORKSPACE_CASES = [
    ("f32 fused cosine", 130, 5000, 96, 10, COS, F32, {}),
    ("f32 fused dot", 130, 5000, 256, 10, DOT, F32, {}),
    ("f32 fused euclidean k=1024", 64, 4099, 256, 1024, EUC, F32, {}),
    ("f32 materialised k=1025", 64, 4099, 256, 1025, DOT, F32, {}),
    ("f32 global sort k=3000", 33, 8192, 96, 3000, COS, F32, {}),
    ("f32 screened", 70, 3037, 256, 10, COS, F32, SCREEN_ON),
    ("f32 screen off", 70, 3037, 256, 10, COS, F32, SCREEN_OFF),
    ("bf16 wave-specialised k=100", 130, 16384, 256, 100, COS, BF16, {}),
    ("bf16 one-wave k=500", 70, 5000, 96, 500, EUC, BF16, {}),
    ("bf16 widened d=1024", 70, 3000, 1024, 100, COS, BF16, {}),
    ("bf16 widened k=1000", 70, 3000, 256, 1000, DOT, BF16, {}),
    ("bf16 widened k=1500", 33, 3000, 96, 1500, COS, BF16, {}),
    # whole query blocks (qb_full != 0) and split units only (qb_full == 0), with one
    # workgroup running every unit, and two workgroups over three blocks (two whole, one split)
    ("f32 one workgroup, whole blocks", 130, 5000, 96, 10, COS, F32, {"PMM_CUS": "1"}),
    ("f32 one workgroup, split units", 130, 5000, 96, 10, COS, F32, {"PMM_CUS": "1", "PMM_F32_WHOLE": "0"}),
    ("f32 two workgroups, three blocks", 300, 5000, 96, 10, EUC, F32, {"PMM_CUS": "2", "PMM_F32_WHOLE": "1"}),
    ("f32 split units only", 300, 5000, 96, 10, DOT, F32, {"PMM_F32_WHOLE": "0"}),
    ("bf16 one workgroup, whole blocks", 130, 16384, 256, 100, COS, BF16, {"PMM_CUS": "1"}),
    ("bf16 one workgroup, split units", 130, 16384, 256, 100, COS, BF16, {"PMM_CUS": "1", "PMM_BF16_WHOLE": "0"}),
    ("bf16 two workgroups, three blocks", 300, 16384, 256, 100, EUC, BF16, {"PMM_CUS": "2", "PMM_BF16_WHOLE": "1"}),
    ("bf16 split units only", 300, 16384, 256, 100, DOT, BF16, {"PMM_BF16_WHOLE": "0"}),
    ("screened one workgroup, whole blocks", 130, 3037, 256, 10, COS, F32, {"PMM_CUS": "1", **SCREEN_ON}),
    ("screened split units only", 130, 3037, 256, 10, COS, F32, {"PMM_BF16_WHOLE": "0", **SCREEN_ON}),
    # the three fill routes of the fused f32 path: a memset (or the norms kernel's fill), the
    # one-launch prologue, the store-mode seed
    ("f32 cosine unseeded", 130, 5000, 96, 10, COS, F32, {"PMM_SEED": "0"}),
    ("f32 cosine seeded", 130, 5000, 96, 10, COS, F32, {"PMM_SEED": "1"}),
    ("f32 cosine seeded by the GEMM", 130, 5000, 96, 10, COS, F32, {"PMM_SEED": "1", "PMM_SEED_GEMM": "1"}),
    ("f32 dot unseeded", 130, 5000, 256, 10, DOT, F32, {"PMM_SEED": "0"}),
    ("f32 dot seeded", 130, 5000, 256, 10, DOT, F32, {"PMM_SEED": "1"}),
    ("f32 dot seeded by the GEMM", 130, 5000, 256, 10, DOT, F32, {"PMM_SEED": "1", "PMM_SEED_GEMM": "1"}),
    ("f32 euclidean seeded by the GEMM", 130, 5000, 96, 10, EUC, F32, {"PMM_SEED": "1", "PMM_SEED_GEMM": "1"}),
    ("bf16 unseeded", 130, 16384, 256, 100, COS, BF16, {"PMM_BF16_SEED": "0"}),
    ("screened, long corpus (seeded)", 70, 16384, 256, 10, COS, F32, SCREEN_ON),
    ("screened, long corpus, unseeded", 70, 16384, 256, 10, COS, F32, {"PMM_BF16_SEED": "0", **SCREEN_ON}),
    # m no multiple of the query block, n no multiple of the tile, d no multiple of the K step
    ("f32 130x5003x37", 130, 5003, 37, 10, COS, F32, {}),
    ("f32 33x1037x37 euclidean", 33, 1037, 37, 100, EUC, F32, {}),
    ("f32 33x1037x37 k=1025", 33, 1037, 37, 1025, COS, F32, {}),
    ("screened 33x1037x37", 33, 1037, 37, 10, COS, F32, SCREEN_ON),
    ("bf16 130x5003x37", 130, 5003, 37, 10, COS, BF16, {}),
    ("bf16 33x1037x37 k=500", 33, 1037, 37, 500, DOT, BF16, {}),
    # the materialised paths' row-chunk loops past the first chunk (PMM_MATERIALISE_BUDGET = R rows of
    # tests/row_chunk_cases.py's per_row): the score block, the sort keys and the tile counter are reused
    ("f32 materialised k=1025, chunks of 24 rows", 64, 4099, 256, 1025, DOT, F32, {BUDGET_KNOB: str(24 * 4099 * 4)}),
    ("f32 global sort k=3000, chunks of 13 rows", 33, 8192, 96, 3000, COS, F32,
     {BUDGET_KNOB: str(13 * (8192 * 4 + 8192 * 16))}),
    ("f64 materialised, chunks of 12 rows", 33, 1037, 37, 10, EUC, "f64",
     {"PMM_F64_FUSED": "0", BUDGET_KNOB: str(12 * 1037 * 8)}),
]


@pytest.mark.parametrize("case", WORKSPACE_CASES, ids=lambda c: c[0])
def test_route_in_a_poisoned_workspace(env, case):
    label, m, n, d, k, metric, compute, knobs = case
    for name, value in knobs.items():
        env.setenv(name, value)
    if knobs.get("PMM_F32_SCREEN") == "1":
        # (the screened route's workspace holds the images and the re-run's bytes)
        here = _native.workspace_bytes(m, n, d, k, metric, compute)
        env.setenv("PMM_F32_SCREEN", "0")
        assert here > _native.workspace_bytes(m, n, d, k, metric, compute), f"{label}: the call does not screen"
        env.setenv("PMM_F32_SCREEN", "1")
    rs = np.random.RandomState(m + n + d + k)
    if BUDGET_KNOB not in knobs:
        poisoned_workspace(randn(rs, m, d), randn(rs, n, d), k, metric, compute, label)
        return
    # a row-chunk case: the clean run and the three poisoned ones each launch the score GEMM once per chunk
    _native.timing_reset()
    _native.timing_enable(True)
    try:
        if compute == "f64":
            # (the f64 entries take no workspace argument: the host entry on a poisoned arena)
            q, c = randn(rs, m, d, np.float64), randn(rs, n, d, np.float64)
            want = under_poison(env, lambda: _native.topk_host(q, c, k, metric), label)
            assert_oracle(want, q, c, k, metric, label)
        else:
            poisoned_workspace(randn(rs, m, d), randn(rs, n, d), k, metric, compute, label)
        launches = _native.timing_read("gemm_f64_scores" if compute == "f64" else "gemm_f32_scores")[1]
    finally:
        _native.timing_enable(False)
        _native.timing_reset()
    assert launches == 3 * (1 + len(POISONS)), f"{label}: {launches} score launches in four calls of three chunks"


def test_screened_rerun_rows_in_poisoned_reserved_bytes(env, capfd):
    """tests/test_workspace_routes.py's crowded band: the rows that overflow are gathered, re-run on the
    f32 kernel and scattered back inside the workspace's reserved bytes, which hold the poison."""
    env.setenv("PMM_CUS", "1")
    env.setenv("PMM_F32_SCREEN", "1")
    env.setenv("PMM_SCREEN_DEBUG", "1")
    rs = np.random.RandomState(3)
    d, k = 128, 10
    v = rs.randn(d).astype(np.float32)
    near = v[None, :] * (1.0 + rs.randn(2000, d).astype(np.float32) * 10.0 ** rs.uniform(-6, -4, (2000, 1)).astype(np.float32))
    c = np.concatenate([rs.randn(1500, d).astype(np.float32), near.astype(np.float32)])
    c = np.ascontiguousarray(c[rs.permutation(len(c))])
    q = np.ascontiguousarray(np.concatenate([v[None, :] * np.float32(0.5), rs.randn(34, d).astype(np.float32)]))
    capfd.readouterr()
    poisoned_workspace(q, c, k, COS, F32, "crowded band", ld=d + 32)
    reports = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pmm screen]")]
    assert len(reports) == 1 + len(POISONS), reports
    for ln in reports:
        rep = {kv.split("=")[0]: kv.split("=")[1] for kv in ln.split()[2:] if "=" in kv}
        assert int(rep["overflowed"]) >= 1 and int(rep["rerun_rows"]) >= int(rep["overflowed"]), ln
        assert int(rep["whole_call_f32"]) == 0, ln


@pytest.mark.parametrize("compute", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("metric", METRICS)
def test_k_above_n_leaves_empty_slots_under_every_poison(env, metric, compute):
    m, n, d, k = 5, 7, 37, 10
    rs = np.random.RandomState(70 + metric)
    q, c = randn(rs, m, d), randn(rs, n, d)
    idx, bits_ = poisoned_workspace(q, c, k, metric, compute, f"k > n metric={metric}", exact=False)
    assert np.all(idx[:, n:] == EMPTY_IDX) and np.all(bits_[:, n:] == EMPTY_SCORE)
    assert np.all(np.sort(idx[:, :n], axis=1) == np.arange(n, dtype=np.uint32)[None, :])
    if compute == F32:
        assert_oracle((idx[:, :n], bits_[:, :n].view(np.float32)), q, c, n, metric, "k > n, the filled slots")


# ---------------------------------------------------------------------------
# B. Host entries and handles under PMM_ARENA_POISON
# ---------------------------------------------------------------------------
def under_poison(env, call, label):
    """call() with the knob unset, then under each poison: the same bytes.  Returns the clean result."""
    env.delenv("PMM_ARENA_POISON", raising=False)
    want = call()
    try:
        for b in POISONS:
            env.setenv("PMM_ARENA_POISON", POISON_TEXT[b])
            assert_same(call(), want, f"{label}, arena filled with {b:#04x}")
    finally:
        env.delenv("PMM_ARENA_POISON", raising=False)
    return want


@pytest.mark.parametrize("metric", METRICS)
def test_host_f32_entry(env, metric):
    rs = np.random.RandomState(10 + metric)
    q, c = randn(rs, 130, 37), randn(rs, 5003, 37)
    for k in (10, 1025):
        want = under_poison(env, lambda: _native.topk_host(q, c, k, metric), f"pmm_topk_f32_ex f32 k={k}")
        assert_oracle(want, q, c, k, metric, f"pmm_topk_f32_ex f32 k={k}")
    env.setenv("PMM_F32_SCREEN", "1")
    if metric == COS:
        want = under_poison(env, lambda: _native.topk_host(q, c, 10, metric), "pmm_topk_f32_ex screened")
        assert_oracle(want, q, c, 10, metric, "pmm_topk_f32_ex screened")


@pytest.mark.parametrize("shape", [(130, 5003, 37, 10), (70, 16384, 256, 100), (33, 3000, 1024, 100)],
                         ids=["one-wave", "wave-specialised", "widened"])
def test_host_bf16_compute(env, shape):
    m, n, d, k = shape
    rs = np.random.RandomState(m + n)
    q, c = randn(rs, m, d), randn(rs, n, d)
    for metric in METRICS:
        under_poison(env, lambda: _native.topk_host(q, c, k, metric, BF16), f"pmm_topk_f32_ex bf16 metric={metric}")


@pytest.mark.parametrize("fused", ["1", "0"])
def test_host_f64_entry(env, fused):
    env.setenv("PMM_F64_FUSED", fused)
    rs = np.random.RandomState(64)
    q, c = randn(rs, 33, 37, np.float64), randn(rs, 1037, 37, np.float64)
    for metric in METRICS:
        want = under_poison(env, lambda: _native.topk_host(q, c, 10, metric), f"pmm_topk_f64 fused={fused} metric={metric}")
        assert_oracle(want, q, c, 10, metric, f"pmm_topk_f64 fused={fused}")
    want = under_poison(env, lambda: _native.topk_host(q, c, 1037, COS), f"pmm_topk_f64 fused={fused} k=n")
    assert_oracle(want, q, c, 1037, COS, f"pmm_topk_f64 fused={fused} k=n")


def test_host_f64_overflow_falls_back(env):
    """tests/test_gpu_parity.py::test_f64_fused_overflow_falls_back's construction: every corpus row beats
    every earlier one, the buffers overflow and the call is redone materialised in the same workspace."""
    env.setenv("PMM_F64_FUSED", "1")
    n, d = 20000, 16
    q = np.ones((4, d))
    c = np.repeat(np.arange(n, dtype=np.float64)[:, None], d, axis=1) / n
    want = under_poison(env, lambda: _native.topk_host(q, c, 10, DOT), "pmm_topk_f64 overflow fallback")
    assert want[0].tolist() == [list(range(n - 1, n - 11, -1))] * 4
    assert_oracle(want, q, c, 10, DOT, "pmm_topk_f64 overflow fallback")


@pytest.mark.parametrize("fused", ["1", "0"])
def test_f64_device_entry_in_the_arena(env, fused):
    import torch

    env.setenv("PMM_F64_FUSED", fused)
    m, n, d, k = 33, 1037, 37, 10
    ld = roundup(d, 16)
    rs = np.random.RandomState(6)
    q, c = randn(rs, m, d, np.float64), randn(rs, n, d, np.float64)
    dev = torch.device("cuda:0")
    tq, tc = torch.zeros((m, ld), dtype=torch.float64, device=dev), torch.zeros((n, ld), dtype=torch.float64, device=dev)
    tq[:, :d], tc[:, :d] = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)

    def call(metric):
        oi = torch.full((m, k), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        osc = torch.full((m, k), 123.0, dtype=torch.float64, device=dev)
        _native.topk_f64_device(tq.data_ptr(), ld, m, tc.data_ptr(), ld, n, d, k, metric, oi.data_ptr(), osc.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return oi.cpu().numpy().view(np.uint32), osc.cpu().numpy()

    for metric in METRICS:
        want = under_poison(env, lambda: call(metric), f"pmm_topk_f64_device fused={fused} metric={metric}")
        assert_oracle(want, q, c, k, metric, f"pmm_topk_f64_device fused={fused}")


def i8_rows(rs, rows, d):
    return np.ascontiguousarray(rs.randint(-128, 128, size=(rows, d)).astype(np.int8))


def test_host_i8_entry_and_band_overflow_rerun(env):
    rs = np.random.RandomState(8)
    q, c = i8_rows(rs, 33, 70), i8_rows(rs, 3001, 70)
    for metric in METRICS:
        want = under_poison(env, lambda: _native.topk_i8_host(q, c, 10, metric), f"pmm_topk_i8 metric={metric}")
        assert_oracle(want, q.astype(np.float64), c.astype(np.float64), 10, metric, "pmm_topk_i8")
    # tests/test_gpu_int8.py::test_identical_rows_overflow_the_band_and_rerun: 600 equal rows tie at
    # every place of a k = 10 list; with 64-entry buffers the rows overflow and are re-run widened
    c[100:700] = q[3]
    env.setenv("PMM_I8_CAP", "64")
    _native.timing_enable(True)
    try:
        for metric in METRICS:
            _native.timing_reset()
            want = under_poison(env, lambda: _native.topk_i8_host(q, c, 10, metric), f"pmm_topk_i8 re-run metric={metric}")
            assert _native.timing_read("widen_i8_f64")[1] >= 1 + len(POISONS), "no row was re-run"
            assert_oracle(want, q.astype(np.float64), c.astype(np.float64), 10, metric, "pmm_topk_i8 re-run")
    finally:
        _native.timing_enable(False)
        _native.timing_reset()


@pytest.mark.parametrize("kind", ["f32", "f64 fused", "f64 materialised", "bf16", "i8"])
def test_corpus_handles(env, kind):
    rs = np.random.RandomState(len(kind))
    m, n, d, k = 33, 5003, 37, 10
    if kind == "i8":
        q, c = i8_rows(rs, m, d), i8_rows(rs, n, d)
        dc = _native.DeviceCorpus.int8(c)
    else:
        dt = np.float64 if kind.startswith("f64") else np.float32
        q, c = randn(rs, m, d, dt), randn(rs, n, d, dt)
        if kind.startswith("f64"):
            env.setenv("PMM_F64_FUSED", "1" if kind == "f64 fused" else "0")
        dc = _native.DeviceCorpus(c, compute="bf16") if kind == "bf16" else _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            want = under_poison(env, lambda: dc.topk(q, k, metric), f"{kind} handle metric={metric}")
            if kind != "bf16":
                wide = np.float64 if kind == "i8" else q.dtype
                assert_oracle(want, q.astype(wide), c.astype(wide), k, metric, f"{kind} handle")
    finally:
        dc.close()


def test_f32_handle_builds_its_image_and_screens(env):
    """A fresh handle per arena state: its first screened call builds the image, its second reads it."""
    env.setenv("PMM_F32_SCREEN", "1")
    rs = np.random.RandomState(77)
    q, c = randn(rs, 70, 256), randn(rs, 3037, 256)

    def call():
        dc = _native.DeviceCorpus(c)
        try:
            before = dc.nbytes
            first = dc.topk(q, 10, COS)
            assert dc.nbytes > before, "the handle built no screen image: the call did not screen"
            return first + dc.topk(q, 10, COS)
        finally:
            dc.close()

    want = under_poison(env, call, "f32 handle, image build and screened call")
    assert_same(want[2:], want[:2], "second screened call")
    assert_oracle(want[:2], q, c, 10, COS, "f32 handle screened")


@pytest.mark.parametrize("kind", ["mask offset 0", "mask offset 3", "ids"])
@pytest.mark.parametrize("image", [False, True], ids=["plain parent", "parent with image"])
def test_subset_derivation_and_search(env, kind, image):
    rs = np.random.RandomState(31)
    m, n, d, k = 33, 3037, 256 if image else 37, 10
    q, c = randn(rs, m, d), randn(rs, n, d)
    mask = rs.rand(n) < 0.4
    mask[[0, n - 1]] = True
    ids = np.flatnonzero(mask).astype(np.uint32)
    shift = 3 if kind == "mask offset 3" else 0
    bitmap = np.packbits(np.concatenate([np.ones(shift, bool), mask]), bitorder="little")
    if image:
        env.setenv("PMM_F32_SCREEN", "1")
    dc = _native.DeviceCorpus(c)
    try:
        if image:
            before = dc.nbytes
            dc.topk(q, k, COS)
            assert dc.nbytes > before, "the parent built no screen image"

        def call():
            sub = dc.subset(ids) if kind == "ids" else dc.subset_bitmap(bitmap.ctypes.data, shift)
            try:
                out = (sub.index_map(),)
                for metric in METRICS:
                    out += sub.topk(q, k, metric)
                return out
            finally:
                sub.close()

        want = under_poison(env, call, f"subset by {kind}")
        assert np.array_equal(want[0], ids)
        sel = np.ascontiguousarray(c[ids])
        for j, metric in enumerate(METRICS):
            oi, osc = oracle.topk(q, sel, k, metric)
            assert_same((want[1 + 2 * j], want[2 + 2 * j]), (ids[np.asarray(oi).astype(np.int64)], np.asarray(osc).astype(np.float32)),
                        f"subset by {kind} metric={metric} vs oracle")
    finally:
        dc.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("path", ["kernel", "loop"])
def test_partition_and_grouped_search(env, dtype, path):
    from test_gpu_grouped import assert_exact, main_shape, truth

    d, k = 37, 10
    q, c, ql, cl = main_shape(dtype, d, 5)
    env.setenv("PMM_GROUPED", path)
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            def call():
                part = dc.partition(cl, 8)
                try:
                    return (part.index_map(),) + part.topk_grouped(q, ql, k, metric)
                finally:
                    part.close()

            want = under_poison(env, call, f"grouped {path} metric={metric}")
            assert np.array_equal(want[0], _native.partition_plan(cl, 8)[0])
            assert_exact(want[1:], truth(q, c, ql, cl, k, metric), k, f"grouped {path} metric={metric}", dtype)
    finally:
        dc.close()


@pytest.mark.parametrize("route", ["sort", "any-k"])
def test_range_search(env, route):
    from test_gpu_range import cut, ranked

    m, n, d = 33, 2000, 37
    rs = np.random.RandomState(12)
    q, c = randn(rs, m, d), randn(rs, n, d)
    if route == "any-k":
        env.setenv("PMM_RANGE_SORT_MAX", "1024")
    dc = _native.DeviceCorpus(c)
    try:
        for metric in METRICS:
            full = ranked(q, c, metric)
            finite = full[1][np.isfinite(full[1])]
            # every row of the corpus (segments of 2000 keys: past PMM_RANGE_SORT_MAX), about a
            # tenth of them (wave and workgroup tiers), and no hit at all
            everything = float("inf") if metric == EUC else -float("inf")
            nothing = -1.0 if metric == EUC else float("inf")
            tenth = float(np.quantile(finite, 0.1 if metric == EUC else 0.9))
            for name, t in (("every row", everything), ("a tenth", tenth), ("no hit", nothing)):
                want = under_poison(env, lambda: dc.range(q, t, metric), f"range {route} {name} metric={metric}")
                assert_same(want, cut(full, t, metric), f"range {route} {name} metric={metric} vs oracle")
                if name == "no hit":
                    assert want[0].tolist() == [0] * (m + 1) and want[1].size == 0
    finally:
        dc.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", [37, 64])
def test_matmul(env, dtype, d):
    rs = np.random.RandomState(d)
    q, c = randn(rs, 67, d, dtype), randn(rs, 301, d, dtype)
    q[3, :] = 0.0
    c[5, :] = -0.0  # (zero sums: the padded dimension's sign pass)
    want = under_poison(env, lambda: (np.array(_native.matmul_host(q, c)),), f"matmul d={d}")
    assert_same(want, (np.asarray(oracle.matmul(q, c)).astype(dtype),), f"matmul d={d} vs oracle")


@pytest.mark.parametrize("kind", ["f32", "f64 fused", "f64 materialised", "bf16"])
def test_three_shards_on_one_device(env, device_list, kind):
    """set_devices([0, 0, 0]): 130 rows in shards of 43, 43 and 44, k = 44 (two shards shorter than k)
    and k = 10, through the host entry and a sharded handle."""
    rs = np.random.RandomState(130)
    f64 = kind.startswith("f64")
    dt = np.float64 if f64 else np.float32
    q, c = randn(rs, 33, 40, dt), randn(rs, 130, 40, dt)
    c[100] = c[3]  # a tie across shards
    if f64:
        env.setenv("PMM_F64_FUSED", "1" if kind == "f64 fused" else "0")
    compute = BF16 if kind == "bf16" else F32
    _native.set_devices([])
    one = {(k, metric): _native.topk_host(q, c, k, metric, compute) for k in (10, 44) for metric in METRICS}
    _native.set_devices([0, 0, 0])
    dc = _native.DeviceCorpus(c, compute="bf16") if kind == "bf16" else _native.DeviceCorpus(c)
    try:
        assert dc.shards == 3
        for (k, metric), want in one.items():
            got = under_poison(env, lambda: _native.topk_host(q, c, k, metric, compute) + dc.topk(q, k, metric),
                               f"{kind} three shards k={k} metric={metric}")
            assert_same(got[:2], want, f"{kind} sharded host entry k={k} metric={metric} vs one device")
            assert_same(got[2:], want, f"{kind} sharded handle k={k} metric={metric} vs one device")
            if kind != "bf16":
                assert_oracle(want, q, c, k, metric, f"{kind} one device k={k}")
    finally:
        _native.set_devices([])
        dc.close()


# ---------------------------------------------------------------------------
# C. Guard bands and free slack, device API
# ---------------------------------------------------------------------------
class Banded:
    """`nbytes` of device memory between two bands of at least GUARD pattern bytes, the inner
    pointer aligned to `align`."""

    def __init__(self, nbytes, align=256, fill=None):
        import torch

        self.t = torch.full((nbytes + 2 * GUARD + align,), PATTERN, dtype=torch.uint8, device="cuda:0")
        self.lo = GUARD + (-(self.t.data_ptr() + GUARD)) % align
        self.hi = self.lo + nbytes
        self.ptr = self.t.data_ptr() + self.lo
        if fill is not None:
            self.t[self.lo:self.hi] = fill

    def inner(self, dtype, shape):
        return self.t[self.lo:self.hi].cpu().numpy().view(dtype).reshape(shape)

    def check(self, label):
        import torch

        assert bool(torch.all(self.t[:self.lo] == PATTERN)), f"{label}: bytes before the buffer were written"
        assert bool(torch.all(self.t[self.hi:] == PATTERN)), f"{label}: bytes behind the buffer were written"


def framed_rows(a, dt, pad, zero_to=None):
    """a's rows inside a taller, wider tensor: 64 rows of NaN before and after, a row stride 64
    elements above the padded width, every slack column NaN; columns d .. zero_to - 1 zero
    (zero_to: roundup(d, pad) where the entry wants zero padding, d where it wants none).
    Returns (tensor, pointer to row 0, row stride)."""
    import torch

    rows, d = a.shape
    dp = roundup(d, pad)
    zero_to = dp if zero_to is None else zero_to
    ld = dp + 64
    t = torch.full((rows + 128, ld), float("nan"), dtype=dt, device="cuda:0")
    t[64:64 + rows, :zero_to] = 0
    t[64:64 + rows, :d] = torch.from_numpy(a).to("cuda:0").to(dt)
    return t, t[64].data_ptr(), ld


def tight_rows(a, dt, pad):
    import torch

    rows, d = a.shape
    t = torch.zeros((rows, roundup(d, pad)), dtype=dt, device="cuda:0")
    t[:, :d] = torch.from_numpy(a).to("cuda:0").to(dt)
    return t, t.data_ptr(), t.shape[1]


GUARDED_CASES = [
    ("f32 fused", 130, 5003, 37, 10, COS, "f32", {}),
    ("f32 fused dot", 33, 1037, 96, 100, DOT, "f32", {}),
    ("f32 screened", 70, 3037, 200, 10, COS, "f32", SCREEN_ON),
    ("f32 materialised", 33, 1037, 37, 1025, EUC, "f32", {}),
    ("bf16 wave-specialised", 130, 16384, 200, 100, COS, "bf16", {}),
    ("bf16 one-wave", 70, 5003, 37, 500, EUC, "bf16", {}),
    ("bf16 widened", 33, 3000, 1000, 100, DOT, "bf16", {}),
    ("f64 fused", 33, 1037, 37, 10, COS, "f64", {"PMM_F64_FUSED": "1"}),
    ("f64 materialised", 33, 1037, 37, 10, EUC, "f64", {"PMM_F64_FUSED": "0"}),
]


@pytest.mark.parametrize("case", GUARDED_CASES, ids=lambda c: c[0])
def test_topk_inside_guard_bands_and_nan_slack(env, case):
    import torch

    label, m, n, d, k, metric, kind, knobs = case
    for name, value in knobs.items():
        env.setenv(name, value)
    tdt, pad, sdt = {"f32": (torch.float32, 32, np.float32), "bf16": (torch.bfloat16, 128, np.float32),
                     "f64": (torch.float64, 16, np.float64)}[kind]
    rs = np.random.RandomState(m + n + d)
    q, c = randn(rs, m, d, np.float64 if kind == "f64" else np.float32), randn(rs, n, d, np.float64 if kind == "f64" else np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    compute = BF16 if kind == "bf16" else F32
    wb = 0 if kind == "f64" else _native.workspace_bytes(m, n, d, k, metric, compute)

    def run(rows_of, banded):
        (hq, pq, ldq), (hc, pc, ldc) = rows_of(q, tdt, pad), rows_of(c, tdt, pad)
        oi = Banded(m * k * 4, fill=0x5A)
        osc = Banded(m * k * np.dtype(sdt).itemsize, fill=0x5A)
        ws = Banded(wb, fill=POISONS[0]) if wb else None
        if kind == "f64":
            _native.topk_f64_device(pq, ldq, m, pc, ldc, n, d, k, metric, oi.ptr, osc.ptr, stream=stream)
        else:
            fn = _native.topk_bf16_device if kind == "bf16" else _native.topk_device
            fn(pq, ldq, m, pc, ldc, n, d, k, metric, oi.ptr, osc.ptr, workspace=ws.ptr, workspace_bytes=wb, stream=stream)
        torch.cuda.synchronize()
        if banded:
            for name, b in (("indices", oi), ("scores", osc), ("workspace", ws)):
                if b is not None:
                    b.check(f"{label} {name}")
        del hq, hc
        return oi.inner(np.uint32, (m, k)), osc.inner(sdt, (m, k))

    want = run(tight_rows, True)
    assert_same(run(framed_rows, True), want, f"{label}: operands inside NaN rows and NaN stride slack")
    if kind != "bf16":
        assert_oracle(want, q, c, k, metric, label)


@pytest.mark.parametrize("entry", ["round", "prepare"])
@pytest.mark.parametrize("d", [37, 200, 256])
def test_rounding_entries_inside_guard_bands(env, entry, d):
    """pmm_round_bf16_device and pmm_screen_prepare_device: the bf16 rows and the per-row arrays
    between guard bands, the f32 rows inside NaN rows with NaN behind column d (their stride
    asks for no padding)."""
    import torch

    rows, ldo = 70, roundup(d, 128)
    rs = np.random.RandomState(d)
    a = randn(rs, rows, d)

    def run(rows_of):
        ht, pa, ld = rows_of(a)
        out = Banded(rows * ldo * 2, fill=0x5A)
        arrs = [Banded(rows * 4, fill=0x5A) for _ in range(4)]
        scal = Banded(8, fill=0)
        if entry == "round":
            _native.round_bf16_device(pa, ld, rows, d, out.ptr, ldo, norm=arrs[0].ptr, inv_norm=arrs[1].ptr, sq=arrs[2].ptr,
                                      sq_factor=arrs[3].ptr)
        else:
            _native.screen_prepare_device(pa, ld, rows, d, out.ptr, ldo, norm=arrs[0].ptr, inv_norm=arrs[1].ptr,
                                          rel=arrs[2].ptr, unsafe=arrs[3].ptr, scalars=scal.ptr)
        torch.cuda.synchronize()
        for j, b in enumerate([out, scal] + arrs):
            b.check(f"{entry} d={d} output {j}")
        del ht
        return (out.inner(np.uint16, (rows, ldo)), scal.inner(np.uint32, (2,))) + tuple(b.inner(np.uint32, (rows,)) for b in arrs)

    want = run(lambda x: tight_rows(x, torch.float32, 1))
    assert_same(run(lambda x: framed_rows(x, torch.float32, 1, zero_to=d)), want, f"{entry} d={d}: rows inside NaN")
    # the rounded rows against torch's round-to-nearest-even cast, zero behind column d
    ref = torch.zeros((rows, ldo), dtype=torch.bfloat16)
    ref[:, :d] = torch.from_numpy(a).to(torch.bfloat16)
    assert np.array_equal(want[0], ref.view(torch.int16).numpy().view(np.uint16)), f"{entry} d={d}: rounded rows"


@pytest.mark.parametrize("entry", ["merge", "strided", "sorted strided"])
def test_merge_entries_inside_guard_bands(env, entry):
    """The three merge entries: outputs between guard bands; the strided entries read lists laid
    out with slack between rows and lists that holds winning entries (index 7, score +inf for
    cosine), which must not enter a list."""
    import torch

    m, lists, k_in, k_out = 37, 5, 40, 100
    rs = np.random.RandomState(5)
    idx = np.stack([np.concatenate([g * 4096 + rs.permutation(4096)[:k_in] for g in range(lists)]) for _ in range(m)])
    idx = idx.reshape(m, lists, k_in).astype(np.uint32)
    sc = rs.randn(m, lists, k_in).astype(np.float32)
    order = np.argsort(-sc, axis=2, kind="stable")  # every list best first
    idx, sc = np.take_along_axis(idx, order, 2), np.take_along_axis(sc, order, 2)
    idx[:, 1, k_in - 5:] = EMPTY_IDX  # a list with empty slots at its end
    sc[:, 1, k_in - 5:] = np.nan
    dev = torch.device("cuda:0")
    # truth: the k_out best of a row's entries, score descending, then index ascending
    fi, fs = idx.reshape(m, -1), sc.reshape(m, -1)
    want_i = np.full((m, k_out), EMPTY_IDX, np.uint32)
    want_s = np.full((m, k_out), EMPTY_SCORE, np.uint32).view(np.float32)
    for r in range(m):
        ok = fi[r] != EMPTY_IDX
        o = np.lexsort((fi[r][ok], -fs[r][ok]))[:k_out]
        want_i[r, :o.size], want_s[r, :o.size] = fi[r][ok][o], fs[r][ok][o]
    if entry == "merge":
        ti = torch.from_numpy(idx.view(np.int32)).to(dev)
        ts = torch.from_numpy(sc).to(dev)
        row_stride, list_stride = lists * k_in, k_in
    else:
        row_stride, list_stride = lists * (k_in + 8) + 16, k_in + 8
        ti = torch.full((m + 1, row_stride), 7, dtype=torch.int32, device=dev)
        ts = torch.full((m + 1, row_stride), float("inf"), dtype=torch.float32, device=dev)
        for g in range(lists):
            ti[:m, g * list_stride:g * list_stride + k_in] = torch.from_numpy(idx[:, g].view(np.int32).copy()).to(dev)
            ts[:m, g * list_stride:g * list_stride + k_in] = torch.from_numpy(sc[:, g].copy()).to(dev)
    oi, osc = Banded(m * k_out * 4, fill=0x5A), Banded(m * k_out * 4, fill=0x5A)
    if entry == "merge":
        _native.merge_device(ti.data_ptr(), ts.data_ptr(), m, lists, k_in, k_out, COS, oi.ptr, osc.ptr)
    else:
        _native.merge_strided_device(ti.data_ptr(), ts.data_ptr(), m, lists, k_in, row_stride, list_stride, k_out, COS,
                                     oi.ptr, osc.ptr, sorted_lists=entry == "sorted strided")
    torch.cuda.synchronize()
    oi.check(f"{entry} indices")
    osc.check(f"{entry} scores")
    assert_same((oi.inner(np.uint32, (m, k_out)), osc.inner(np.float32, (m, k_out))), (want_i, want_s), entry)
