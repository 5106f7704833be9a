"""The fused top-k's route (route_topk in pmm_capi.hip) seen from outside.

CPU: pmm_topk_workspace_bytes is the route's size, so a table of sizes pins
every route and its edges (integer planning: equality, no margin; the library
plans for 256 CUs without a GPU, and an MI355X has 256).  The numbers were
recorded from the build before the route function existed.

GPU: each route runs through the device API in a caller's workspace of exactly
workspace_bytes(...), which shows that the sizer and the executor agree on the
layout; merge_bytes then reads the counts at the offsets the route names.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
from parity import check_topk, dot_scale, round_bf16
from polars_matmul import _native

COS, DOT, EUC = 0, 1, 2
F32, BF16 = _native.COMPUTE_F32, _native.COMPUTE_BF16
METRIC_NAMES = {COS: "cosine", DOT: "dot", EUC: "euclidean"}

# (label, m, n, d, k, metric, compute, PMM_F32_SCREEN, bytes at d, bytes at d padded to 32 (f32) / 128 (bf16))
SIZES = [
    ("f32 fused c1 cosine", 1000, 10000, 256, 10, COS, F32, None, 66153984, 66153984),
    ("f32 fused c1 dot", 1000, 10000, 256, 10, DOT, F32, None, 66065664, 66065664),
    ("f32 fused c1 euclidean", 1000, 10000, 256, 10, EUC, F32, None, 66153984, 66153984),
    ("f32 fused d=100", 1000, 10000, 100, 10, COS, F32, None, 66153984, 66153984),
    ("f32 fused small d=96", 256, 16384, 96, 10, EUC, F32, None, 84152576, 84152576),
    ("f32 fused k=1024", 256, 16384, 256, 1024, DOT, F32, None, 570558720, 570558720),
    ("f32 materialised k=1025", 256, 16384, 256, 1025, DOT, F32, None, 16844032, 16844032),
    ("f32 materialised cosine k=1025 d=100", 100, 5000, 100, 1025, COS, F32, None, 2021120, 2021120),
    ("f32 global sort k=3000", 64, 8192, 96, 3000, COS, F32, None, 10519040, 10519040),
    ("screen on 33x1037x700", 33, 1037, 700, 100, COS, F32, "1", 6932480, 6932480),
    ("screen on 70x3037x768", 70, 3037, 768, 10, COS, F32, "1", 20287488, 20287488),
    ("screen on 33x2037x96", 33, 2037, 96, 10, COS, F32, "1", 6489600, 6489600),
    ("screen on, re-run chunks m=3000", 3000, 20000, 256, 10, COS, F32, "1", 159089152, 159089152),
    ("screen off 33x1037x700", 33, 1037, 700, 100, COS, F32, "0", 2849536, 2849536),
    ("screen off 33x2037x96", 33, 2037, 96, 10, COS, F32, "0", 3741184, 3741184),
    ("screen on, dot stays fused", 33, 1037, 700, 100, DOT, F32, "1", 2840576, 2840576),
    ("screen unset c3 (on)", 100000, 1000000, 768, 100, COS, F32, None, 14466184192, 14466184192),
    ("screen unset long corpus (on)", 1000, 1000000, 768, 100, COS, F32, None, 2027744000, 2027744000),
    ("screen unset 10k x 100k (off)", 10000, 100000, 768, 100, COS, F32, None, 719618304, 719618304),
    ("screen 0 c3", 100000, 1000000, 768, 100, COS, F32, "0", 5373018112, 5373018112),
    ("screen edge k=192", 256, 16384, 256, 192, COS, F32, "1", 278279936, 278279936),
    ("screen edge k=193", 256, 16384, 256, 193, COS, F32, "1", 168038656, 168038656),
    ("screen edge d=768", 256, 16384, 768, 100, COS, F32, "1", 295655168, 295655168),
    ("screen edge d=800", 256, 16384, 800, 100, COS, F32, "1", 134484224, 134484224),
    ("bf16 native k=100", 256, 16384, 256, 100, COS, BF16, None, 134484224, 134484224),
    ("bf16 native k=100 dot d=96", 256, 16384, 96, 100, DOT, BF16, None, 134351104, 134351104),
    ("bf16 native c4", 100000, 1000000, 768, 100, COS, BF16, None, 7389600256, 7389600256),
    ("bf16 native one-wave k=500", 256, 16384, 256, 500, COS, BF16, None, 268701952, 268701952),
    ("bf16 native k=960", 256, 16384, 256, 960, EUC, BF16, None, 268701952, 268701952),
    ("bf16 widened d=1024", 256, 16384, 1024, 100, COS, BF16, None, 202641664, 202641664),
    # (the widened rows are roundup(d, 32) floats wide: a d padded to 128 sizes more)
    ("bf16 widened d=800", 256, 16384, 800, 100, COS, BF16, None, 187732224, 194121984),
    ("bf16 widened k=1000", 256, 16384, 256, 1000, COS, BF16, None, 587731200, 587731200),
    ("bf16 widened k=1500", 64, 8192, 256, 1500, COS, BF16, None, 10584576, 10584576),
    ("bf16 widened d=1024, screen forced (never screens)", 256, 16384, 1024, 100, COS, BF16, "1", 202641664,
     202641664),
]


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    return monkeypatch


def set_screen(monkeypatch, screen):
    if screen is None:
        monkeypatch.delenv("PMM_F32_SCREEN", raising=False)
    else:
        monkeypatch.setenv("PMM_F32_SCREEN", screen)


@pytest.mark.parametrize("case", SIZES, ids=lambda c: c[0])
def test_workspace_bytes_unchanged(clean_env, case):
    _, m, n, d, k, metric, compute, screen, want, want_padded = case
    set_screen(clean_env, screen)
    pad = 32 if compute == F32 else 128
    assert _native.workspace_bytes(m, n, d, k, metric, compute) == want
    assert _native.workspace_bytes(m, n, -(-d // pad) * pad, k, metric, compute) == want_padded
    if compute == F32:
        # callers name d or roundup(d, 32): the same route either way
        assert want == want_padded


# ---------------------------------------------------------------------------
# GPU: the executor runs in exactly the bytes the sizer names
# ---------------------------------------------------------------------------
# (label, m, n, d, k, metric, compute, PMM_F32_SCREEN, fused route: merge_bytes applies)
RUNS = [
    ("f32 fused cosine", 130, 5000, 96, 10, COS, F32, None, True),
    ("f32 fused dot", 130, 5000, 256, 10, DOT, F32, None, True),
    ("f32 fused euclidean k=1024", 64, 4099, 256, 1024, EUC, F32, None, True),
    ("f32 materialised k=1025", 64, 4099, 256, 1025, DOT, F32, None, False),
    ("f32 global sort k=3000", 33, 8192, 96, 3000, COS, F32, None, False),
    ("f32 screened", 70, 3037, 256, 10, COS, F32, "1", True),
    ("f32 screen off", 70, 3037, 256, 10, COS, F32, "0", True),
    ("bf16 native wave-specialised k=100", 130, 16384, 256, 100, COS, BF16, None, True),
    ("bf16 native one-wave k=500", 70, 5000, 96, 500, EUC, BF16, None, True),
    ("bf16 widened d=1024", 70, 3000, 1024, 100, COS, BF16, None, True),
    ("bf16 widened k=1000", 70, 3000, 256, 1000, DOT, BF16, None, True),
    ("bf16 widened k=1500", 33, 3000, 96, 1500, COS, BF16, None, False),
]


def truth_scores(q, c, metric):
    from golden.make_golden import truth_scores as ts

    return ts(q, c, METRIC_NAMES[metric])


def run_in_exact_workspace(m, n, d, k, metric, compute, q, c, ld, index_base=0):
    """One device-API call in a caller's workspace of exactly workspace_bytes(...); returns the lists,
    the workspace and a closure that repeats the call with another workspace size."""
    import torch

    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if compute == BF16 else torch.float32
    tq = torch.zeros((m, ld), dtype=dt, device=dev)
    tc = torch.zeros((n, ld), dtype=dt, device=dev)
    tq[:, :d] = torch.from_numpy(q).to(dev).to(dt)
    tc[:, :d] = torch.from_numpy(c).to(dev).to(dt)
    wb = _native.workspace_bytes(m, n, d, k, metric, compute)
    # (zeroed: this test owns the size; tests/test_gpu_dirty_scratch.py owns the contents)
    ws = torch.zeros(wb, dtype=torch.uint8, device=dev)
    oi = torch.empty((m, k), dtype=torch.int32, device=dev)
    osc = torch.empty((m, k), dtype=torch.float32, device=dev)
    fn = _native.topk_bf16_device if compute == BF16 else _native.topk_device

    def call(nbytes):
        fn(tq.data_ptr(), ld, m, tc.data_ptr(), ld, n, d, k, metric, oi.data_ptr(), osc.data_ptr(),
           index_base=index_base, workspace=ws.data_ptr(), workspace_bytes=nbytes,
           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return oi.cpu().numpy().view(np.uint32), osc.cpu().numpy()

    idx, sc = call(wb)
    return idx, sc, ws, wb, call


@pytest.mark.gpu
@pytest.mark.parametrize("case", RUNS, ids=lambda c: c[0])
def test_route_runs_in_exactly_its_workspace(clean_env, case):
    label, m, n, d, k, metric, compute, screen, fused = case
    assert _native.device_count() > 0, "no HIP device visible"
    set_screen(clean_env, screen)
    rs = np.random.RandomState(m + n + d + k)
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    ld = -(-d // 128) * 128 if compute == BF16 else d
    idx, sc, ws, wb, call = run_in_exact_workspace(m, n, d, k, metric, compute, q, c, ld)
    if compute == BF16:
        q, c = round_bf16(q), round_bf16(c)
    scale = dot_scale(q, c) if metric == DOT else None
    check_topk(idx, sc, truth_scores(q, c, metric), metric != EUC, rtol=1e-5, atol=1e-5, scale=scale, label=label)
    if fused:
        assert _native.merge_bytes(ws.data_ptr(), m, n, d, k, metric, compute) >= m * k * 8
    with pytest.raises(_native.PmmError) as ei:
        call(wb - 1)
    assert ei.value.code == _native.PMM_ERR_ARG


@pytest.mark.gpu
def test_screened_rerun_rows_in_exactly_their_workspace(clean_env, capfd):
    """test_gpu_screen's crowded band (its construction and its assertions on the screen's report) through
    the device API: the rows that overflow are gathered from strided query rows, re-run on the f32 kernel
    inside the caller's exact workspace and scattered back."""
    from test_gpu_screen import same_bits, screen_report

    assert _native.device_count() > 0, "no HIP device visible"
    clean_env.setenv("PMM_CUS", "1")
    clean_env.setenv("PMM_F32_SCREEN", "1")
    clean_env.setenv("PMM_SCREEN_DEBUG", "1")
    rs = np.random.RandomState(3)
    d, k = 128, 10
    v = rs.randn(d).astype(np.float32)
    near = v[None, :] * (1.0 + rs.randn(2000, d).astype(np.float32) * 10.0 ** rs.uniform(-6, -4, (2000, 1)).astype(np.float32))
    c = np.concatenate([rs.randn(1500, d).astype(np.float32), near.astype(np.float32)])
    c = c[rs.permutation(len(c))]
    q = np.concatenate([v[None, :] * np.float32(0.5), rs.randn(34, d).astype(np.float32)])
    capfd.readouterr()
    idx, sc, _, _, _ = run_in_exact_workspace(len(q), len(c), d, k, COS, F32, q, c, ld=d + 32)
    rep = screen_report(capfd)
    assert rep["S"] == 1 and rep["overflowed"] >= 1
    assert rep["rerun_rows"] >= rep["overflowed"] and rep["whole_call_f32"] == 0
    oi, osc = oracle.topk(q, c, k, oracle.COSINE)
    assert np.array_equal(idx.astype(np.int64), np.asarray(oi).astype(np.int64))
    assert same_bits(sc, np.asarray(osc).astype(np.float32))
