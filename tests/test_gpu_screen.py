"""Screened f32 top-k (cosine): the bf16 screen + exact f32 re-score must return
what the f32 kernel returns, bit for bit -- the same indices, the same f32
scores, the same tie order -- and so what the CPU oracle returns.

Every case runs with PMM_F32_SCREEN=1 (forced wherever the path's limits
allow) and is compared with the oracle and with the same call under
PMM_F32_SCREEN=0.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

COS = 0


@pytest.fixture(scope="module")
def native():
    from polars_matmul import _native

    assert _native.device_count() > 0, "no HIP device visible"
    return _native


def same_bits(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def screen_report(capfd):
    """The screened call's own report (PMM_SCREEN_DEBUG): plan, overflowed and re-run rows."""
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pmm screen]")]
    assert lines, "no screened call reported"
    rep = {}
    for tok in lines[0].split()[2:]:
        key, val = tok.split("=")
        rep[key] = float(val) if "." in val or "e" in val else int(val)
    return rep


def both(native, monkeypatch, q, c, k, label, expect_screen=True):
    """screen on == screen off == oracle; returns the screened result."""
    monkeypatch.setenv("PMM_SCREEN_DEBUG", "1")
    q = np.ascontiguousarray(q, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    monkeypatch.setenv("PMM_F32_SCREEN", "0")
    i0, s0 = native.topk_host(q, c, k, COS)
    monkeypatch.setenv("PMM_F32_SCREEN", "1")
    native.timing_enable(True)
    native.timing_reset()
    try:
        i1, s1 = native.topk_host(q, c, k, COS)
        _, launches = native.timing_read("/screen")
    finally:
        native.timing_enable(False)
    if expect_screen:
        assert launches >= 1, f"{label}: the screened path did not run"
    assert np.array_equal(i1, i0), f"{label}: indices differ from the unscreened call"
    assert same_bits(s1, s0), f"{label}: scores differ from the unscreened call"
    oi, osc = oracle.topk(q, c, k, oracle.COSINE)
    assert np.array_equal(i1.astype(np.int64), np.asarray(oi).astype(np.int64)), f"{label}: indices differ from the oracle"
    assert same_bits(s1, np.asarray(osc).astype(np.float32)), f"{label}: scores differ from the oracle"
    return i1, s1


# m not a multiple of the 32-row wave; n the smallest allowed (k) and k + 37
# style sizes that are no multiple of the 64-column tile; d padded to 128;
# k = 1, 10, 100 and k = n
SHAPES = [
    # (m, n, d, k)
    (1, 1, 1, 1), (1, 38, 37, 1), (33, 10, 128, 10), (33, 47, 700, 10), (70, 100, 768, 100),
    (70, 137, 1, 100), (1, 137, 768, 100), (33, 100, 37, 100), (70, 47, 128, 47), (33, 1037, 700, 100),
    (70, 1037, 37, 10), (1, 3000, 128, 1), (70, 3037, 768, 10),
]


@pytest.mark.parametrize("m,n,d,k", SHAPES)
def test_screen_matches_f32_and_oracle(native, monkeypatch, m, n, d, k):
    rs = np.random.RandomState(1000 * m + n + d + k)
    both(native, monkeypatch, rs.randn(m, d), rs.randn(n, d), k, f"{m}x{n}x{d} k={k}")


def test_screen_index_base_device_api(native, monkeypatch):
    import torch

    rs = np.random.RandomState(7)
    m, n, d, k, base = 33, 2037, 96, 10, 12345
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    dev = torch.device("cuda:0")
    tq, tc = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PMM_F32_SCREEN", mode)
        wb = native.workspace_bytes(m, n, d, k, COS)
        ws = torch.zeros(wb, dtype=torch.uint8, device=dev)
        oi = torch.empty((m, k), dtype=torch.int32, device=dev)
        osc = torch.empty((m, k), dtype=torch.float32, device=dev)
        native.topk_device(tq.data_ptr(), d, m, tc.data_ptr(), d, n, d, k, COS, oi.data_ptr(), osc.data_ptr(),
                           index_base=base, workspace=ws.data_ptr(), workspace_bytes=wb,
                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out[mode] = (oi.cpu().numpy(), osc.cpu().numpy())
        if mode == "1":
            # the merge bytes of a screened call; a workspace one byte short is refused
            assert native.merge_bytes(ws.data_ptr(), m, n, d, k, COS) >= m * k * 8
            with pytest.raises(native.PmmError) as ei:
                native.topk_device(tq.data_ptr(), d, m, tc.data_ptr(), d, n, d, k, COS, oi.data_ptr(),
                                   osc.data_ptr(), index_base=base, workspace=ws.data_ptr(),
                                   workspace_bytes=wb - 1, stream=torch.cuda.current_stream().cuda_stream)
            assert ei.value.code == native.PMM_ERR_ARG
    assert np.array_equal(out["0"][0], out["1"][0]) and same_bits(out["0"][1], out["1"][1])
    oi, osc = oracle.topk(q, c, k, oracle.COSINE)
    assert np.array_equal(out["1"][0].astype(np.int64), np.asarray(oi).astype(np.int64) + base)
    assert same_bits(out["1"][1], np.asarray(osc).astype(np.float32))


def test_screen_split_units_default_plan(native, monkeypatch, capfd):
    # default planning cuts one query block's corpus into one-tile split units
    rs = np.random.RandomState(11)
    capfd.readouterr()
    both(native, monkeypatch, rs.randn(70, 200), rs.randn(9037, 200), 100, "one-tile split units")
    rep = screen_report(capfd)
    assert rep["S"] > 1 and rep["qb_full"] == 0


def test_screen_split_units_share_compacted_thresholds(native, monkeypatch, capfd):
    # Eight split units of 18 tiles each, unseeded, compaction trigger 47
    # (capg 256, k = 10): every unit starts at "accept all", so its first tile
    # alone (64 columns) passes the trigger -- every unit compacts, publishes
    # a_k - eps through gthr and prunes with the other units' bounds
    monkeypatch.setenv("PMM_CUS", "8")
    monkeypatch.setenv("PMM_CTRIG", "47")
    monkeypatch.setenv("PMM_BF16_SEED", "0")
    rs = np.random.RandomState(12)
    capfd.readouterr()
    both(native, monkeypatch, rs.randn(70, 200), rs.randn(9037, 200), 10, "compacting split units")
    rep = screen_report(capfd)
    assert rep["S"] == 8 and rep["tps"] == 18 and rep["qb_full"] == 0 and rep["ctrig"] == 47
    assert rep["rerun_rows"] == 0


def test_screen_whole_blocks(native, monkeypatch, capfd):
    # planned for one workgroup the query block runs whole (one segment per row)
    monkeypatch.setenv("PMM_CUS", "1")
    rs = np.random.RandomState(11)
    capfd.readouterr()
    both(native, monkeypatch, rs.randn(70, 200), rs.randn(9037, 200), 100, "whole blocks")
    rep = screen_report(capfd)
    assert rep["qb_full"] == 1 and rep["S"] == 1


def test_screen_crowded_band_overflows_and_reruns(native, monkeypatch, capfd):
    # ~2000 near-copies of one vector at relative spacing 1e-4 .. 1e-6 and a
    # query aligned with it: far more than a segment holds within 2 eps of the
    # k-th, so the row overflows and the f32 kernel finishes it.  Planned for
    # one workgroup: the row's single segment (capg 256) sees the whole crowd.
    monkeypatch.setenv("PMM_CUS", "1")
    rs = np.random.RandomState(3)
    d, k = 128, 10
    v = rs.randn(d).astype(np.float32)
    near = v[None, :] * (1.0 + rs.randn(2000, d).astype(np.float32) * 10.0 ** rs.uniform(-6, -4, (2000, 1)).astype(np.float32))
    c = np.concatenate([rs.randn(1500, d).astype(np.float32), near.astype(np.float32)])
    c = c[rs.permutation(len(c))]
    q = np.concatenate([v[None, :] * np.float32(0.5), rs.randn(34, d).astype(np.float32)])
    capfd.readouterr()
    both(native, monkeypatch, q, c, k, "crowded band")
    rep = screen_report(capfd)
    assert rep["S"] == 1 and rep["overflowed"] >= 1
    assert rep["rerun_rows"] >= rep["overflowed"] and rep["whole_call_f32"] == 0


def test_screen_exact_duplicates_go_to_the_lower_index(native, monkeypatch):
    rs = np.random.RandomState(5)
    base = rs.randn(40, 64).astype(np.float32)
    c = np.concatenate([base] * 30)  # every corpus row 30 times
    q = rs.randn(33, 64).astype(np.float32)
    i1, s1 = both(native, monkeypatch, q, c, 100, "duplicates")
    # equal scores are listed in ascending index order
    for r in range(i1.shape[0]):
        tie = s1[r, 1:] == s1[r, :-1]
        assert np.all(i1[r, 1:][tie].astype(np.int64) > i1[r, :-1][tie].astype(np.int64))


def test_screen_worst_case_rounding(native, monkeypatch):
    rs = np.random.RandomState(9)
    m, n, d, k = 33, 1037, 700, 10
    # every element a half-ulp tie of bf16, (1 + 2^-8) 2^e, mixed signs
    tie = np.float32(1.0 + 2.0 ** -8)
    q = (tie * np.exp2(rs.randint(-2, 3, (m, d))) * rs.choice([-1.0, 1.0], (m, d))).astype(np.float32)
    c = (tie * np.exp2(rs.randint(-2, 3, (n, d))) * rs.choice([-1.0, 1.0], (n, d))).astype(np.float32)
    both(native, monkeypatch, q, c, k, "half-ulp ties")
    # elements spanning 2^-30 .. 2^30 within a row
    q = (rs.randn(m, d) * np.exp2(rs.randint(-30, 31, (m, d)))).astype(np.float32)
    c = (rs.randn(n, d) * np.exp2(rs.randint(-30, 31, (n, d)))).astype(np.float32)
    both(native, monkeypatch, q, c, k, "wide range")
    # one dominant element per row
    q = rs.randn(m, d).astype(np.float32)
    c = rs.randn(n, d).astype(np.float32)
    q[np.arange(m), rs.randint(0, d, m)] = 1000.0
    c[np.arange(n), rs.randint(0, d, n)] *= 997.0
    both(native, monkeypatch, q, c, k, "dominant element")


@pytest.mark.parametrize("where", ["query", "corpus"])
@pytest.mark.parametrize("what", ["zero-row", "nan", "inf", "subnormal", "above-bf16-max"])
def test_screen_unsafe_inputs_fall_back(native, monkeypatch, capfd, where, what):
    """A value above the largest finite bf16 overflows the row's norm: its finite dots
    then score +-0.0, whose sign the lists must keep as the oracle does."""
    rs = np.random.RandomState(13)
    q = rs.randn(33, 100).astype(np.float32)
    c = rs.randn(1037, 100).astype(np.float32)
    a = q if where == "query" else c
    if what == "zero-row":
        a[5, :] = 0.0
    else:
        a[5, 17] = {"nan": np.nan, "inf": np.inf, "subnormal": 1e-40, "above-bf16-max": 3.4e38}[what]
    capfd.readouterr()
    both(native, monkeypatch, q, c, 10, f"{what} in a {where} row")
    rep = screen_report(capfd)
    if where == "query":  # the row is re-run on the f32 kernel
        assert rep["rerun_rows"] >= 1 and rep["corpus_unsafe"] == 0 and rep["whole_call_f32"] == 0
    else:  # the whole call goes to the f32 kernel
        assert rep["corpus_unsafe"] == 1 and rep["whole_call_f32"] == 1


def test_small_call_takes_the_unscreened_path_by_default(native, monkeypatch):
    monkeypatch.delenv("PMM_F32_SCREEN", raising=False)
    rs = np.random.RandomState(17)
    q, c = rs.randn(1000, 256).astype(np.float32), rs.randn(10000, 256).astype(np.float32)
    native.timing_enable(True)
    native.timing_reset()
    try:
        native.topk_host(q, c, 10, COS)
        _, screened = native.timing_read("/screen")
        _, fused = native.timing_read("gemm_f32_topk")
    finally:
        native.timing_enable(False)
    assert screened == 0 and fused >= 1
