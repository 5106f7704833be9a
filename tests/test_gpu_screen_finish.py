"""The screened path's two-phase exact finish (screen_rescore_kernel): the k
best approximate entries of a row are scored first, and the k-th of their exact
scores rules out most of the rest.  Whatever the plan -- one segment per row,
split units with a surplus per segment, many short segments, a band that
outgrows the kernel's list -- the lists must stay what the f32 kernel and the
CPU oracle return, bit for bit, and the kernel must never gather more than the
single pass it replaces (`rescored <= kept` in the PMM_SCREEN_DEBUG report).

Every case runs with PMM_F32_SCREEN=1 and is compared with the oracle and with
the same call under PMM_F32_SCREEN=0.
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
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pmm screen]")]
    assert lines, "no screened call reported"
    rep = {}
    for tok in lines[0].split()[2:]:
        key, val = tok.split("=")
        rep[key] = float(val) if "." in val or "e" in val else int(val)
    return rep


def both(native, monkeypatch, q, c, k, label):
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
        _, launches = native.timing_read("merge_topk/rescore")
    finally:
        native.timing_enable(False)
    assert launches >= 1, f"{label}: the exact finish did not run"
    assert np.array_equal(i1, i0), f"{label}: indices differ from the unscreened call"
    assert same_bits(s1, s0), f"{label}: scores differ from the unscreened call"
    oi, osc = oracle.topk(q, c, k, oracle.COSINE)
    assert np.array_equal(i1.astype(np.int64), np.asarray(oi).astype(np.int64)), f"{label}: indices differ from the oracle"
    assert same_bits(s1, np.asarray(osc).astype(np.float32)), f"{label}: scores differ from the oracle"
    return i1, s1


def test_whole_block_one_segment(native, monkeypatch, capfd):
    monkeypatch.setenv("PMM_CUS", "1")
    rs = np.random.RandomState(11)
    capfd.readouterr()
    both(native, monkeypatch, rs.randn(70, 200), rs.randn(9037, 200), 100, "whole blocks")
    rep = screen_report(capfd)
    assert rep["S"] == 1 and rep["rerun_rows"] == 0
    assert rep["rescored"] <= rep["kept"]
    assert rep["max_per_row"] <= rep["capg"]


def test_split_units_with_a_surplus_per_segment(native, monkeypatch, capfd):
    # Eight split units of 18 tiles, unseeded, compaction trigger 47, k = 10:
    # every segment keeps the band under its own k-th, several times what the
    # row needs.  The k-th exact score of the row's k best must rule most of
    # them out (test_screen_finish_cpu.py: the rule alone, on this seed).
    monkeypatch.setenv("PMM_CUS", "8")
    monkeypatch.setenv("PMM_CTRIG", "47")
    monkeypatch.setenv("PMM_BF16_SEED", "0")
    rs = np.random.RandomState(12)
    capfd.readouterr()
    both(native, monkeypatch, rs.randn(70, 200), rs.randn(9037, 200), 10, "compacting split units")
    rep = screen_report(capfd)
    assert rep["S"] == 8 and rep["tps"] == 18 and rep["rerun_rows"] == 0
    print(f"kept {rep['kept']} rescored {rep['rescored']} max_per_row {rep['max_per_row']}")
    assert rep["rescored"] < rep["kept"]
    assert rep["rescored"] >= 70 * 10


def test_default_plan_one_tile_split_units(native, monkeypatch, capfd):
    # many segments with fewer than k entries each: the selection spans them
    rs = np.random.RandomState(11)
    capfd.readouterr()
    both(native, monkeypatch, rs.randn(70, 200), rs.randn(9037, 200), 100, "one-tile split units")
    rep = screen_report(capfd)
    assert rep["S"] > 1 and rep["rerun_rows"] == 0
    assert 70 * 100 <= rep["rescored"] <= rep["kept"]


def test_exact_duplicates_go_to_the_lower_index(native, monkeypatch, capfd):
    rs = np.random.RandomState(5)
    base = rs.randn(40, 64).astype(np.float32)
    c = np.concatenate([base] * 30)  # every corpus row 30 times: the k-th falls inside a run of ties
    q = rs.randn(33, 64).astype(np.float32)
    capfd.readouterr()
    i1, s1 = both(native, monkeypatch, q, c, 100, "duplicates")
    rep = screen_report(capfd)
    assert rep["rescored"] <= rep["kept"]
    for r in range(i1.shape[0]):
        tie = s1[r, 1:] == s1[r, :-1]
        assert tie.any()
        assert np.all(i1[r, 1:][tie].astype(np.int64) > i1[r, :-1][tie].astype(np.int64))


# n_r <= k (k = n; n just above k with d = 1), m = 1 and 33, padded K != d
@pytest.mark.parametrize("m,n,d,k", [(1, 1, 1, 1), (33, 10, 128, 10), (70, 47, 128, 47), (70, 137, 1, 100),
                                     (1, 1037, 37, 10), (33, 1037, 700, 100), (1, 3000, 700, 1), (33, 3037, 37, 10)])
def test_few_entries_and_edges(native, monkeypatch, capfd, m, n, d, k):
    rs = np.random.RandomState(1000 * m + n + d + k)
    capfd.readouterr()
    both(native, monkeypatch, rs.randn(m, d), rs.randn(n, d), k, f"{m}x{n}x{d} k={k}")
    rep = screen_report(capfd)
    assert rep["rescored"] <= rep["kept"]
    if n == k:
        assert rep["rescored"] == rep["kept"] == m * n


def crowd(rs, d):
    # ~2000 near-copies of one vector at relative spacing 1e-4 .. 1e-6 and a
    # query aligned with it: far more than a segment holds within 2 eps of the k-th
    v = rs.randn(d).astype(np.float32)
    near = v[None, :] * (1.0 + rs.randn(2000, d).astype(np.float32) * 10.0 ** rs.uniform(-6, -4, (2000, 1)).astype(np.float32))
    c = np.concatenate([rs.randn(1500, d).astype(np.float32), near.astype(np.float32)])
    c = c[rs.permutation(len(c))]
    q = np.concatenate([v[None, :] * np.float32(0.5), rs.randn(34, d).astype(np.float32)])
    return q, c


def test_crowded_band_overflows_and_reruns(native, monkeypatch, capfd):
    # one workgroup: the row's single segment sees the whole crowd, overflows
    # and is re-run; the kernel walks a full segment and the other rows stay exact
    monkeypatch.setenv("PMM_CUS", "1")
    q, c = crowd(np.random.RandomState(3), 128)
    capfd.readouterr()
    both(native, monkeypatch, q, c, 10, "crowded band")
    rep = screen_report(capfd)
    assert rep["S"] == 1 and rep["overflowed"] >= 1
    assert rep["rerun_rows"] >= rep["overflowed"] and rep["whole_call_f32"] == 0
    assert rep["rescored"] <= rep["kept"]


def test_crowded_band_over_split_units(native, monkeypatch, capfd):
    # the same crowd cut into split units: the crowded row's live entries lie
    # in several segments and outnumber the kernel's list, which then takes
    # several rounds
    q, c = crowd(np.random.RandomState(3), 128)
    capfd.readouterr()
    both(native, monkeypatch, q, c, 10, "crowded band, split units")
    rep = screen_report(capfd)
    assert rep["S"] > 1
    assert rep["rescored"] <= rep["kept"]
    print(f"max_per_row {rep['max_per_row']} overflowed {rep['overflowed']}")


def test_device_entry_prepares_both_operands_in_one_read_each(native, monkeypatch):
    import torch

    rs = np.random.RandomState(7)
    m, n, d, k, base = 33, 2037, 96, 10, 12345
    q, c = rs.randn(m, d).astype(np.float32), rs.randn(n, d).astype(np.float32)
    dev = torch.device("cuda:0")
    tq, tc = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PMM_F32_SCREEN", mode)
        wb = native.workspace_bytes(m, n, d, k, COS)
        ws = torch.zeros(wb, dtype=torch.uint8, device=dev)
        oi = torch.empty((m, k), dtype=torch.int32, device=dev)
        osc = torch.empty((m, k), dtype=torch.float32, device=dev)
        native.timing_enable(True)
        native.timing_reset()
        try:
            native.topk_device(tq.data_ptr(), d, m, tc.data_ptr(), d, n, d, k, COS, oi.data_ptr(), osc.data_ptr(),
                               index_base=base, workspace=ws.data_ptr(), workspace_bytes=wb, stream=stream)
            torch.cuda.synchronize()
            _, rounds = native.timing_read("norms_f32/round")
        finally:
            native.timing_enable(False)
        out[mode] = (oi.cpu().numpy(), osc.cpu().numpy())
        if mode == "1":
            assert rounds == 1, "the device entry's preparation is one timed stage"
            with pytest.raises(native.PmmError) as ei:
                native.topk_device(tq.data_ptr(), d, m, tc.data_ptr(), d, n, d, k, COS, oi.data_ptr(),
                                   osc.data_ptr(), index_base=base, workspace=ws.data_ptr(),
                                   workspace_bytes=wb - 1, stream=stream)
            assert ei.value.code == native.PMM_ERR_ARG
    assert np.array_equal(out["0"][0], out["1"][0]) and same_bits(out["0"][1], out["1"][1])
    oi, osc = oracle.topk(q, c, k, oracle.COSINE)
    assert np.array_equal(out["1"][0].astype(np.int64), np.asarray(oi).astype(np.int64) + base)
    assert same_bits(out["1"][1], np.asarray(osc).astype(np.float32))
