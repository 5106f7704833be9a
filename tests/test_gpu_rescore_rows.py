"""The exact re-score's wave-wide row reads (screen_rescore_kernel): the listed
candidates are gathered in groups of 16 rows, one 128-byte line of every row
per step, with the loads two steps ahead of the chains.  What can go wrong is
in the loop's edges: a list shorter or longer than a group or a wave, a partial
last group, a single step per row or an odd number of them, a row with no more
than k live entries (phase 2 alone), a list that outgrows the kernel's and
takes several rounds, strided operands.

Every case drives the screened route (PMM_F32_SCREEN=1) through the device
entry and compares indices and scores bit for bit with the same call under
PMM_F32_SCREEN=0, the f32 kernel.  The PMM_SCREEN_DEBUG report's counts show
that a case really took the path it is meant for.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS = 0
LIST = 256  # kRescoreList (csrc/pmm_kernels.hip)
M_MAX, N_MAX = 129, 5000


@pytest.fixture(scope="module")
def native():
    from polars_matmul import _native

    assert _native.device_count() > 0, "no HIP device visible"
    return _native


def pad32(d):
    return (d + 31) // 32 * 32


_inputs = {}


def inputs(d):
    """The module's operands of dimension d (rows sliced per case), unchanged
    between the cases."""
    if d not in _inputs:
        rs = np.random.RandomState(7000 + d)
        _inputs[d] = (rs.randn(M_MAX, d).astype(np.float32), rs.randn(N_MAX, d).astype(np.float32))
    return _inputs[d]


def screen_report(capfd):
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[pmm screen]")]
    assert len(lines) == 1, f"expected one screened call, saw {len(lines)}"
    rep = {}
    for tok in lines[0].split()[2:]:
        key, val = tok.split("=")
        rep[key] = float(val) if "." in val or "e" in val else int(val)
    return rep


def strided(torch, x, ld):
    """x's rows zero-padded to stride ld on the device."""
    t = torch.zeros((x.shape[0], ld), dtype=torch.float32, device="cuda:0")
    t[:, : x.shape[1]] = torch.from_numpy(x).to("cuda:0")
    return t


def run(native, monkeypatch, capfd, q, c, k, ldq=None, ldc=None):
    """-> the screened call's report, after comparing it with the f32 kernel's
    result bit for bit."""
    import torch

    m, d = q.shape
    n = c.shape[0]
    ldq = ldq or pad32(d)
    ldc = ldc or pad32(d)
    tq, tc = strided(torch, q, ldq), strided(torch, c, ldc)
    stream = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("PMM_SCREEN_DEBUG", "1")
    out = {}
    rep = None
    for mode in ("0", "1"):
        monkeypatch.setenv("PMM_F32_SCREEN", mode)
        wb = native.workspace_bytes(m, n, d, k, COS)
        ws = torch.zeros(wb, dtype=torch.uint8, device="cuda:0")
        oi = torch.empty((m, k), dtype=torch.int32, device="cuda:0")
        osc = torch.empty((m, k), dtype=torch.float32, device="cuda:0")
        capfd.readouterr()
        native.timing_enable(True)
        native.timing_reset()
        try:
            native.topk_device(tq.data_ptr(), ldq, m, tc.data_ptr(), ldc, n, d, k, COS, oi.data_ptr(), osc.data_ptr(),
                               workspace=ws.data_ptr(), workspace_bytes=wb, stream=stream)
            torch.cuda.synchronize()
            _, launches = native.timing_read("merge_topk/rescore")
        finally:
            native.timing_enable(False)
        out[mode] = (oi.cpu().numpy(), osc.cpu().numpy())
        if mode == "1":
            assert launches >= 1, "the exact finish did not run"
            rep = screen_report(capfd)
    label = f"{m}x{n}x{d} k={k} ldq={ldq} ldc={ldc}"
    assert np.array_equal(out["1"][0], out["0"][0]), f"{label}: indices differ from the f32 kernel's"
    assert np.array_equal(out["1"][1].view(np.uint32), out["0"][1].view(np.uint32)), \
        f"{label}: scores differ from the f32 kernel's"
    return rep


@pytest.mark.parametrize("d", [32, 96, 768])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 100, 192])
def test_list_lengths_around_a_group_and_a_wave(native, monkeypatch, capfd, k, d):
    q, c = inputs(d)
    emptied = 0
    for n in (k, k + 1, 300, 5000):
        for m in (1, 33, 129):
            rep = run(native, monkeypatch, capfd, q[:m], c[:n], k)
            print(f"k={k} d={d} n={n} m={m}: S={rep['S']} kept={rep['kept']} rescored={rep['rescored']} "
                  f"max_per_row={rep['max_per_row']} rerun_rows={rep['rerun_rows']}")
            assert rep["whole_call_f32"] == 0
            assert rep["rescored"] <= rep["kept"]
            if n == k:
                # every row has n_r = n <= k live entries: phase 2 alone scores all of them
                assert rep["rescored"] == rep["kept"] == m * n and rep["max_per_row"] == n
            else:
                assert rep["rescored"] >= (m - rep["rerun_rows"]) * k
            if n == 5000:
                emptied += rep["kept"] - rep["rescored"]
                if m == 129:
                    assert rep["S"] > 1, "the corpus was not split: a row's entries lie in one segment"
    # n = 5000: the k-th exact score of phase 1 rules entries out, so phase 2 empties them
    assert emptied > 0


@pytest.mark.parametrize("k,dups", [(10, 300), (100, 400)])
def test_crowded_row_takes_several_rounds(native, monkeypatch, capfd, k, dups):
    # `dups` exact copies of one corpus row and a query along it: the copies'
    # approximate and exact scores are equal, phase 1 takes the k of lowest
    # index, nothing rules the others out, and phase 2's list (dups - k) is
    # longer than the kernel's.  The ties at P and at e_k go to the lower index.
    d = 96
    q, c = inputs(d)
    rs = np.random.RandomState(31 + k)
    c = c[:3000].copy()
    where = np.sort(rs.choice(3000, dups, replace=False))
    c[where] = c[where[0]]
    q = q[:33].copy()
    q[0] = c[where[0]] * np.float32(0.5)
    assert dups - k > LIST
    rep = run(native, monkeypatch, capfd, q, c, k)
    print(f"k={k} dups={dups}: S={rep['S']} kept={rep['kept']} rescored={rep['rescored']} "
          f"max_per_row={rep['max_per_row']} rerun_rows={rep['rerun_rows']} overflowed={rep['overflowed']}")
    assert rep["rerun_rows"] == 0 and rep["whole_call_f32"] == 0, "the crowded row was not finished by the re-score"
    assert rep["max_per_row"] >= dups > k + LIST


@pytest.mark.parametrize("d,ldq,ldc", [(32, 36, 44), (96, 108, 96), (768, 768, 780), (200, 228, 236)])
def test_strided_operands(native, monkeypatch, capfd, d, ldq, ldc):
    q, c = inputs(d)
    for m, n, k in ((33, 300, 65), (129, 5000, 100)):
        rep = run(native, monkeypatch, capfd, q[:m], c[:n], k, ldq=ldq, ldc=ldc)
        assert rep["whole_call_f32"] == 0 and rep["rescored"] >= (m - rep["rerun_rows"]) * k
