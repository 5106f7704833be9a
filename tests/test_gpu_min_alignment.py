"""The device entries at the weakest layout include/pmm.h allows ("Streams and
alignment").

Torch's allocator hands out bases aligned to 256 bytes or better and the other tests pad strides
by 32 or 64 elements, so 16-byte loads, LDS staging and the output stores never ran at the
alignment the header states as the minimum.  Every case of tests/device_cases.py runs twice: with
tight, 256-byte-aligned operands, and with everything at its minimum --

  bases      256-byte boundary + 16 bytes (pack_sign input, rounding and f32 norms inputs: + 4
             bytes with an odd stride; f64 norms input: + 8)
  strides    f32 roundup(d, 32) + 4, bf16 roundup(d, 128) + 8, int8 roundup(d, 64) + 16, bits
             roundup(w, 16) + 16, f64 roundup(d, 16) + 2; the padding columns zero, every byte
             behind them NaN (floats) or 0x7F (integers)
  outputs    out_idx and f32 scores at + 4 bytes, f64 scores at + 8, the packed bits at + 8 with
             ld_out = roundup(ceil(d / 8), 8), the bf16 rows at + 16, all between guard bands
  workspace  f32 and bf16 entries: boundary + 16, between guard bands, filled with 0xFF

-- and the two results are the same bytes, and the bytes of the CPU truth.

What the entries refuse, decided by reading the code (a misaligned access is not tried out):
  * f64 rows at an odd stride: f64_tile stages its rows with 16-byte loads, so a row must start
    16-byte aligned: the strides are multiples of 2 (PMM_ERR_ARG otherwise);
  * an f32 / bf16 workspace below 16-byte alignment: its regions start at multiples of 256 from
    the base and hold 64-bit keys under atomics, 16-byte fills and the rows the kernels stage with
    16-byte loads (the screen's images, the widened bf16 rows): PMM_ERR_ARG;
  * an int8 / bit workspace that is not 256-byte aligned, as the header already said.
Every refusal names the offending value, writes nothing and leaves the thread usable.
"""
from __future__ import annotations

import os

import pytest

import device_cases as dc
from polars_matmul import _native

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    assert _native.device_count() > 0, "no HIP device visible"
    return monkeypatch


def test_the_weak_layout_is_the_minimum():
    """The table the module rests on, checked against the entries' rules without a device call."""
    for case in dc.TOPK_CASES:
        pad, _, extra, _, soff = dc.TOPK_KINDS[case.kind]
        elem = {"f32": 4, "bf16": 2, "f64": 8, "i8": 1, "bits": 1}[case.kind]
        for op in case.operands:
            assert op.weak_ld == dc.roundup(op.d, pad) + extra and op.weak_off == 16
            assert (op.weak_ld * elem) % 16 == 0 and (op.weak_ld - dc.roundup(op.d, pad)) * elem == 16, case.name
        assert [o.weak_off for o in case.outputs] == [4, soff]


@pytest.mark.parametrize("case", dc.CASES + dc.ODD_K_CASES + dc.FILL_CASES, ids=repr)
def test_weakest_layout_equals_tight(env, case):
    dc.apply_knobs(env, case)
    want = dc.baseline(case)
    got = dc.run_case(case, weak=True)
    dc.assert_outputs(case, got, want, "operands, outputs and workspace at the weakest alignment and stride")
    truth = case.truth
    dc.assert_outputs(case, {**want, **truth}, want, "the tight call against the CPU truth")


@pytest.mark.parametrize("which", ["workspace alone at + 16", "operands and outputs alone at + 16"])
def test_f32_prologue_branch_sees_mixed_alignment(env, which):
    """topk_f32_fused takes its one-launch prologue by the alignment of q, c and the workspace
    together: each alone at the minimum."""
    case = dc.F32_FUSED
    want = dc.expected(case)
    if which.startswith("workspace"):
        got = dc.run_case(case, weak=False, ws_off=16)
    else:
        got = dc.run_case(case, weak=True, ws_off=0)
    dc.assert_outputs(case, got, want, which)


def refused(case, label, needles, weak_ld=None, ws_off=0):
    """The call at tight operands except for the one offending value: PMM_ERR_ARG whose message
    holds every needle, nothing written; then the same call without the offence succeeds."""
    import torch

    ops, outs = dc.place_operands(case, weak=False), dc.place_outputs(case, weak=False)
    if weak_ld:
        ops = {nm: (pl, weak_ld if nm == "q" else ld) for nm, (pl, ld) in ops.items()}
    ws = dc.place_workspace(case, ws_off)
    torch.cuda.synchronize()
    with pytest.raises(_native.PmmError) as err:
        dc.call_placed(case, ops, outs, ws, 0)
    torch.cuda.synchronize()
    assert err.value.code == _native.PMM_ERR_ARG, f"{label}: {err.value}"
    text = _native.last_error()
    assert text == str(err.value)
    for needle in needles(ws):
        assert needle in text, f"{label}: {text!r} does not name {needle!r}"
    dc.assert_untouched(outs, label)
    if ws is not None:
        assert bool(torch.all(ws.view == dc.WS_FILL)), f"{label}: the workspace was written"
        ws.check(f"{label} workspace")
    # the following call on the same thread
    dc.assert_outputs(case, dc.run_case(case), dc.expected(case), f"the call after {label}")


@pytest.mark.parametrize("case", [dc.INT8, dc.BITS], ids=repr)
def test_int8_and_bit_workspace_below_256_is_refused(env, case):
    dc.apply_knobs(env, case)
    refused(case, "a workspace 16 bytes past a 256-byte boundary", lambda ws: ("256-byte-aligned", f"{ws.ptr:#x}"), ws_off=16)


@pytest.mark.parametrize("off", [4, 8])
@pytest.mark.parametrize("case", [dc.F32_FUSED, dc.F32_SCREENED, dc.BF16_WS, dc.BF16_WIDENED], ids=repr)
def test_f32_and_bf16_workspace_below_16_is_refused(env, case, off):
    dc.apply_knobs(env, case)
    refused(case, f"a workspace {off} bytes past a 16-byte boundary", lambda ws: ("16-byte-aligned", f"{ws.ptr:#x}"),
            ws_off=off)


@pytest.mark.parametrize("case", [dc.F64_FUSED, dc.F64_MATERIALISED], ids=repr)
def test_f64_odd_stride_is_refused(env, case):
    """roundup(d, 16) + 1 doubles: every second row would start 8 bytes off a 16-byte boundary."""
    dc.apply_knobs(env, case)
    ld = case.operand("q").tight_ld + 1
    # (the query rows are placed at the tight stride: the entry must refuse before it reads a byte)
    refused(case, f"an odd row stride ldq={ld}", lambda ws: ("multiples of 2", f"ldq={ld}"), weak_ld=ld)
