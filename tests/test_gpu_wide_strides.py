"""The device entries at row strides whose spans pass 2^31 and 2^32 bytes ("Largest
row stride"; the other end of the layout axis of tests/test_gpu_min_alignment.py).

One operand is wide per call, placed on the device (device_cases.place_wide: the poison filled
there, the rows written through a strided view), the others tight; guard bands checked after the
call; outputs bit-equal to the CPU truth and to the tight call.  No tolerances.  Every f32 and
bf16 call runs under pmm_timing_enable and asserts the launch counts of its case
(wide_stride_cases: the tile variant's and the seed form's marks, the kernels' names).

Stride rungs, in bytes, each from the constant it crosses.  R rows of stride S in one span:
"first" has R * S >= 2^31 and (R - 1) * S < 2^32, "both" has (R - 1) * S >= 2^32.

  entry / operand                 span R                         first         both
  f32, bf16 top-k, ldq and ldc    kDescRowsMax = 256 rows of     refused: the largest stride is
                                  one GEMM descriptor            kMaxRowStrideBytes = 8388592
  f64, int8, bit top-k, corpus    the n = 300 rows               2^23 + 512    2^24 + 512
  f64, int8, bit top-k, queries   the m = 33 rows                2^26 + 512    144 MiB + 512
  pack_sign, norms, round_bf16,   the 70 rows                    2^25 + 512    2^26 + 512
    screen_prepare, input rows
  strided merges                  lists * list_stride * 4 bytes  --            5 * (2^28 + 64) * 4

Result per entry and route:

  pmm_topk_f32_device   tile variants 0-5, 5 with PMM_CUS=4, the seeded      refused above 8388592
                        prologue in its three forms, the seed by the GEMM,   bytes; exact at 8388592
                        screened: n = 300, both operands in turn             (256-column tiles: the
                                                                             span ends 4 KiB below
                                                                             2^31)
                        materialised k = 1025 (n = 4099): ldq at the limit, ldc = 2^20 + 512
                        a 512-row seed sample at ldc = 8388592: runs unseeded, exact
  pmm_topk_bf16_device  wave-specialised, one-wave (PMM_BF16_WS=0),          refused above 8388592
                        unseeded, seeded (n = 600, PMM_SEED_NS=64)           bytes; exact at 8388592
                        default 1024-row seed (n = 8192): ldq at the limit, ldc = 2^19 + 512
                        fire-and-forget kernel of libpmm_ff.so (n = 4099, PMM_BF16_FF=2): ldq at
                        the limit (its 64-row spans), ldc = 2^20 + 512
  pmm_topk_f64_device   fused and materialised                               exact at every rung
  pmm_topk_i8_device, pmm_topk_bits_device                                   exact at every rung
  pmm_pack_sign_device, pmm_norms_f32/f64_device, pmm_round_bf16_device,
    pmm_screen_prepare_device, input stride                                  exact at every rung
  pmm_merge_topk_strided_device, pmm_merge_sorted_topk_strided_device        exact

The f32 and bf16 GEMMs read rows through buffer descriptors of at most 2^31 - 1 bytes with 32-bit
offsets; a load past the descriptor returns zeros, so a longer stride would score the far rows of
a tile as zero vectors without a fault.  The entries refuse such a stride before they enqueue
anything (pmm_internal.h kMaxRowStrideBytes).  A threshold seed's descriptor spans its whole
sample; a sample that does not fit is not scored and the call runs unseeded.
tests/test_wide_strides_cpu.py shows on the oracle that these inputs would tell a clamped or
wrapped read, of a tile or of a seed's sample, from the truth.

Left uncovered, and why:
  * bf16 corpus tiles are 32 to 128 rows, so at 8388592 bytes their spans end at 2^30 and below:
    only the f32 256-column tiles sit at the descriptor's end;
  * the bf16 kernels' per-K-step instantiations (PMM_BF16_KS = d / 128) run at 1 and 2 steps
    (d = 37, 256), not at 3 to 6;
  * a bf16 sample too long for one descriptor needs n >= 8 ns rows at more than 2^31 / ns bytes
    each, 17 GB at the least: the unseeded fallback is run for the f32 entry only;
  * the output strides (ld_out, ldo) of the packing and rounding entries stay at their tight
    values; pmm.h and DESIGN.md claim the input strides only.

Wall time on an MI355X: 33 s for the module's 208 tests; the process's first call takes most of
the slowest test's 12 s, every other test is under 3 s.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import pytest

import device_cases as dc
from device_cases import COS
from polars_matmul import _native
from wide_stride_cases import (BF16_CASES, ELEM, F32_CASES, F32_SEED_SKIPPED, FF_CASES, LIMIT_BYTES, MERGE_LIST_STRIDE,
                               ROW_RUNGS, SOUND_CASES, TOPK_RUNGS, refused_strides)

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    assert _native.device_count() > 0, "no HIP device visible"
    yield monkeypatch
    import torch

    torch.cuda.empty_cache()  # (no test leaves its gigabytes to the next one)


@pytest.fixture(scope="module")
def ffn():
    """libpmm_ff.so bound beside libpmm.so (tests/test_gpu_parity.py's fixture)."""
    import importlib.util

    path = os.path.join(os.path.dirname(_native.__file__), "libpmm_ff.so")
    assert os.path.exists(path), "libpmm_ff.so not built (make -C polars-matmul_amd ff)"
    spec = importlib.util.spec_from_file_location("polars_matmul._native_ff", _native.__file__)
    mod = importlib.util.module_from_spec(spec)
    old = os.environ.get("PMM_LIB")
    os.environ["PMM_LIB"] = "libpmm_ff.so"
    try:
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            os.environ.pop("PMM_LIB", None)
        else:
            os.environ["PMM_LIB"] = old
    assert mod.LIB_PATH.endswith("libpmm_ff.so") and mod.lib() is not _native.lib()
    return mod


@contextlib.contextmanager
def launches(case, label, expect=None):
    """The timing records of the calls inside: the case's launch counts, exactly."""
    lib = case.native or _native
    lib.timing_reset()
    lib.timing_enable(True)
    try:
        yield
    finally:
        lib.timing_enable(False)
    for name, want in (case.launches if expect is None else expect).items():
        got = lib.timing_read(name)[1]
        assert got == want, f"{case.name}, {label}: {got} launches of {name!r}, not {want}"
    lib.timing_reset()


def refused(case, name, ld):
    """Tight operands, the stride of `name` alone replaced (the entry must refuse before it reads
    a byte): PMM_ERR_ARG naming the stride and the largest one accepted, nothing written."""
    import torch

    lib = case.native or _native
    ops, outs = dc.place_operands(case, weak=False), dc.place_outputs(case, weak=False)
    ops = {nm: (pl, ld if nm == name else tight) for nm, (pl, tight) in ops.items()}
    ws = dc.place_workspace(case)
    torch.cuda.synchronize()
    with pytest.raises(lib.PmmError) as err:
        dc.call_placed(case, ops, outs, ws, 0)
    torch.cuda.synchronize()
    assert err.value.code == lib.PMM_ERR_ARG, str(err.value)
    text = str(err.value)
    for needle in (f"ld{name}={ld}", f"{LIMIT_BYTES} bytes", f"({LIMIT_BYTES // ELEM[case.kind]} elements)"):
        assert needle in text, f"{case.name}: {text!r} does not name {needle!r}"
    dc.assert_untouched(outs, f"{case.name}: ld{name}={ld}")
    if ws is not None:
        assert bool(torch.all(ws.view == dc.WS_FILL)), f"{case.name}: the workspace was written"


def exact_wide_and_refused_beyond(env, case):
    dc.apply_knobs(env, case)
    with launches(case, "tight"):
        tight = dc.run_case(case)
    want = {**tight, **case.truth}
    dc.assert_outputs(case, tight, want, "the tight call against the CPU truth")
    elem = ELEM[case.kind]
    for name in ("q", "c"):
        with launches(case, f"ld{name} wide"):
            got = dc.run_case(case, wide={name: case.wide[name] // elem})
        dc.assert_outputs(case, got, want, f"ld{name} = {case.wide[name]} bytes")
        del got
        for ld in refused_strides(case.kind):
            refused(case, name, ld)
    # the call after the refusals, on the same thread
    dc.assert_outputs(case, dc.run_case(case), want, "the call after the refusals")
    return want


@pytest.mark.parametrize("case", F32_CASES + BF16_CASES, ids=repr)
def test_largest_stride_is_exact_and_the_next_is_refused(env, case):
    exact_wide_and_refused_beyond(env, case)


@pytest.mark.parametrize("case", FF_CASES, ids=repr)
def test_fire_and_forget_kernel_at_the_largest_query_stride(env, ffn, case):
    case.native = ffn
    try:
        want = exact_wide_and_refused_beyond(env, case)
    finally:
        case.native = None
    # the product's kernels (PMM_BF16_FF has no effect there) give the same lists
    dc.assert_outputs(case, dc.run_case(case), want, "libpmm.so against libpmm_ff.so")


@pytest.mark.parametrize("case", F32_SEED_SKIPPED, ids=repr)
def test_f32_sample_past_one_descriptor_runs_unseeded(env, case):
    """512 sample rows at 8388592 bytes are 2^32: the seed is left out, not run on rows that read
    as zeros; at the tight stride and with the queries wide the same call seeds."""
    dc.apply_knobs(env, case)
    with launches(case, "tight"):
        tight = dc.run_case(case)
    want = {**tight, **case.truth}
    dc.assert_outputs(case, tight, want, "the tight call against the CPU truth")
    with launches(case, "ldq wide"):
        got = dc.run_case(case, wide={"q": LIMIT_BYTES // 4})
    dc.assert_outputs(case, got, want, "ldq at the largest stride")
    with launches(case, "ldc wide", {"gemm_f32_seed": 0, "seed_select": 0, "gemm_f32_topk": 1}):
        got = dc.run_case(case, wide={"c": LIMIT_BYTES // 4})
    dc.assert_outputs(case, got, want, "ldc at the largest stride")


@pytest.mark.parametrize("rung", ["first", "both"])
@pytest.mark.parametrize("name", ["q", "c"])
@pytest.mark.parametrize("case", SOUND_CASES, ids=repr)
def test_f64_int8_and_bit_topk_exact_at_every_rung(env, case, name, rung):
    dc.apply_knobs(env, case)
    want = dc.expected(case)
    dc.assert_outputs(case, dc.baseline(case), want, "the tight call against the CPU truth")
    nbytes = TOPK_RUNGS[name][rung]
    got = dc.run_case(case, wide={name: nbytes // ELEM[case.kind]})
    dc.assert_outputs(case, got, want, f"ld{name} = {nbytes} bytes")


ROW_INPUTS = [c for c in dc.ROW_CASES if c.kind in ("pack", "norms", "rounding")]


@pytest.mark.parametrize("rung", ["first", "both"])
@pytest.mark.parametrize("case", ROW_INPUTS, ids=repr)
def test_row_entries_exact_at_every_input_rung(env, case, rung):
    want = dc.expected(case)
    dc.assert_outputs(case, dc.baseline(case), want, "the tight call against the CPU truth")
    (op,) = case.operands
    got = dc.run_case(case, wide={op.name: ROW_RUNGS[rung] // op.elem})
    dc.assert_outputs(case, got, want, f"input stride {ROW_RUNGS[rung]} bytes")


@pytest.mark.parametrize("sorted_lists", [False, True])
def test_strided_merges_past_4_gib(env, sorted_lists):
    """Five lists per row at list_stride = 2^28 + 64 entries: the last list starts past 2^32
    bytes.  idx and score share one allocation (pmm.h: score = buffer + an offset inside the
    list's slack), 4.3 GB; every byte outside the lists is the poison, the entries of a merge
    case of device_cases."""
    import torch

    base = dc.merge_case("sorted strided merge" if sorted_lists else "strided merge")
    m, lists, k_in, k_out = 37, 5, 40, 100
    row_stride, ls = k_in + 8, MERGE_LIST_STRIDE
    assert lists * ls * 4 > 1 << 32 and m * row_stride * 2 <= ls
    rows = {op.name: op.data for op in base.operands}
    small_ls = k_in + 8  # (the list stride of the base case's image)
    score_off = m * row_stride  # entries between idx and score
    nent = (lists - 1) * ls + score_off + m * row_stride
    pl = dc.Placed(nent * 4, 0, fill=dc.NAN_BYTE)
    dev = pl.view.view(torch.int32)
    for g in range(lists):
        for nm, off in (("idx", 0), ("score", score_off)):
            src = np.ascontiguousarray(rows[nm][:m, g * small_ls:g * small_ls + k_in]).view(np.int32)
            dst = torch.as_strided(dev, (m, k_in), (row_stride, 1), dev.storage_offset() + g * ls + off)
            dst.copy_(torch.from_numpy(src))
    outs = dc.place_outputs(base, weak=False)
    torch.cuda.synchronize()
    _native.merge_strided_device(pl.ptr, pl.ptr + score_off * 4, m, lists, k_in, row_stride, ls, k_out, COS,
                                 outs["idx"].ptr, outs["score"].ptr, 0, sorted_lists=sorted_lists)
    torch.cuda.synchronize()
    pl.check("the lists")
    for nm, o in outs.items():
        o.check(f"output {nm}")
    got = dc.read_outputs(base, outs)
    dc.assert_outputs(base, got, dc.expected(base), "list_stride past 2^32 bytes")
