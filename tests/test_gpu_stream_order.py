"""The device entries' stream contract (include/pmm.h, "Device-resident entry points"; DESIGN.md
§4, "Streams and alignment"): work enqueued on the caller's HIP stream, no host synchronisation.

Every other device-API test passes torch's current stream, the legacy null stream, which
synchronises implicitly with every blocking stream: a kernel, memset or copy put on stream 0 or
on the thread's own stream, or an input read before the caller's stream produced it, passes
there.  Here the caller's stream is a side stream (torch creates them non-blocking: no implicit
ordering with stream 0) and the producer of the inputs is held back on it by a delay:

  1. on s: delay, asynchronous copies of the real rows from pinned memory over operands that
     hold poison (NaN, 0x7F bytes), the entry with stream = s, copies of the outputs into second
     buffers; only then s.synchronize().  Ordered code never races; anything on another stream
     reads the poison or leaves the pattern in the outputs.  A caller's workspace holds 0xFF.
  2. the control, once per module and without the library: the same delay and copy on s, a plain
     read of the operand on a second side stream that does not wait for s must see the poison,
     else the delay is too short and every test of the module fails with that message.
  3. an event recorded right behind the delay is still pending when the entry returns: the entry
     did not block the host.  Asserted for every entry and route that pmm.h promises it for, with
     a caller's workspace or an arena that does not grow; not for the places pmm.h lists as
     synchronising (the screened f32 route, the f64 fused scan, the int8 and bit entries).
  4. two caller streams on one arena (workspace = NULL), 5. a device call in flight when a host
     entry and a handle take the arena, 6. the null stream next to a side stream.

The delay.  Measured on an MI355X with events around the entry on the null stream (tight
operands, a caller's workspace, five calls after a warm-up): the slowest case's entry, "f32
materialised k=1025", takes 0.64 ms (next: bf16 one-wave k=500 and f32 global sort k=3000 at
0.35 ms, the row entries 0.01 ms) = ENTRY_MS.  DELAY_MS = 40 ms is at least twenty times that
(12.8 ms) and at least 20 ms, so launch latency and a busy shared machine do not close the gap;
the module calibrates torch.cuda._sleep's cycle count against events (a chain of large matmuls
where this torch has no _sleep) and the control measures the delay it got.

No graph capture here: arena growth allocates memory, so capturing these entries is out of scope.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import device_cases as dc
import oracle
from polars_matmul import _native

pytestmark = pytest.mark.gpu

ENTRY_MS = 0.64    # the slowest case's entry on the null stream, measured (see the docstring)
DELAY_MS = 40.0    # >= 20 * ENTRY_MS and >= 20 ms
assert DELAY_MS >= 20 * ENTRY_MS and DELAY_MS >= 20.0


@pytest.fixture
def env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    assert _native.device_count() > 0, "no HIP device visible"
    return monkeypatch


class Delay:
    """enqueue(): DELAY_MS of device time on the current torch stream."""

    def __init__(self, ms):
        import torch

        self.ms = ms
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is not None:
            self.unit = 10_000_000  # cycles of whatever clock _sleep counts: calibrated below
            work = lambda: self.sleep(self.unit)
        else:
            self.a = torch.randn(4096, 4096, device="cuda:0")
            work = lambda: torch.mm(self.a, self.a)
        s = torch.cuda.Stream()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            work()  # (the first launch pays the load of the kernel)
            t0.record()
            work()
            t1.record()
        s.synchronize()
        self.unit_ms = t0.elapsed_time(t1)
        assert self.unit_ms > 0.0
        self.repeat = 1.25 * ms / self.unit_ms  # a quarter above the target

    def enqueue(self):
        import torch

        if self.sleep is not None:
            self.sleep(int(self.unit * self.repeat))
        else:
            for _ in range(int(self.repeat) + 1):
                torch.mm(self.a, self.a)


@pytest.fixture(scope="module")
def delay():
    """The delay, after the control has shown that a consumer which does not wait sees the poison."""
    import torch

    assert _native.device_count() > 0, "no HIP device visible"
    d = Delay(DELAY_MS)
    n = 1 << 20
    operand = torch.full((n,), dc.NAN_BYTE, dtype=torch.uint8, device="cuda:0")
    fresh = torch.zeros(n, dtype=torch.uint8).pin_memory()
    seen = torch.full((n,), 0x33, dtype=torch.uint8, device="cuda:0")
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t0.record()
        d.enqueue()
        t1.record()
        operand.copy_(fresh, non_blocking=True)
    with torch.cuda.stream(s2):  # (it does not wait for s)
        seen.copy_(operand, non_blocking=True)
    s2.synchronize()
    early = seen.cpu().numpy()
    s.synchronize()
    got_ms = t0.elapsed_time(t1)
    if not np.all(early == dc.NAN_BYTE):
        pytest.fail(f"the delay is too short: a read on a second stream that does not wait saw {int(np.sum(early == 0))} "
                    f"of {n} fresh bytes behind a delay of {got_ms:.1f} ms: the tests of this module could not fail")
    assert bool(torch.all(operand == 0)), "the control's own copy did not land"
    assert got_ms >= DELAY_MS, f"the delay ran {got_ms:.1f} ms, not the {DELAY_MS} ms the module rests on"
    return d


def delayed_call(case, delay, null_stream=False):
    """The sequence of the module's docstring (1.) for one case.  null_stream: the rows are still
    produced on s behind the delay, but the entry runs on stream 0 after it waited for s.
    Returns (outputs read from the second buffers, whether the producer was still pending when
    the entry returned)."""
    import torch

    s = torch.cuda.Stream()
    ops = dc.place_operands(case, weak=False, filled=False)
    pinned = {nm: torch.from_numpy(case.operand(nm).image(ld)).pin_memory() for nm, (_, ld) in ops.items()}
    outs = dc.place_outputs(case, weak=False)
    second = {nm: torch.full((pl.nbytes,), 0xC3, dtype=torch.uint8, device="cuda:0") for nm, pl in outs.items()}
    ws = dc.place_workspace(case)
    gate = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay.enqueue()
        gate.record()
        for nm, (pl, _) in ops.items():
            pl.view.copy_(pinned[nm], non_blocking=True)
        for o in case.outputs:
            if o.zeroed:
                outs[o.name].view.zero_()
        if not null_stream:
            dc.call_placed(case, ops, outs, ws, s.cuda_stream)
            pending = not gate.query()
            for nm, pl in outs.items():
                second[nm].copy_(pl.view, non_blocking=True)
    if null_stream:
        assert torch.cuda.current_stream().cuda_stream == 0
        torch.cuda.current_stream().wait_stream(s)
        dc.call_placed(case, ops, outs, ws, 0)
        pending = not gate.query()
        for nm, pl in outs.items():
            second[nm].copy_(pl.view, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    s.synchronize()
    dc.check_bands(case, ops, outs, ws, case.name)
    got = {o.name: second[o.name].cpu().numpy().view(o.dtype).reshape(o.shape) for o in case.outputs}
    return got, pending


@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_delayed_producer_ordered_consumer(env, delay, case):
    dc.apply_knobs(env, case)
    # (first: the null-stream baseline also probes the device and grows the arena to the call's
    # need, so neither happens behind the delay)
    want = dc.expected(case)
    got, pending = delayed_call(case, delay)
    dc.assert_outputs(case, got, want, "behind a delayed producer on a side stream")
    if not case.blocks:
        assert pending, f"{case.name}: the producer's delay had run out when the entry returned: the entry blocked the host"


@pytest.mark.parametrize("other", [dc.F32_K7, dc.F64_MATERIALISED, dc.INT8, dc.BITS], ids=repr)
def test_two_caller_streams_on_one_arena(env, delay, other):
    """A on s1 behind the delay, B on s2 at once, A again on s1, all with workspace = NULL: each
    use of the arena waits for the last one's event when it comes from another stream."""
    import torch

    a = dc.F32_FUSED
    for case in (a, other):
        dc.apply_knobs(env, case)
    want_a, want_b = dc.expected(a), dc.expected(other)
    # the warm-up: both needs, so that the sequence never grows the arena (growth synchronises)
    dc.assert_outputs(a, dc.run_case(a, arena=True), want_a, "in the arena")
    dc.assert_outputs(other, dc.run_case(other, arena=True), want_b, "in the arena")
    if other.kind == "f32":
        assert other.workspace_bytes() <= a.workspace_bytes()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ops_a, ops_b = dc.place_operands(a, weak=False), dc.place_operands(other, weak=False)
    outs_a, outs_b, outs_a2 = dc.place_outputs(a, False), dc.place_outputs(other, False), dc.place_outputs(a, False)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        delay.enqueue()
    dc.call_placed(a, ops_a, outs_a, None, s1.cuda_stream)
    dc.call_placed(other, ops_b, outs_b, None, s2.cuda_stream)
    dc.call_placed(a, ops_a, outs_a2, None, s1.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    dc.assert_outputs(a, dc.read_outputs(a, outs_a), want_a, "call A on s1")
    dc.assert_outputs(other, dc.read_outputs(other, outs_b), want_b, "call B on s2")
    dc.assert_outputs(a, dc.read_outputs(a, outs_a2), want_a, "call A' on s1")
    dc.check_bands(a, ops_a, outs_a, None, "call A")
    dc.check_bands(other, ops_b, outs_b, None, "call B")
    dc.check_bands(a, ops_a, outs_a2, None, "call A'")


def test_device_call_in_flight_then_a_host_entry(env, delay):
    """A with workspace = NULL on s1 behind the delay; on the same thread a host entry and a handle
    take the thread's arena on the thread's stream: they wait for A's event."""
    import torch

    a = dc.F32_FUSED
    want_a = dc.expected(a)
    rs = np.random.RandomState(9)
    q, c = rs.randn(33, 37).astype(np.float32), rs.randn(1037, 37).astype(np.float32)
    oi, osc = oracle.topk(q, c, 10, dc.EUC)
    want_host = (np.asarray(oi).astype(np.uint32), np.asarray(osc).astype(np.float32))
    handle = _native.DeviceCorpus(c)
    try:
        # the warm-up: the arena holds the largest of the three needs before the sequence
        _native.topk_host(q, c, 10, dc.EUC)
        handle.topk(q, 10, dc.EUC)
        dc.run_case(a, arena=True)
        s1 = torch.cuda.Stream()
        ops, outs = dc.place_operands(a, weak=False), dc.place_outputs(a, False)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            delay.enqueue()
        dc.call_placed(a, ops, outs, None, s1.cuda_stream)
        host = _native.topk_host(q, c, 10, dc.EUC)
        held = handle.topk(q, 10, dc.EUC)
        s1.synchronize()
    finally:
        handle.close()
    dc.assert_outputs(a, dc.read_outputs(a, outs), want_a, "the device call in flight")
    dc.assert_same(host, want_host, "the host entry behind a device call in flight")
    dc.assert_same(held, want_host, "the handle behind a device call in flight")
    dc.check_bands(a, ops, outs, None, "the device call in flight")


def test_null_stream_next_to_a_side_stream(env, delay):
    """stream = NULL is the HIP default stream: the rows produced on s, the entry on stream 0
    after stream 0 waited for s."""
    case = dc.F32_FUSED
    want = dc.expected(case)
    got, pending = delayed_call(case, delay, null_stream=True)
    dc.assert_outputs(case, got, want, "on the null stream behind a producer on a side stream")
    assert pending, "the entry blocked the host"
