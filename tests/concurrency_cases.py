"""Shared by the thread tests (tests/test_gpu_concurrency.py,
tests/test_concurrency_cpu.py): the thread frame and the bit-for-bit
comparison of whole results.  A plain module, not a test file.

The frame: every thread has work of its own, all threads leave one barrier
together, each does a fixed number of rounds, the first exception of a thread
is re-raised on the main thread, and no thread may be alive after the join.
"""
from __future__ import annotations

import threading

import numpy as np
import pyarrow as pa

JOIN = 120  # seconds a join waits: far above any test's run time, so a hang fails and does not block


def arrow_parts(arr):
    """A List<Struct{index, score}> column as (offsets, indices, score bits); any other column as its values."""
    if pa.types.is_large_list(arr.type) or pa.types.is_list(arr.type):
        return (arr.offsets.to_numpy(), arr.values.field("index").to_numpy(zero_copy_only=False),
                arr.values.field("score").to_numpy(zero_copy_only=False).view(np.uint64))
    return (np.asarray(arr.to_numpy(zero_copy_only=False)),)


def frozen(x):
    """A result as nested tuples of (dtype, shape, bytes) and plain values: == is bit equality.
    An object with ``__slots__`` (the checked arguments of polars_matmul) is the tuple of its
    slots, without the cache key and the array that keeps its buffers alive."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, pa.Array):
        return frozen(arrow_parts(x))
    if isinstance(x, np.generic):
        return x.item()
    if hasattr(type(x), "__slots__"):
        return tuple(frozen(getattr(x, name)) for name in type(x).__slots__ if name not in ("key", "keep"))
    return x


def assert_bits(got, want, label):
    g, w = frozen(got), frozen(want)
    if g != w:
        parts = [j for j, (a, b) in enumerate(zip(g, w)) if a != b] if isinstance(g, tuple) and len(g) == len(w) else "all"
        raise AssertionError(f"{label}: the bytes differ from the expected result (outputs {parts})")


def run_threads(works, rounds):
    """works[t](round) on thread t, every thread from one barrier, ``rounds`` rounds each.
    Returns results[t][round]; the first exception of a thread is re-raised here."""
    n = len(works)
    start = threading.Barrier(n)
    results = [[None] * rounds for _ in range(n)]
    errors = []

    def body(t):
        try:
            start.wait(timeout=JOIN)
            for r in range(rounds):
                results[t][r] = works[t](r)
        except BaseException as e:  # noqa: BLE001 - re-raised on the main thread
            errors.append((t, e))

    threads = [threading.Thread(target=body, args=(t,)) for t in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=JOIN)
    assert not any(th.is_alive() for th in threads), "a thread is still running"
    if errors:
        t, e = errors[0]
        raise AssertionError(f"thread {t} raised {e!r} ({len(errors)} of {n} threads failed)") from e
    return results
