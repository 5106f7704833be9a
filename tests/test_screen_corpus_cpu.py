"""CPU side of the screen on cached corpus handles: the footprint formula with
the screen image, the two new C-ABI entries, the one-pass prepare kernel's
resources (hipcc cross-compiles gfx950 here), the residual bound's bracket in
f32 arithmetic, and the corpus cache's re-accounting after a handle grew."""
from __future__ import annotations

import collections
import os
import re
import subprocess
import tempfile

import numpy as np
import pyarrow as pa
import pytest

from isa_util import CSRC, FLAGS, HIPCC, have_hipcc
from polars_matmul import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d, dp, dpb", [(72, 96, 128), (128, 128, 128), (700, 704, 768), (768, 768, 768)])
def test_corpus_device_bytes_with_the_screen_image(d, dp, dpb):
    n = 1000
    plain = n * dp * 4 + 16 * n
    assert _native.corpus_device_bytes(n, d, np.float32) == plain
    assert _native.corpus_device_bytes(n, d, np.float32, screen=False) == plain
    # bf16 rows at stride roundup(d, 128) + a residual and a flag per row
    assert _native.corpus_device_bytes(n, d, np.float32, screen=True) == plain + n * dpb * 2 + 8 * n
    assert _native.corpus_device_bytes(n, d, np.float32, "f32", True) == plain + n * dpb * 2 + 8 * n
    # only f32 handles have an image: the figure of an f64 or a bf16 handle is the plain one
    for dtype, compute in ((np.float64, "f32"), (np.float32, "bf16"), (np.float64, "bf16")):
        assert (_native.corpus_device_bytes(n, d, dtype, compute, screen=True)
                == _native.corpus_device_bytes(n, d, dtype, compute))


def test_library_and_header_have_the_new_entries():
    lib = _native.lib()
    header = open(os.path.join(ROOT, "include", "pmm.h")).read()
    for name in ("pmm_corpus_bytes", "pmm_screen_prepare_device"):
        assert getattr(lib, name) is not None
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(r"^int %s\(" % name, header, re.M), f"include/pmm.h does not declare {name}"


def test_nbytes_without_the_library_entry_is_the_creation_value(monkeypatch):
    import ctypes
    import threading

    class OldLib:  # a library object from before pmm_corpus_bytes
        pass

    monkeypatch.setattr(_native, "_lib", OldLib())
    dc = object.__new__(_native.DeviceCorpus)
    dc._h = ctypes.c_void_p(1234)
    dc._lock = threading.Lock()
    dc._nbytes0 = 4242
    assert dc.nbytes == 4242

    class NewLib:
        def pmm_corpus_bytes(self, h, out):
            out._obj.value = 5000
            return 0

    monkeypatch.setattr(_native, "_lib", NewLib())
    assert dc.nbytes == 5000
    dc._h = ctypes.c_void_p()  # closed
    assert dc.nbytes == 4242


@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_screen_prepare_kernel_uses_no_scratch():
    # 8 parked values, the row's three running sums and up to 7 tail values per lane: all in registers
    from test_kernel_resources import scratch_by_kernel

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bf16.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_bf16.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = {k: v for k, v in scratch_by_kernel(asm).items() if "screen_prepare_kernel" in k}
    assert len(sc) == 1, sorted(sc)
    assert list(sc.values()) == [(0, 0)], f"scratch (bytes, instructions): {sc}"
    name = next(iter(sc))
    body = asm.split(f".amdhsa_kernel {name}")[1].split(".end_amdhsa_kernel")[0]
    lds = [int(l.split()[1]) for l in body.splitlines() if l.strip().startswith(".amdhsa_group_segment_fixed_size")]
    assert lds and 0 < lds[0] <= 40 * 1024, lds  # the parked f32 band: 4 workgroups per CU
    # rows come in and leave as 16-byte accesses
    func = asm.split(f"\n{name}:")[1].split("s_endpgm")[0]
    assert "global_load_dwordx4" in func and "global_store_dwordx4" in func


def test_residual_bound_bracket_holds_in_f32():
    # The kernel's rel = min(sqrt(r2 / n2) (1 + 2^-9), 2^-8) with f32 sums, on the draws of
    # tests/test_gpu_screen_prepare.py: inside rho <= rel <= min(rho (1 + 2^-8) + 2^-20, 2^-8), the bracket
    # that test asserts on the device (sequential f32 sums here: the longest chains any order has).
    import test_gpu_screen_prepare as t

    for d in t.DIMS:
        a, bad = t.draw(d)
        x = a[bad == 0]
        xb = (t.rne_bits(x).astype(np.uint32) << 16).view(np.float32)
        r = (x - xb).astype(np.float32)
        r2 = np.zeros(len(x), np.float32)
        n2 = np.zeros(len(x), np.float32)
        for j in range(d):
            r2 = (r2 + r[:, j] * r[:, j]).astype(np.float32)
            n2 = (n2 + x[:, j] * x[:, j]).astype(np.float32)
        rel = np.minimum(np.sqrt((r2 / n2).astype(np.float32)).astype(np.float32) * np.float32(1 + 2.0 ** -9),
                         np.float32(2.0 ** -8))
        rho = t.rho64(x)
        hi = np.minimum(rho * (1 + 2.0 ** -8) + 2.0 ** -20, 2.0 ** -8)
        assert (rel >= rho).all() and (rel <= hi).all(), d


def test_topk_reaccounts_the_cache_after_a_handle_grew(monkeypatch):
    # an f32 handle grows when its first screened call builds the image: _topk sums the cache again after the
    # call and evicts least-recently-used OTHER entries; the entry in use stays
    from polars_matmul import _polars_matmul as pm

    closed = []

    class StubCorpus:
        def __init__(self, c):
            self.nbytes = c.nbytes
            self.rows = c.shape[0]

        def acquire(self):
            return self

        def release(self):
            pass

        def close(self):
            closed.append(self.rows)

        def topk(self, q, k, metric):
            self.nbytes += 3 << 20  # the image
            return np.zeros((q.shape[0], k), np.uint32), np.zeros((q.shape[0], k), np.float32)

    monkeypatch.setattr(_native, "DeviceCorpus", StubCorpus)
    monkeypatch.setattr(_native, "device_memory", lambda: (1 << 40, 1 << 40))
    monkeypatch.setattr(_native, "get_devices", lambda: [])
    monkeypatch.setattr(pm, "_apply_devices_env", lambda: None)
    monkeypatch.setattr(pm, "_CACHE_ON", True)
    monkeypatch.setattr(pm, "_CACHE_BYTES", 8 << 20)
    monkeypatch.setattr(pm, "_cache", collections.OrderedDict())
    q = np.zeros((2, 128), dtype=np.float32)

    def corpus(rows):  # 2 MiB per 4096 rows
        c = np.zeros((rows, 128), dtype=np.float32)
        return pa.FixedSizeListArray.from_arrays(pa.array(c.reshape(-1)), 128)

    a, b = corpus(4096), corpus(4097)
    pm._topk(q, a, 1, "cosine")  # a: 2 MiB + 3
    assert len(pm._cache) == 1 and closed == []
    pm._topk(q, b, 1, "cosine")  # a 5 + b 5 = 10 MiB > 8: a, the older one, leaves
    assert closed == [4096] and [v[1].rows for v in pm._cache.values()] == [4097]
    pm._topk(q, b, 1, "cosine")  # b alone at 8 MiB: within the bound
    assert closed == [4096] and len(pm._cache) == 1
    pm._topk(q, b, 1, "cosine")  # b alone at 11 MiB: over, but the entry in use is not evicted
    assert closed == [4096] and [v[1].rows for v in pm._cache.values()] == [4097]
