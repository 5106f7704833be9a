"""ctypes binding of ``libpmm.so`` (the C ABI declared in ``include/pmm.h``).

The reference binds its numerics through pyo3 (src/lib.rs:15-62); this module
is the equivalent binding for the HIP library.  ctypes releases the GIL for
the duration of every foreign call, as ``py.detach`` does in src/lib.rs:25/45.

There is no CPU fallback: if ``libpmm.so`` is missing, importing this module
raises ImportError; if no gfx950 device is visible, every compute call raises
RuntimeError with the library's message.
"""
from __future__ import annotations

import atexit
import collections
import ctypes
import importlib.util
import os
import sys
import threading

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        # diagnostics only: PMM_LIB=libpmm_stats.so (make stats) adds the
                        # bf16 kernels' per-phase cycle counters (PMM_STATS=1)
                        os.environ.get("PMM_LIB", "libpmm.so"))

PMM_OK = 0
PMM_ERR_ARG = 1
PMM_ERR_HIP = 2
PMM_ERR_UNSUPPORTED = 3
PMM_ERR_NODEVICE = 4

METRIC_COSINE = 0
METRIC_DOT = 1
METRIC_EUCLIDEAN = 2

COMPUTE_F32 = 0
COMPUTE_BF16 = 1

# Every symbol include/pmm.h declares (checked by tests/test_boundary.py).
EXPORTED_SYMBOLS = (
    "pmm_version",
    "pmm_last_error",
    "pmm_metric_from_str",
    "pmm_metric_higher_is_better",
    "pmm_device_count",
    "pmm_device_memory",
    "pmm_set_device",
    "pmm_set_devices",
    "pmm_get_devices",
    "pmm_shard_plan",
    "pmm_topk_f32",
    "pmm_topk_f32_ex",
    "pmm_topk_f64",
    "pmm_topk_f64_device",
    "pmm_matmul_f32",
    "pmm_matmul_f64",
    "pmm_host_alloc",
    "pmm_host_free",
    "pmm_topk_workspace_bytes",
    "pmm_topk_merge_bytes",
    "pmm_topk_f32_device",
    "pmm_topk_bf16_device",
    "pmm_merge_topk_device",
    "pmm_merge_topk_strided_device",
    "pmm_merge_sorted_topk_strided_device",
    "pmm_norms_f32_device",
    "pmm_norms_f64_device",
    "pmm_round_bf16_device",
    "pmm_screen_prepare_device",
    "pmm_corpus_create_f32",
    "pmm_corpus_create_f64",
    "pmm_corpus_create_bf16",
    "pmm_corpus_dtype",
    "pmm_corpus_destroy",
    "pmm_corpus_info",
    "pmm_corpus_shards",
    "pmm_corpus_bytes",
    "pmm_corpus_subset_ids",
    "pmm_corpus_subset_mask",
    "pmm_corpus_index_map",
    "pmm_partition_plan",
    "pmm_corpus_partition",
    "pmm_corpus_groups",
    "pmm_topk_f32_grouped",
    "pmm_topk_f64_grouped",
    "pmm_probe_plan",
    "pmm_topk_f32_probed",
    "pmm_topk_f32_corpus",
    "pmm_topk_f64_corpus",
    "pmm_topk_bf16_corpus",
    "pmm_range_f32_corpus",
    "pmm_topk_f32_candidates",
    "pmm_corpus_create_f32_docs",
    "pmm_corpus_docs",
    "pmm_topk_f32_maxsim",
    "pmm_kmeans_f32_corpus",
    "pmm_range_f32_self",
    "pmm_topk_f32_self",
    "pmm_components_f32_self",
    "pmm_range_self_plan",
    "pmm_sort_plan",
    "pmm_topk_i8",
    "pmm_topk_i8_corpus",
    "pmm_topk_i8_device",
    "pmm_topk_i8_workspace_bytes",
    "pmm_corpus_create_i8",
    "pmm_pack_sign_device",
    "pmm_corpus_create_bits",
    "pmm_corpus_sign_bits",
    "pmm_corpus_bits_rows",
    "pmm_topk_bits",
    "pmm_topk_bits_corpus",
    "pmm_topk_bits_workspace_bytes",
    "pmm_topk_bits_device",
    "pmm_timing_enable",
    "pmm_timing_reset",
    "pmm_timing_read",
)

def _preload_hip_runtime() -> None:
    """PyTorch-ROCm ships its own libamdhip64.so (SONAME libamdhip64.so.7, as
    /opt/rocm's).  Whichever is loaded first serves the whole process; if
    libpmm.so pulled in /opt/rocm's runtime first, a later `import torch`
    would run on a runtime it was not built against.  When torch is installed
    (and not yet imported), its runtime library is loaded here by path --
    without importing torch -- so libpmm.so and any later torch share it and
    torch device pointers / streams can be passed to the C ABI."""
    if os.environ.get("PMM_NO_TORCH_PRELOAD") == "1" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    hip = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(hip):
        try:
            ctypes.CDLL(hip, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


_preload_hip_runtime()

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"polars_matmul: HIP library not built ({LIB_PATH} missing). "
        "Run `make -C polars-matmul_amd` or `python -c 'import __graft_entry__ as g; g.build()'`."
    )

_lib = ctypes.CDLL(LIB_PATH)

_vp, _i64, _i32, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_u32 = ctypes.c_uint32

_SIGS = {
    "pmm_version": ([], ctypes.c_char_p),
    "pmm_last_error": ([], ctypes.c_char_p),
    "pmm_metric_from_str": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)], _i32),
    "pmm_metric_higher_is_better": ([_i32], _i32),
    "pmm_device_count": ([ctypes.POINTER(ctypes.c_int)], _i32),
    "pmm_device_memory": ([ctypes.POINTER(_sz), ctypes.POINTER(_sz)], _i32),
    "pmm_set_device": ([_i32], _i32),
    "pmm_set_devices": ([ctypes.POINTER(ctypes.c_int), _i32], _i32),
    "pmm_get_devices": ([ctypes.POINTER(ctypes.c_int), _i32, ctypes.POINTER(ctypes.c_int)], _i32),
    "pmm_shard_plan": ([ctypes.POINTER(ctypes.c_int), _i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32,
                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                        ctypes.POINTER(ctypes.c_int)], _i32),
    "pmm_topk_f32": ([_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_topk_f32_ex": ([_vp, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp], _i32),
    "pmm_topk_f64": ([_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_topk_f64_device": ([_vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _u32, _vp, _vp, _vp], _i32),
    "pmm_matmul_f32": ([_vp, _i64, _vp, _i64, _i64, _vp], _i32),
    "pmm_matmul_f64": ([_vp, _i64, _vp, _i64, _i64, _vp], _i32),
    "pmm_host_alloc": ([_sz, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_host_free": ([_vp], _i32),
    "pmm_topk_workspace_bytes": ([_i64, _i64, _i64, _i64, _i32, _i32], _sz),
    "pmm_topk_merge_bytes": ([_vp, _i64, _i64, _i64, _i64, _i32, _i32, ctypes.POINTER(ctypes.c_uint64)], _i32),
    "pmm_topk_f32_device": (
        [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _u32, _vp, _vp, _vp, _sz, _vp],
        _i32,
    ),
    "pmm_topk_bf16_device": (
        [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _u32, _vp, _vp, _vp, _sz, _vp], _i32
    ),
    "pmm_merge_topk_device": ([_vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_merge_topk_strided_device": (
        [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_merge_sorted_topk_strided_device": (
        [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_norms_f32_device": ([_vp, _i64, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_norms_f64_device": ([_vp, _i64, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_round_bf16_device": ([_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp], _i32),
    "pmm_screen_prepare_device": ([_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "pmm_corpus_create_f32": ([_vp, _i64, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_create_bf16": ([_vp, _i64, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_create_f64": ([_vp, _i64, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_dtype": ([_vp, ctypes.POINTER(ctypes.c_int)], _i32),
    "pmm_corpus_destroy": ([_vp], _i32),
    "pmm_corpus_info": (
        [_vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)],
        _i32,
    ),
    "pmm_corpus_shards": ([_vp, ctypes.POINTER(ctypes.c_int)], _i32),
    "pmm_corpus_bytes": ([_vp, ctypes.POINTER(_sz)], _i32),
    "pmm_corpus_subset_ids": ([_vp, _vp, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_subset_mask": ([_vp, _vp, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_index_map": ([_vp, _vp, _i64, ctypes.POINTER(ctypes.c_int64)], _i32),
    "pmm_partition_plan": ([_vp, _i64, _i64, _vp, _vp, ctypes.POINTER(ctypes.c_int64)], _i32),
    "pmm_corpus_partition": ([_vp, _vp, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_groups": ([_vp, ctypes.POINTER(ctypes.c_int64), _vp, _i64], _i32),
    "pmm_topk_f32_grouped": ([_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_topk_f64_grouped": ([_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_probe_plan": ([_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int64)],
                       _i32),
    "pmm_topk_f32_probed": ([_vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_topk_f32_corpus": ([_vp, _vp, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_topk_f64_corpus": ([_vp, _vp, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_topk_bf16_corpus": ([_vp, _vp, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_range_f32_corpus": ([_vp, _vp, _i64, ctypes.c_float, _i32, _i64, _vp, _vp, _vp,
                              ctypes.POINTER(ctypes.c_int64)], _i32),
    "pmm_topk_f32_candidates": ([_vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_corpus_create_f32_docs": ([_vp, _i64, _i64, _vp, _i64, _vp], _i32),
    "pmm_corpus_docs": ([_vp, _vp, _vp, _i64], _i32),
    "pmm_topk_f32_maxsim": ([_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp], _i32),
    "pmm_kmeans_f32_corpus": ([_vp, _i64, _vp, _i32, _i64, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int64),
                               ctypes.POINTER(ctypes.c_int)], _i32),
    "pmm_range_f32_self": ([_vp, ctypes.c_float, _i32, _i64, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int64)], _i32),
    "pmm_topk_f32_self": ([_vp, _i64, _i32, _vp, _vp], _i32),
    "pmm_components_f32_self": ([_vp, ctypes.c_float, _i32, _vp, ctypes.POINTER(ctypes.c_int64),
                                 ctypes.POINTER(ctypes.c_int64)], _i32),
    "pmm_range_self_plan": ([_i64, _i32, _i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64),
                             ctypes.POINTER(ctypes.c_int64)], _i32),
    "pmm_sort_plan": ([_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
    "pmm_topk_i8": ([_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_topk_i8_corpus": ([_vp, _vp, _i64, _i64, _i32, _vp, _vp], _i32),
    "pmm_topk_i8_device": ([_vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _u32, _vp, _vp, _vp, _sz, _vp], _i32),
    "pmm_topk_i8_workspace_bytes": ([_i64, _i64, _i64, _i64, _i32], _sz),
    "pmm_corpus_create_i8": ([_vp, _i64, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_pack_sign_device": ([_vp, _i64, _i64, _i64, _vp, _i64, _vp], _i32),
    "pmm_corpus_create_bits": ([_vp, _i64, _i64, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_sign_bits": ([_vp, ctypes.POINTER(ctypes.c_void_p)], _i32),
    "pmm_corpus_bits_rows": ([_vp, _vp], _i32),
    "pmm_topk_bits": ([_vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp], _i32),
    "pmm_topk_bits_corpus": ([_vp, _vp, _i64, _i64, _vp, _vp], _i32),
    "pmm_topk_bits_workspace_bytes": ([_i64, _i64, _i64, _i64], _sz),
    "pmm_topk_bits_device": ([_vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _u32, _vp, _vp, _vp, _sz, _vp], _i32),
    "pmm_timing_enable": ([_i32], _i32),
    "pmm_timing_reset": ([], _i32),
    "pmm_timing_read": (
        [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)],
        _i32,
    ),
}
for _name, (_args, _res) in _SIGS.items():
    _fn = getattr(_lib, _name)
    _fn.argtypes = _args
    _fn.restype = _res


def lib() -> ctypes.CDLL:
    return _lib


class PmmError(RuntimeError):
    """A failing libpmm call; ``code`` is the PMM_ERR_* value."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


def last_error() -> str:
    return (_lib.pmm_last_error() or b"").decode(errors="replace")


def check(rc: int) -> None:
    if rc != PMM_OK:
        raise PmmError(rc, last_error())


def ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


def version() -> str:
    return _lib.pmm_version().decode()


def device_count() -> int:
    n = ctypes.c_int(0)
    check(_lib.pmm_device_count(ctypes.byref(n)))
    return n.value


def device_memory():
    """(free, total) bytes of HBM on the device host calls run on."""
    f, t = _sz(0), _sz(0)
    check(_lib.pmm_device_memory(ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def set_devices(ids) -> None:
    """Row-shard the corpus of later host top-k calls (and corpus handles
    created afterwards) over these HIP devices, results merged on ids[0]
    (pmm_set_devices).  An empty list returns to one device."""
    ids = [int(i) for i in ids]
    arr = (ctypes.c_int * max(1, len(ids)))(*ids)
    check(_lib.pmm_set_devices(arr, len(ids)))


def get_devices():
    """The current device list (pmm_get_devices); [] = one device."""
    n = ctypes.c_int(0)
    check(_lib.pmm_get_devices(None, 0, ctypes.byref(n)))
    arr = (ctypes.c_int * max(1, n.value))()
    check(_lib.pmm_get_devices(arr, n.value, ctypes.byref(n)))
    return list(arr[:n.value])


def range_self_plan(n: int, cus: int, variant: int = -1):
    """The triangular schedule of the self range search's emit pass
    (pmm_range_self_plan; pure, no GPU): (variant, block_tile_visits,
    block_tile_full) for n rows on a device of ``cus`` compute units."""
    v = ctypes.c_int(0)
    visits, full = ctypes.c_int64(0), ctypes.c_int64(0)
    check(_lib.pmm_range_self_plan(n, cus, variant, ctypes.byref(v), ctypes.byref(visits), ctypes.byref(full)))
    return int(v.value), int(visits.value), int(full.value)


SORT_PIECE = np.dtype([("self", "<u4"), ("first", "<u4"), ("T", "<u4"), ("kout", "<u4"), ("dst", "<i8")])


def sort_plan(offsets, smax: int, cap: int):
    """The sort plan of ragged key lists (pmm_sort_plan; pure, no GPU):
    (piece bounds, block-sort pieces, the longest of them, the cut segments'
    pieces as SORT_PIECE records, the merged total)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    m = offsets.size - 1
    room = m + int(offsets[-1]) // max(int(smax), 1) + 1  # no plan has more pieces
    po, mid, cut = np.empty(room + 1, np.int64), np.empty(room, np.int32), np.empty(room, SORT_PIECE)
    n = np.zeros(5, np.int64)
    check(_lib.pmm_sort_plan(ptr(offsets), m, int(smax), int(cap), ptr(po), ptr(mid), ptr(cut), ptr(n)))
    return po[:n[0] + 1], mid[:n[1]], int(n[2]), cut[:n[3]], int(n[4])


def shard_plan(devs, m: int, n: int, d: int, k: int, metric: int, compute: int = COMPUTE_F32,
               host_rows: bool = True):
    """The sharded search's memory plan (pmm_shard_plan; pure, no GPU):
    (plan_of[g], [(device, bytes) per distinct-device plan], list_offsets[g])."""
    G = len(devs)
    arr = (ctypes.c_int * G)(*[int(x) for x in devs])
    plan_of = (ctypes.c_int * G)()
    plan_dev = (ctypes.c_int * G)()
    plan_bytes = (ctypes.c_uint64 * G)()
    offs = (ctypes.c_uint64 * G)()
    npl = ctypes.c_int(0)
    check(_lib.pmm_shard_plan(arr, G, m, n, d, k, metric, compute, 1 if host_rows else 0, plan_of, plan_dev,
                              plan_bytes, offs, ctypes.byref(npl)))
    return (list(plan_of), [(plan_dev[j], int(plan_bytes[j])) for j in range(npl.value)], [int(x) for x in offs])


def metric_from_str(s: str) -> int:
    out = ctypes.c_int(-1)
    check(_lib.pmm_metric_from_str(s.encode(), ctypes.byref(out)))
    return out.value


def topk_host(q: np.ndarray, c: np.ndarray, k: int, metric: int, compute: int = COMPUTE_F32):
    """Host-buffer top-k.  q: (m, d), c: (n, d) C-contiguous, both f32 or both f64;
    0 <= k <= n.  Returns (idx uint32 (m, k), scores (m, k) in the input dtype)."""
    m, d = q.shape
    n = c.shape[0]
    idx = np.empty((m, k), dtype=np.uint32)
    sc = np.empty((m, k), dtype=q.dtype)
    if q.dtype == np.float32:
        rc = _lib.pmm_topk_f32_ex(ptr(q), m, ptr(c), n, d, k, metric, compute, ptr(idx), ptr(sc))
    else:
        rc = _lib.pmm_topk_f64(ptr(q), m, ptr(c), n, d, k, metric, ptr(idx), ptr(sc))
    check(rc)
    return idx, sc


def topk_i8_host(q: np.ndarray, c: np.ndarray, k: int, metric: int):
    """Host-buffer top-k of int8 rows (pmm_topk_i8).  q: (m, d), c: (n, d) int8;
    0 <= k <= n.  Returns (idx uint32 (m, k), scores float64 (m, k)): the bits
    ``topk_host`` returns for the same values as float64."""
    q = np.ascontiguousarray(q, dtype=np.int8)
    c = np.ascontiguousarray(c, dtype=np.int8)
    m, d = q.shape
    n = c.shape[0]
    idx = np.empty((m, k), dtype=np.uint32)
    sc = np.empty((m, k), dtype=np.float64)
    check(_lib.pmm_topk_i8(ptr(q), m, ptr(c), n, d, k, metric, ptr(idx), ptr(sc)))
    return idx, sc


def topk_i8_device(q_ptr: int, ldq: int, m: int, c_ptr: int, ldc: int, n: int, d: int, k: int, metric: int,
                   out_idx_ptr: int, out_score_ptr: int, *, index_base: int = 0, workspace: int = 0,
                   workspace_bytes: int = 0, stream: int = 0) -> None:
    """pmm_topk_i8_device over device pointers (row strides in bytes)."""
    check(_lib.pmm_topk_i8_device(q_ptr, ldq, m, c_ptr, ldc, n, d, k, metric, index_base, out_idx_ptr,
                                  out_score_ptr, workspace or None, workspace_bytes, stream or None))


def i8_workspace_bytes(m: int, n: int, d: int, k: int, metric: int) -> int:
    return int(_lib.pmm_topk_i8_workspace_bytes(m, n, d, k, metric))


def _bit_rows(a, what: str, w=None) -> np.ndarray:
    """``a`` as the bit-row entries take it: a C-contiguous 2-D uint8 array
    (of ``w`` bytes a row when given), else the TypeError they raise."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or (w is not None and a.shape[1] != w):
        width = "" if w is None else f" of {w} bytes a row"
        raise TypeError(f"{what} takes a 2-D uint8 array of packed bits{width} (pack_sign makes one), "
                        f"got {a.dtype} with shape {a.shape}")
    return np.ascontiguousarray(a)


def topk_bits_host(q: np.ndarray, c: np.ndarray, k: int):
    """Host-buffer Hamming top-k of packed bit rows (pmm_topk_bits).  q: (m, w),
    c: (n, w) uint8; 0 <= k <= n.  Returns (idx uint32 (m, k), scores float64
    (m, k)): the integer distances, least first, ties to the lower index."""
    q = _bit_rows(q, "topk_bits_host")
    c = _bit_rows(c, "topk_bits_host")
    if q.shape[1] != c.shape[1]:
        raise ValueError("dimension mismatch")
    m, w = q.shape
    n = c.shape[0]
    idx = np.empty((m, k), dtype=np.uint32)
    sc = np.empty((m, k), dtype=np.float64)
    check(_lib.pmm_topk_bits(ptr(q), m, ptr(c), n, w, k, ptr(idx), ptr(sc)))
    return idx, sc


def topk_bits_device(q_ptr: int, ldq: int, m: int, c_ptr: int, ldc: int, n: int, w: int, k: int,
                     out_idx_ptr: int, out_score_ptr: int, *, index_base: int = 0, workspace: int = 0,
                     workspace_bytes: int = 0, stream: int = 0) -> None:
    """pmm_topk_bits_device over device pointers (row strides in bytes)."""
    check(_lib.pmm_topk_bits_device(q_ptr, ldq, m, c_ptr, ldc, n, w, k, index_base, out_idx_ptr, out_score_ptr,
                                    workspace or None, workspace_bytes, stream or None))


def bits_workspace_bytes(m: int, n: int, w: int, k: int) -> int:
    return int(_lib.pmm_topk_bits_workspace_bytes(m, n, w, k))


def pack_sign_device(x_ptr: int, ldx: int, rows: int, d: int, out_ptr: int, ld_out: int, *, stream: int = 0) -> None:
    """pmm_pack_sign_device over device pointers: ldx in floats, ld_out in
    bytes (a multiple of 8, at least roundup(ceil(d / 8), 8))."""
    check(_lib.pmm_pack_sign_device(x_ptr, ldx, rows, d, out_ptr, ld_out, stream or None))


def bits_device_bytes(n: int, w: int) -> int:
    """HBM a bit corpus of n rows of w packed bytes holds
    (pmm_corpus_create_bits): the rows at stride roundup(w, 16) and a u32
    popcount per row."""
    return n * (-(-w // 16) * 16) + 4 * n


class _PinnedBlock:
    """One page-locked host block of the result pool; returns itself to the
    pool when the last array / Arrow buffer viewing it is released."""

    __slots__ = ("ptr", "nbytes", "pool", "__weakref__")

    def __init__(self, ptr_value: int, nbytes: int, pool: "PinnedPool"):
        self.ptr, self.nbytes, self.pool = ptr_value, nbytes, pool

    def __del__(self):  # pragma: no cover - exercised through the GC
        try:
            self.pool._give_back(self.ptr, self.nbytes)
        except Exception:
            pass


class PinnedPool:
    """Recycled page-locked result buffers (pmm_host_alloc).  A `.pmm.matmul`
    result (m x n values) lands in one of these: no page faults, D2H at link
    rate, and the buffer becomes the Arrow child buffer of the result Series
    without a copy.  Blocks come back when their arrays are freed; at most
    `cap_bytes` of idle blocks are kept (PMM_PINNED_POOL_BYTES, default 1 GiB;
    0 disables the pool).

    Re-entrancy: a block's finaliser can run inside any allocation (a cyclic
    GC pass), including one made by `take` on the same thread.  So returning a
    block takes no lock and allocates nothing: `_give_back` appends
    (ptr, nbytes) to a deque (append is atomic), and `take` moves returned
    blocks into the free lists under the lock, where nothing is allocated
    either (the lists are preallocated per size; Python objects for the result
    are built after the lock is released)."""

    MIN_BYTES = 1 << 20  # smaller results: a plain numpy array

    def __init__(self, cap_bytes: int):
        self.cap = cap_bytes
        self.free = {}  # nbytes -> [ptr, ...]
        self.idle = 0
        self.lock = threading.Lock()
        self.returned = collections.deque()  # (ptr, nbytes) from finalisers, lock-free

    def _absorb(self):
        """Move finalised blocks into the free lists (lock held by caller).
        Returns the pointers that exceed the cap, to be freed after the lock
        is released."""
        over = []
        while True:
            try:
                p, nbytes = self.returned.popleft()
            except IndexError:
                return over
            if self.idle + nbytes <= self.cap:
                self.free.setdefault(nbytes, []).append(p)
                self.idle += nbytes
            else:
                over.append(p)

    def take(self, nbytes: int):
        """A (pointer, owner) for nbytes, or None (pool off, too small, or the
        allocation failed)."""
        if self.cap <= 0 or nbytes < self.MIN_BYTES:
            return None
        p = None
        with self.lock:
            over = self._absorb()
            lst = self.free.get(nbytes)
            if lst:
                self.idle -= nbytes
                p = lst.pop()
        for q in over:
            _lib.pmm_host_free(q)
        if p is None:
            out = ctypes.c_void_p()
            if _lib.pmm_host_alloc(nbytes, ctypes.byref(out)) != PMM_OK or not out.value:
                return None
            p = out.value
        return p, _PinnedBlock(p, nbytes, self)

    def _give_back(self, p: int, nbytes: int) -> None:
        # runs from finalisers: never waits on the lock (the finaliser may run
        # inside `take` on the thread that holds it), allocates nothing beyond
        # the deque node before it tries the lock
        self.returned.append((p, nbytes))
        # opportunistic drain: blocks past the cap are freed as they come back,
        # not left page-locked until a later take(); when the lock
        # is busy, its holder or the next call drains them.  Not at interpreter
        # shutdown (module globals may be gone; the process exit frees them)
        if sys.is_finalizing() or _lib is None:
            return
        self.drain(blocking=False)

    def drain(self, blocking: bool = True) -> None:
        """Move returned blocks into the free lists and free those past the cap."""
        if not self.lock.acquire(blocking=blocking):
            return
        try:
            over = self._absorb()
        finally:
            self.lock.release()
        for q in over:
            _lib.pmm_host_free(q)

    def pending_bytes(self) -> int:
        """Bytes returned by finalisers and not yet absorbed (from the deque
        itself, so no unlocked counter can drift)."""
        return sum(n for _, n in list(self.returned))

    def idle_bytes(self) -> int:
        with self.lock:
            over = self._absorb()
            n = self.idle
        for q in over:
            _lib.pmm_host_free(q)
        return n

    def clear(self) -> None:
        with self.lock:
            over = self._absorb()
            ptrs = [p for lst in self.free.values() for p in lst] + over
            self.free.clear()
            self.idle = 0
        for p in ptrs:
            _lib.pmm_host_free(p)


pinned_pool = PinnedPool(int(os.environ.get("PMM_PINNED_POOL_BYTES", str(1 << 30))))
atexit.register(pinned_pool.clear)  # idle page-locked blocks go back to the OS at exit


def pinned_empty(shape, dtype) -> np.ndarray:
    """np.empty in a pooled page-locked block when one is available (the block
    is owned by the returned array's buffer chain), else np.empty."""
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    got = pinned_pool.take(nbytes)
    if got is None:
        return np.empty(shape, dtype=dtype)
    p, owner = got
    raw = (ctypes.c_char * nbytes).from_address(p)
    raw._pmm_block = owner  # the array's base holds the block until released
    return np.frombuffer(raw, dtype=dtype).reshape(shape)


def matmul_host(q: np.ndarray, c: np.ndarray) -> np.ndarray:
    m, d = q.shape
    n = c.shape[0]
    out = pinned_empty((m, n), q.dtype)
    fn = _lib.pmm_matmul_f32 if q.dtype == np.float32 else _lib.pmm_matmul_f64
    check(fn(ptr(q), m, ptr(c), n, d, ptr(out)))
    return out


def topk_device(q_ptr: int, ldq: int, m: int, c_ptr: int, ldc: int, n: int, d: int, k: int,
                metric: int, out_idx_ptr: int, out_score_ptr: int, *, index_base: int = 0,
                compute: int = COMPUTE_F32, workspace: int = 0, workspace_bytes: int = 0,
                stream: int = 0) -> None:
    """Device-resident fused top-k (pointers are HBM addresses, e.g. torch data_ptr())."""
    check(_lib.pmm_topk_f32_device(q_ptr, ldq, m, c_ptr, ldc, n, d, k, metric, compute,
                                   index_base, out_idx_ptr, out_score_ptr, workspace or None,
                                   workspace_bytes, stream or None))


def topk_f64_device(q_ptr: int, ldq: int, m: int, c_ptr: int, ldc: int, n: int, d: int, k: int,
                    metric: int, out_idx_ptr: int, out_score_ptr: int, *, index_base: int = 0,
                    stream: int = 0) -> None:
    """Device-resident f64 top-k (pmm_topk_f64_device; row strides >= roundup(d, 16))."""
    check(_lib.pmm_topk_f64_device(q_ptr, ldq, m, c_ptr, ldc, n, d, k, metric, index_base, out_idx_ptr,
                                   out_score_ptr, stream or None))


def topk_bf16_device(q_ptr: int, ldq: int, m: int, c_ptr: int, ldc: int, n: int, d: int, k: int,
                     metric: int, out_idx_ptr: int, out_score_ptr: int, *, index_base: int = 0,
                     workspace: int = 0, workspace_bytes: int = 0, stream: int = 0) -> None:
    """Device-resident bf16 top-k (bf16 row bit patterns in HBM, e.g. a
    torch.bfloat16 tensor's data_ptr()); row strides >= roundup(d, 128)."""
    check(_lib.pmm_topk_bf16_device(q_ptr, ldq, m, c_ptr, ldc, n, d, k, metric, index_base,
                                    out_idx_ptr, out_score_ptr, workspace or None, workspace_bytes,
                                    stream or None))


def merge_device(idx_ptr: int, score_ptr: int, m: int, lists: int, k_in: int, k_out: int,
                 metric: int, out_idx_ptr: int, out_score_ptr: int, stream: int = 0) -> None:
    check(_lib.pmm_merge_topk_device(idx_ptr, score_ptr, m, lists, k_in, k_out, metric,
                                     out_idx_ptr, out_score_ptr, stream or None))


def merge_strided_device(idx_ptr: int, score_ptr: int, m: int, lists: int, k_in: int,
                         row_stride: int, list_stride: int, k_out: int, metric: int,
                         out_idx_ptr: int, out_score_ptr: int, stream: int = 0, *,
                         sorted_lists: bool = False) -> None:
    """k-way merge of strided lists; sorted_lists=True: every list is
    best-first (a top-k or merge output), so the prefix fast path applies
    (pmm_merge_sorted_topk_strided_device)."""
    fn = _lib.pmm_merge_sorted_topk_strided_device if sorted_lists else _lib.pmm_merge_topk_strided_device
    check(fn(idx_ptr, score_ptr, m, lists, k_in, row_stride, list_stride, k_out, metric, out_idx_ptr,
             out_score_ptr, stream or None))


def norms_device(a_ptr: int, ld: int, rows: int, d: int, squared: bool, out_ptr: int, *,
                 f64: bool = False, stream: int = 0) -> None:
    """Row norms (or squared norms) of device rows in the reference's order
    (pmm_norms_f32_device / pmm_norms_f64_device)."""
    fn = _lib.pmm_norms_f64_device if f64 else _lib.pmm_norms_f32_device
    check(fn(a_ptr, ld, rows, d, 1 if squared else 0, out_ptr, stream or None))


def round_bf16_device(a_ptr: int, ld: int, rows: int, d: int, out_ptr: int, ldo: int, *, norm: int = 0,
                      inv_norm: int = 0, sq: int = 0, sq_factor: int = 0, stream: int = 0) -> None:
    """f32 device rows -> zero-padded bf16 rows of stride ``ldo`` (a multiple of
    8, >= d; roundup(d, 128) for ``topk_bf16_device``) and, in the same pass,
    any of the four per-row f32 arrays of the rounded rows: norm, the cosine
    factor 1 / norm (0 at or below 1e-6), squared norm, the euclidean factor
    (pmm_round_bf16_device).  0 skips an array."""
    check(_lib.pmm_round_bf16_device(a_ptr, ld, rows, d, out_ptr, ldo, norm or None, inv_norm or None,
                                     sq or None, sq_factor or None, stream or None))


def screen_prepare_device(a_ptr: int, ld: int, rows: int, d: int, out_ptr: int, ldo: int, *, norm: int = 0,
                          inv_norm: int = 0, rel: int = 0, unsafe: int = 0, scalars: int = 0,
                          stream: int = 0) -> None:
    """f32 device rows -> what the screened f32 cosine top-k needs of them, in
    one pass (pmm_screen_prepare_device): the zero-padded bf16 rows of stride
    ``ldo`` and any of the per-row arrays -- norm and 1 / norm of the unrounded
    row (``norms_device``'s bits), the rounding residual bound ``rel``, the
    ``unsafe`` flag (uint32) -- and, with ``scalars`` (two zeroed uint32
    words), the maximum ``rel`` over the safe rows and the OR of the flags.
    0 skips an array."""
    check(_lib.pmm_screen_prepare_device(a_ptr, ld, rows, d, out_ptr, ldo, norm or None, inv_norm or None,
                                         rel or None, unsafe or None, scalars or None, stream or None))


def workspace_bytes(m: int, n: int, d: int, k: int, metric: int, compute: int = COMPUTE_F32) -> int:
    return int(_lib.pmm_topk_workspace_bytes(m, n, d, k, metric, compute))


def merge_bytes(workspace_ptr: int, m: int, n: int, d: int, k: int, metric: int,
                compute: int = COMPUTE_F32) -> int:
    """Algorithmic bytes of the last fused top-k's merge pass (measurement only)."""
    out = ctypes.c_uint64(0)
    check(_lib.pmm_topk_merge_bytes(workspace_ptr, m, n, d, k, metric, compute, ctypes.byref(out)))
    return int(out.value)


def timing_enable(on: bool = True) -> None:
    check(_lib.pmm_timing_enable(1 if on else 0))


def timing_reset() -> None:
    check(_lib.pmm_timing_reset())


def timing_read(kernel: str):
    ms = ctypes.c_double(0.0)
    n = ctypes.c_int64(0)
    check(_lib.pmm_timing_read(kernel.encode(), ctypes.byref(ms), ctypes.byref(n)))
    return ms.value, n.value


DTYPE_F32 = 0
DTYPE_F64 = 1
DTYPE_BF16 = 2
DTYPE_I8 = 3
DTYPE_BITS = 4

_COMPUTE_MODES = ("f32", "bf16")


def check_compute(compute: str) -> str:
    """``compute`` if it names a compute mode, else the ValueError every
    ``compute=`` keyword of the package raises (the numpy-level ``topk``'s)."""
    if compute not in _COMPUTE_MODES:
        raise ValueError(f"compute must be 'f32' or 'bf16', not {compute!r}")
    return compute


def corpus_device_bytes(n: int, d: int, dtype=np.float32, compute: str = "f32", screen: bool = False) -> int:
    """HBM a DeviceCorpus of n x d rows holds.  f32 (pmm_corpus_create_f32):
    the rows padded to a multiple of 32 floats plus four norm arrays (cosine
    norms and pre-filter factors, euclidean squared norms and factors).  f64
    (pmm_corpus_create_f64): the rows padded to a multiple of 16 doubles plus
    two norm arrays (cosine norms, euclidean squared norms).  compute="bf16"
    (pmm_corpus_create_bf16, whatever ``dtype``): the rows rounded to bf16 and
    padded to a multiple of 128 plus the four f32 norm arrays.
    ``screen=True``: with the screen image an f32 handle builds on its first
    screened cosine call -- the rows rounded to bf16 at stride roundup(d, 128)
    plus a residual and a flag per row.  Only f32 handles have one: an f64 or
    ``compute="bf16"`` handle's figure is the same with and without it."""
    if check_compute(compute) == "bf16":
        return n * (-(-d // 128) * 128) * 2 + n * 4 * 4
    if np.dtype(dtype) == np.int8:  # pmm_corpus_create_i8: the bytes padded to 64, a u32 and an f32 per row
        return n * (-(-d // 64) * 64) + n * 2 * 4
    if np.dtype(dtype) == np.float64:
        dp = -(-d // 16) * 16
        return n * dp * 8 + n * 2 * 8
    dp = -(-d // 32) * 32
    return n * dp * 4 + n * 4 * 4 + (n * (-(-d // 128) * 128) * 2 + 8 * n if screen else 0)


def subset_device_bytes(s: int, d: int, dtype=np.float32, compute: str = "f32", screen: bool = False) -> int:
    """HBM a derived handle of s rows holds (``DeviceCorpus.subset``): a
    handle of s x d rows of the parent's kind -- ``corpus_device_bytes`` -- plus
    its uint32 index map."""
    return corpus_device_bytes(s, d, dtype, compute, screen) + 4 * s


def partitioned_device_bytes(s: int, d: int, G: int, dtype=np.float32, compute: str = "f32") -> int:
    """HBM a partitioned handle of s kept rows in G groups holds
    (``DeviceCorpus.partition``): ``subset_device_bytes`` without a screen
    image (a partitioned handle never has one) plus its G + 1 int64 offsets."""
    return subset_device_bytes(s, d, dtype, compute) + 8 * (G + 1)


NO_GROUP = 0xFFFFFFFF  # the label of a row that is in no group (PMM_NO_GROUP)


def partition_plan(labels, G: int):
    """(perm uint32 [kept], offsets int64 [G + 1]) of pmm_partition_plan: the
    rows whose label is in [0, G) group by group, ascending inside a group;
    rows labelled ``NO_GROUP`` are dropped.  Host only: runs without a GPU."""
    labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    perm = np.empty(labels.size, dtype=np.uint32)
    offsets = np.empty(int(G) + 1, dtype=np.int64)
    kept = ctypes.c_int64(0)
    check(_lib.pmm_partition_plan(ptr(labels), labels.size, int(G), ptr(perm), ptr(offsets), ctypes.byref(kept)))
    return perm[:kept.value], offsets


def _probe_lists(probe_offsets, probe_labels, m: int):
    """(offsets int64 (m + 1,), labels uint32) as the probed entries take them."""
    po = np.ascontiguousarray(probe_offsets, dtype=np.int64).reshape(-1)
    pl = np.ascontiguousarray(probe_labels, dtype=np.uint32).reshape(-1)
    if po.size != m + 1:
        raise ValueError(f"probe_offsets has {po.size} entries for {m} query rows: one more than rows is needed")
    if po[0] != 0 or np.any(np.diff(po) < 0) or po[-1] != pl.size:
        raise ValueError(f"probe_offsets must rise from 0 to len(probe_labels) = {pl.size}")
    return po, pl


def probe_plan(probe_offsets, probe_labels, group_offsets, k: int):
    """(slot_row uint32 [S], slot_label uint32 [S], row_offsets int64 [m + 1],
    row_slots uint32 [S], out_len uint32 [m]) of pmm_probe_plan: the distinct
    (query row, label) slots with a non-empty segment, stably sorted by label;
    every row's slot numbers; every row's list length.  Host only: runs
    without a GPU."""
    po = np.ascontiguousarray(probe_offsets, dtype=np.int64).reshape(-1)
    po, pl = _probe_lists(po, probe_labels, po.size - 1)
    goff = np.ascontiguousarray(group_offsets, dtype=np.int64).reshape(-1)
    m, cap = po.size - 1, int(po[-1])
    slot_row, slot_label = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
    row_slots, row_offsets = np.empty(cap, dtype=np.uint32), np.empty(m + 1, dtype=np.int64)
    out_len = np.empty(m, dtype=np.uint32)
    slots = ctypes.c_int64(0)
    check(_lib.pmm_probe_plan(ptr(po), ptr(pl), m, ptr(goff), goff.size - 1, int(k), ptr(slot_row), ptr(slot_label),
                              ptr(row_offsets), ptr(row_slots), ptr(out_len), ctypes.byref(slots)))
    S = slots.value
    return slot_row[:S], slot_label[:S], row_offsets, row_slots[:S], out_len


def ascending_ids(ids, n: int) -> np.ndarray:
    """Row ids as the subset entries take them: uint32, ascending, unique.
    An id outside [0, n) raises ValueError."""
    ids = np.asarray(ids)
    if ids.dtype.kind not in "iu":
        raise TypeError(f"row ids must be integers, not {ids.dtype}")
    ids = np.unique(ids.reshape(-1))  # sorted, duplicates dropped
    if ids.size and (int(ids[0]) < 0 or int(ids[-1]) >= n):
        bad = int(ids[0]) if int(ids[0]) < 0 else int(ids[-1])
        raise ValueError(f"subset row id {bad} is out of range for a corpus of {n} rows")
    return np.ascontiguousarray(ids, dtype=np.uint32)


class DeviceCorpus:
    """A corpus uploaded once to HBM with its norms (pmm_corpus_*), f32 or f64
    rows by the dtype of ``c`` (the reference's two branches,
    src/matmul.rs:427-468).  ``compute="bf16"``: ``c`` is taken as f32 and kept
    rounded to bf16 with the norms of the rounded rows (pmm_corpus_create_bf16,
    half the HBM of an f32 handle); ``topk`` then takes f32 queries and returns
    f32 scores, those of ``topk_host(..., compute=COMPUTE_BF16)``.

    Reference-counted: ``acquire()`` / ``release()`` bracket a use (``topk``
    does so itself); ``close()`` frees the device memory at once if no use is
    in flight, else when the last one releases it -- a cache may evict a
    handle while another thread is still searching it."""

    is_bits = False  # a bit corpus (``bits`` / ``sign_bits``): ``d`` is the bytes of a row, ``topk`` takes no metric
    _mapped = False  # a derived handle: it holds a uint32 index map beside its rows
    n_docs = 0       # a multi-vector handle (``multivector``): its documents; ``n`` stays the token rows

    def __init__(self, c: np.ndarray, compute: str = "f32"):
        self.compute = check_compute(compute)
        bf16 = compute == "bf16"
        self.dtype = np.dtype(np.float64 if np.asarray(c).dtype == np.float64 and not bf16 else np.float32)
        c = np.ascontiguousarray(c, dtype=self.dtype)
        h = ctypes.c_void_p()
        create = (_lib.pmm_corpus_create_bf16 if bf16 else
                  _lib.pmm_corpus_create_f64 if self.dtype == np.float64 else _lib.pmm_corpus_create_f32)
        check(create(ptr(c), c.shape[0], c.shape[1], ctypes.byref(h)))
        self._h = h
        self._lock = threading.Lock()
        self._refs = 0
        self._closing = False
        self.n, self.d = c.shape
        self._nbytes0 = corpus_device_bytes(self.n, self.d, self.dtype, compute)  # device footprint, not host bytes

    @classmethod
    def int8(cls, c: np.ndarray) -> "DeviceCorpus":
        """An int8 corpus (pmm_corpus_create_i8): the signed bytes as they are
        with each row's integer sum of squares.  ``topk`` then takes int8
        queries and returns float64 scores -- the bits an f64 handle of the
        same values returns -- from the int8 MFMA.  (``DeviceCorpus(c)`` of an
        int8 array converts to f32, as before.)"""
        c = np.asarray(c)
        if c.dtype != np.int8 or c.ndim != 2:
            raise TypeError(f"DeviceCorpus.int8 takes a 2-D int8 array, got {c.dtype} with shape {c.shape}")
        c = np.ascontiguousarray(c)
        h = ctypes.c_void_p()
        check(_lib.pmm_corpus_create_i8(ptr(c), c.shape[0], c.shape[1], ctypes.byref(h)))
        return cls._adopt(h, np.int8, c.shape[0], c.shape[1], corpus_device_bytes(c.shape[0], c.shape[1], np.int8))

    @classmethod
    def multivector(cls, tokens: np.ndarray, doc_offsets) -> "DeviceCorpus":
        """A multi-vector corpus (pmm_corpus_create_f32_docs): the f32 handle
        of the token rows -- every other method sees exactly that handle --
        which also keeps the documents' bounds: document c is token rows
        ``doc_offsets[c]:doc_offsets[c + 1]`` (from 0 to the token count,
        strictly ascending: no empty document).  ``topk_maxsim`` searches it."""
        tokens = np.asarray(tokens)
        if tokens.dtype != np.float32 or tokens.ndim != 2:
            raise TypeError(f"DeviceCorpus.multivector takes a 2-D float32 array, got {tokens.dtype} with shape "
                            f"{tokens.shape}")
        tokens = np.ascontiguousarray(tokens)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.int64).reshape(-1)
        if doc_offsets.size < 2:
            raise ValueError("a multi-vector corpus needs at least one document (two offsets)")
        h = ctypes.c_void_p()
        check(_lib.pmm_corpus_create_f32_docs(ptr(tokens), tokens.shape[0], tokens.shape[1], ptr(doc_offsets),
                                              doc_offsets.size - 1, ctypes.byref(h)))
        self = cls._adopt(h, np.float32, tokens.shape[0], tokens.shape[1],
                          corpus_device_bytes(tokens.shape[0], tokens.shape[1], np.float32) + 8 * doc_offsets.size)
        self.n_docs = int(doc_offsets.size - 1)
        return self

    def doc_offsets(self) -> np.ndarray:
        """The documents' bounds (pmm_corpus_docs): n_docs + 1 int64, or the
        single offset [0] of a handle without documents."""
        n = ctypes.c_int64(0)
        self.acquire()
        try:
            check(_lib.pmm_corpus_docs(self._h, ctypes.byref(n), None, 0))
            out = np.zeros(int(n.value) + 1, dtype=np.int64)
            if n.value:
                check(_lib.pmm_corpus_docs(self._h, ctypes.byref(n), ptr(out), out.size))
        finally:
            self.release()
        return out

    def topk_maxsim(self, q_tokens: np.ndarray, q_offsets, cand_offsets, cand_docs, k: int, metric: int):
        """(idx uint32 (m, k), scores float32 (m, k), lens uint32 (m,)) of
        pmm_topk_f32_maxsim: query row i holds the tokens
        ``q_tokens[q_offsets[i]:q_offsets[i + 1]]`` and is searched among the
        documents ``cand_docs[cand_offsets[i]:cand_offsets[i + 1]]`` (strictly
        ascending document numbers of this multi-vector handle) by the MaxSim
        score -- the sum over its tokens of the best pair score in the
        document; its first ``lens[i]`` slots are the exact top-k there, the
        rest hold index 0xFFFFFFFF and score 0.  Cosine or dot."""
        q_tokens = np.ascontiguousarray(q_tokens, dtype=np.float32)
        if q_tokens.ndim != 2 or q_tokens.shape[1] != self.d:
            raise ValueError("dimension mismatch")
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int64).reshape(-1)
        if q_offsets.size < 1:
            raise ValueError("q_offsets needs m + 1 entries")
        m = q_offsets.size - 1
        if q_tokens.shape[0] < int(q_offsets[-1]):
            raise ValueError(f"q_offsets end at {int(q_offsets[-1])}, the tokens hold {q_tokens.shape[0]} rows")
        cand_offsets = np.ascontiguousarray(cand_offsets, dtype=np.int64)
        if cand_offsets.shape != (m + 1,):
            raise ValueError(f"one list per query row: {m} rows need {m + 1} offsets, got shape {cand_offsets.shape}")
        cand_docs = np.ascontiguousarray(cand_docs, dtype=np.uint32).reshape(-1)
        if cand_docs.size < int(cand_offsets[-1]):
            raise ValueError(f"the offsets end at {int(cand_offsets[-1])}, the ids hold {cand_docs.size}")
        k = int(k)
        idx = np.empty((m, max(k, 0)), dtype=np.uint32)
        sc = np.empty((m, max(k, 0)), dtype=np.float32)
        lens = np.empty(m, dtype=np.uint32)
        self.acquire()
        try:
            check(_lib.pmm_topk_f32_maxsim(self._h, ptr(q_tokens) if q_tokens.size else None, ptr(q_offsets), m,
                                           ptr(cand_offsets), ptr(cand_docs) if cand_docs.size else None, k, metric,
                                           ptr(idx), ptr(sc), ptr(lens)))
        finally:
            self.release()
        return idx, sc, lens

    @classmethod
    def _adopt(cls, h, dtype, n: int, d: int, nbytes0: int) -> "DeviceCorpus":
        """The DeviceCorpus of a native handle made outside ``__init__`` (n
        rows of d elements of ``dtype``, compute "f32")."""
        self = cls.__new__(cls)
        self.compute = "f32"
        self.dtype = np.dtype(dtype)
        self._h = h
        self._lock = threading.Lock()
        self._refs = 0
        self._closing = False
        self.n, self.d = n, d
        self._nbytes0 = nbytes0
        return self

    @classmethod
    def bits(cls, c: np.ndarray) -> "DeviceCorpus":
        """A bit corpus (pmm_corpus_create_bits): rows of packed bits, ``d``
        the bytes of a row.  ``topk(packed_queries, k)`` is then the exact
        Hamming top-k: float64 distances, least first, ties to the lower
        index."""
        c = _bit_rows(c, "DeviceCorpus.bits")
        h = ctypes.c_void_p()
        check(_lib.pmm_corpus_create_bits(ptr(c), c.shape[0], c.shape[1], ctypes.byref(h)))
        self = cls._adopt(h, np.uint8, c.shape[0], c.shape[1], bits_device_bytes(*c.shape))
        self.is_bits = True
        return self

    def sign_bits(self) -> "DeviceCorpus":
        """The bit corpus of this f32 handle's rows (pmm_corpus_sign_bits):
        their signs packed on the device from the resident rows, no upload --
        the handle ``DeviceCorpus.bits(pack_sign(c))`` makes.  On a
        ``subset(sel)`` handle the lists keep the parent's row numbers."""
        h = ctypes.c_void_p()
        self.acquire()
        try:
            check(_lib.pmm_corpus_sign_bits(self._h, ctypes.byref(h)))
        finally:
            self.release()
        w = -(-self.d // 8)  # (the same rows: n is this handle's; a derived parent's map is copied)
        dc = DeviceCorpus._adopt(h, np.uint8, self.n, w, bits_device_bytes(self.n, w) + (4 * self.n if self._mapped else 0))
        dc.is_bits, dc._mapped = True, self._mapped
        return dc

    def bit_rows(self) -> np.ndarray:
        """A bit corpus' rows on the host (pmm_corpus_bits_rows): (n, d) uint8."""
        out = np.empty((self.n, self.d), dtype=np.uint8)
        self.acquire()
        try:
            check(_lib.pmm_corpus_bits_rows(self._h, ptr(out)))
        finally:
            self.release()
        return out

    @property
    def nbytes(self) -> int:
        """HBM the handle holds now (pmm_corpus_bytes): the creation-time
        footprint until an f32 handle has built its screen image.  The
        creation-time figure when the handle is closed or the loaded library
        has no such entry."""
        fn = getattr(_lib, "pmm_corpus_bytes", None)
        with self._lock:
            if fn is None or not self._h:
                return self._nbytes0
            out = _sz(0)
            if fn(self._h, ctypes.byref(out)) != PMM_OK:
                return self._nbytes0
            return int(out.value)

    def acquire(self) -> "DeviceCorpus":
        with self._lock:
            if self._closing or not self._h:
                raise RuntimeError("DeviceCorpus is closed")
            self._refs += 1
        return self

    def release(self) -> None:
        with self._lock:
            self._refs -= 1
            if self._refs == 0 and self._closing:
                self._destroy()

    def topk(self, q: np.ndarray, k: int, metric=None):
        """(idx uint32 (m, k), scores (m, k) in the corpus dtype); q is
        converted to the corpus dtype."""
        if self.is_bits:  # (one score, the Hamming distance: no metric)
            return self._topk_bits(q, k)
        if metric is None:
            raise TypeError("topk() needs a metric (only a bit corpus has none)")
        if self.dtype == np.int8 and np.asarray(q).dtype != np.int8:
            raise TypeError(f"an int8 corpus takes int8 queries, not {np.asarray(q).dtype}")
        q = np.ascontiguousarray(q, dtype=self.dtype)
        if q.shape[1] != self.d:
            raise ValueError("dimension mismatch")
        m = q.shape[0]
        idx = np.empty((m, k), dtype=np.uint32)
        i8 = self.dtype == np.int8
        sc = np.empty((m, k), dtype=np.float64 if i8 else self.dtype)
        fn = (_lib.pmm_topk_i8_corpus if i8 else
              _lib.pmm_topk_bf16_corpus if self.compute == "bf16" else
              _lib.pmm_topk_f64_corpus if self.dtype == np.float64 else _lib.pmm_topk_f32_corpus)
        self.acquire()
        try:
            check(fn(self._h, ptr(q), m, k, metric, ptr(idx), ptr(sc)))
        finally:
            self.release()
        return idx, sc

    def _topk_bits(self, q, k: int):
        q = _bit_rows(q, "a bit corpus", self.d)
        m = q.shape[0]
        idx = np.empty((m, k), dtype=np.uint32)
        sc = np.empty((m, k), dtype=np.float64)
        self.acquire()
        try:
            check(_lib.pmm_topk_bits_corpus(self._h, ptr(q), m, k, ptr(idx), ptr(sc)))
        finally:
            self.release()
        return idx, sc

    # The first call's capacity when ``range`` is given none: 64 hits per query
    # row and at least 65536 entries.  A guess, not a measurement: a near-
    # duplicate or "above 0.9 cosine" search returns a handful of rows per
    # query; a call that finds more pays one more pass with the exact total.
    RANGE_CAP_PER_ROW = 64
    RANGE_CAP_MIN = 1 << 16

    def range(self, q: np.ndarray, threshold: float, metric: int, cap=None):
        """(offsets int64 (m + 1,), idx uint32 (total,), scores float32
        (total,)) of pmm_range_f32_corpus: row i's hits -- every corpus row
        whose score is >= ``threshold`` (cosine, dot) or <= ``threshold``
        (euclidean) -- are entries [offsets[i], offsets[i + 1]), best first.
        An f32 handle of one shard, plain or derived (a derived handle returns
        its parent's row numbers).  ``cap``: the entries the first call has
        room for (default: ``RANGE_CAP_PER_ROW`` per query row, at least
        ``RANGE_CAP_MIN``); when the hits outnumber it the call is repeated
        once with the exact total, so the result does not depend on it."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError("dimension mismatch")
        m = q.shape[0]
        return self._range(m, m * self.n, cap, lambda *out: _lib.pmm_range_f32_corpus(
            self._h, ptr(q), m, float(threshold), metric, *out))

    def _range(self, rows: int, most: int, cap, call):
        """The range entries' cap protocol: ``call(cap, offsets, idx, scores,
        total)`` with room for ``cap`` entries (default: the class constants;
        at most ``most``), once more with the exact total when too small."""
        if cap is None:
            cap = max(self.RANGE_CAP_MIN, self.RANGE_CAP_PER_ROW * rows)
        cap = max(0, min(int(cap), most))
        offsets = np.empty(rows + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        self.acquire()
        try:
            while True:
                idx = np.empty(cap, dtype=np.uint32)
                sc = np.empty(cap, dtype=np.float32)
                check(call(cap, ptr(offsets), ptr(idx) if cap else None, ptr(sc) if cap else None,
                           ctypes.byref(total)))
                if total.value <= cap:
                    break
                cap = total.value  # too small: once more, with room
        finally:
            self.release()
        return offsets, idx[:total.value], sc[:total.value]

    def range_self(self, threshold: float, metric: int, cap=None):
        """(offsets int64 (n + 1,), idx uint32 (total,), scores float32
        (total,)) of pmm_range_f32_self: the handle searched against itself,
        each pair once.  Row i's entries are ``range(rows, ...)``'s for query
        row i without those at positions j <= i (a derived handle returns its
        parent's row numbers; positions are the handle's), same score bits,
        best first.  No rows are uploaded.  The dropped (j, i) has the bits of
        the kept (i, j) for every metric.  ``cap`` as for ``range``: default
        ``RANGE_CAP_PER_ROW`` per row, at least ``RANGE_CAP_MIN``, at most
        n (n - 1) / 2; repeated once with the exact total when too small."""
        n = self.n
        return self._range(n, n * (n - 1) // 2, cap, lambda *out: _lib.pmm_range_f32_self(
            self._h, float(threshold), metric, *out))

    def components_self(self, threshold: float, metric: int):
        """(labels uint32 (n,), components, pairs) of pmm_components_f32_self:
        the duplicate groups of the handle's rows -- the connected components
        of the pairs ``range_self(threshold, metric)`` lists.  ``labels[i]`` is
        the smallest position in row i's group (a derived handle returns its
        parent's row numbers), ``components`` the number of groups, ``pairs``
        the number of pairs (``range_self``'s total).  No pair is stored: the
        device memory of the call is a few words per row whatever the number of
        hits, and there is no cap and no second run."""
        labels = np.empty(self.n, dtype=np.uint32)
        components, pairs = ctypes.c_int64(0), ctypes.c_int64(0)
        self.acquire()
        try:
            check(_lib.pmm_components_f32_self(self._h, float(threshold), metric, ptr(labels),
                                               ctypes.byref(components), ctypes.byref(pairs)))
        finally:
            self.release()
        return labels, components.value, pairs.value

    def topk_self(self, k: int, metric: int):
        """(idx uint32 (n, k'), scores float32 (n, k')) of pmm_topk_f32_self:
        row i's k' = min(k, n - 1) best other rows of the handle -- its ranked
        list of all rows without itself, so an exact duplicate with a lower row
        number is kept and the row itself dropped.  No rows are uploaded."""
        n = self.n
        k = max(0, min(int(k), n - 1))
        idx = np.empty((n, k), dtype=np.uint32)
        sc = np.empty((n, k), dtype=np.float32)
        if k == 0:  # (a handle of one row: empty lists)
            return idx, sc
        self.acquire()
        try:
            check(_lib.pmm_topk_f32_self(self._h, k, metric, ptr(idx), ptr(sc)))
        finally:
            self.release()
        return idx, sc

    def kmeans(self, init: np.ndarray, metric: int, max_iter: int):
        """(centroids float32 (K, d), labels uint32 (n,), scores float32 (n,),
        updates, converged) of pmm_kmeans_f32_corpus: Lloyd's iteration on the
        handle's resident rows from the K initial centroids ``init``, at most
        ``max_iter`` updates.  The labels and scores are the exact f32 top-1
        of every row among the returned centroids (``NO_GROUP`` and NaN for a
        row whose best score is NaN); a derived handle's labels number its own
        rows.  Euclidean or cosine.  No rows are uploaded."""
        init = np.ascontiguousarray(init, dtype=np.float32)
        if init.ndim != 2 or init.shape[1] != self.d:
            raise ValueError("dimension mismatch")
        K, n = init.shape[0], self.n
        cent = np.empty((K, self.d), dtype=np.float32)
        labels = np.empty(n, dtype=np.uint32)
        sc = np.empty(n, dtype=np.float32)
        updates, conv = ctypes.c_int64(0), ctypes.c_int(0)
        self.acquire()
        try:
            check(_lib.pmm_kmeans_f32_corpus(self._h, K, ptr(init) if init.size else None, metric, int(max_iter),
                                             ptr(cent) if cent.size else None, ptr(labels), ptr(sc),
                                             ctypes.byref(updates), ctypes.byref(conv)))
        finally:
            self.release()
        return cent, labels, sc, int(updates.value), bool(conv.value)

    def topk_candidates(self, q: np.ndarray, offsets, ids, k: int, metric: int):
        """(idx uint32 (m, k), scores float32 (m, k), lens uint32 (m,)) of
        pmm_topk_f32_candidates: row i searched only among the corpus rows
        ``ids[offsets[i]:offsets[i + 1]]`` (strictly ascending row numbers of
        this handle); its first ``lens[i]`` = min(k, count) slots are the exact
        top-k there, the rest hold index 0xFFFFFFFF and score 0.  A plain f32
        handle of one shard; the library's refusal raises ``PmmError``."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError("dimension mismatch")
        m = q.shape[0]
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (m + 1,):
            raise ValueError(f"one list per query row: {m} rows need {m + 1} offsets, got shape {offsets.shape}")
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if ids.size < int(offsets[-1]):
            raise ValueError(f"the offsets end at {int(offsets[-1])}, the ids hold {ids.size}")
        k = int(k)
        idx = np.empty((m, max(k, 0)), dtype=np.uint32)
        sc = np.empty((m, max(k, 0)), dtype=np.float32)
        lens = np.empty(m, dtype=np.uint32)
        self.acquire()
        try:
            check(_lib.pmm_topk_f32_candidates(self._h, ptr(q), m, ptr(offsets), ptr(ids) if ids.size else None, k,
                                               metric, ptr(idx), ptr(sc), ptr(lens)))
        finally:
            self.release()
        return idx, sc, lens

    def _derived(self, h: ctypes.c_void_p) -> "DeviceCorpus":
        """The DeviceCorpus of a handle the library derived from this one."""
        dc = DeviceCorpus.__new__(DeviceCorpus)
        dc.compute, dc.dtype, dc.d = self.compute, self.dtype, self.d
        dc._h = h
        dc._lock = threading.Lock()
        dc._refs = 0
        dc._closing = False
        n = ctypes.c_int64(0)
        check(_lib.pmm_corpus_info(h, ctypes.byref(n), None, None))
        dc.n = int(n.value)
        dc._nbytes0 = subset_device_bytes(dc.n, dc.d, dc.dtype, dc.compute)
        dc._mapped = True
        return dc

    def subset(self, sel) -> "DeviceCorpus":
        """A handle derived on the device for the selected rows
        (pmm_corpus_subset_mask / pmm_corpus_subset_ids): ``sel`` is a bool
        array of length n (numpy, or an Arrow Boolean array without nulls,
        whose bitmap is passed as it is), or an integer array of strictly
        ascending row ids (``ascending_ids`` makes one; the library refuses
        others).  No row is uploaded and no norm
        recomputed; compute mode and dtype are this handle's.  ``topk`` on the
        result searches only those rows and returns THIS handle's row numbers.
        The result is independent of this handle and is closed on its own."""
        if hasattr(sel, "buffers") and hasattr(sel, "offset"):
            # an Arrow Boolean array without nulls: its bitmap goes to the
            # device as it is, at the array's offset (no unpacking here)
            if str(sel.type) != "bool" or sel.null_count or len(sel) != self.n:
                raise ValueError(f"an Arrow mask is a Boolean array of {self.n} rows without nulls")
            buf = sel.buffers()[1]  # (kept alive by sel for the call)
            return self.subset_bitmap(buf.address, sel.offset)
        sel = np.asarray(sel)
        h = ctypes.c_void_p()
        self.acquire()
        try:
            if sel.dtype == np.bool_:
                if sel.shape != (self.n,):
                    raise ValueError(f"a mask selects among {self.n} rows, got shape {sel.shape}")
                bits = np.packbits(sel, bitorder="little")
                check(_lib.pmm_corpus_subset_mask(self._h, ptr(bits), 0, ctypes.byref(h)))
            elif sel.dtype.kind in "iu":
                if sel.ndim != 1 or (sel.size and (int(sel.min()) < 0 or int(sel.max()) > 0xFFFFFFFF)):
                    raise ValueError("row ids are a 1-D array of values in [0, n)")
                ids = np.ascontiguousarray(sel, dtype=np.uint32)
                check(_lib.pmm_corpus_subset_ids(self._h, ptr(ids), ids.size, ctypes.byref(h)))
            else:
                raise TypeError(f"a selection is a bool mask or integer row ids, not {sel.dtype}")
            return self._derived(h)
        finally:
            self.release()

    def subset_bitmap(self, address: int, bit_offset: int) -> "DeviceCorpus":
        """``subset`` for a mask held as an Arrow validity-style bitmap in host
        memory (least significant bit first): row r is selected iff bit
        ``bit_offset + r`` of the bytes at ``address`` is set.  The bitmap is
        uploaded as it is and compacted on the device."""
        h = ctypes.c_void_p()
        self.acquire()
        try:
            check(_lib.pmm_corpus_subset_mask(self._h, ctypes.c_void_p(address), bit_offset, ctypes.byref(h)))
            return self._derived(h)
        finally:
            self.release()

    def partition(self, labels, G: int) -> "DeviceCorpus":
        """A handle derived on the device whose rows are stored grouped by
        label (pmm_corpus_partition): ``labels`` holds one uint32 per row of
        this handle, in [0, G) or ``NO_GROUP`` (the row is dropped).  It
        serves ``topk_grouped`` only; ``topk`` and ``subset`` on it raise."""
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        if labels.shape != (self.n,):
            raise ValueError(f"a partition labels each of {self.n} rows, got shape {labels.shape}")
        h = ctypes.c_void_p()
        self.acquire()
        try:
            check(_lib.pmm_corpus_partition(self._h, ptr(labels), int(G), ctypes.byref(h)))
            dc = self._derived(h)
            dc._nbytes0 = partitioned_device_bytes(dc.n, dc.d, int(G), dc.dtype, dc.compute)
            return dc
        finally:
            self.release()

    def group_offsets(self):
        """A partitioned handle's segment bounds (int64, G + 1 entries); None
        for a handle that is not partitioned (pmm_corpus_groups)."""
        G = ctypes.c_int64(0)
        self.acquire()
        try:
            check(_lib.pmm_corpus_groups(self._h, ctypes.byref(G), None, 0))
            if G.value == 0:
                return None
            off = np.empty(G.value + 1, dtype=np.int64)
            check(_lib.pmm_corpus_groups(self._h, ctypes.byref(G), ptr(off), off.size))
            return off
        finally:
            self.release()

    def topk_grouped(self, q: np.ndarray, qlabels, k: int, metric: int):
        """(idx uint32 (m, k), scores (m, k) in the corpus dtype, lens uint32
        (m,)) of pmm_topk_f32_grouped / pmm_topk_f64_grouped on a partitioned
        handle: row i searched inside group ``qlabels[i]`` only; its first
        ``lens[i]`` slots are the exact top-k there in the PARENT's numbering,
        the rest hold index 0xFFFFFFFF and score 0."""
        q = np.ascontiguousarray(q, dtype=self.dtype)
        if q.shape[1] != self.d:
            raise ValueError("dimension mismatch")
        m = q.shape[0]
        qlabels = np.ascontiguousarray(qlabels, dtype=np.uint32)
        if qlabels.shape != (m,):
            raise ValueError(f"one label per query row: {m} rows, labels of shape {qlabels.shape}")
        idx = np.empty((m, k), dtype=np.uint32)
        sc = np.empty((m, k), dtype=self.dtype)
        lens = np.empty(m, dtype=np.uint32)
        fn = _lib.pmm_topk_f64_grouped if self.dtype == np.float64 else _lib.pmm_topk_f32_grouped
        self.acquire()
        try:
            check(fn(self._h, ptr(q), m, ptr(qlabels), k, metric, ptr(idx), ptr(sc), ptr(lens)))
        finally:
            self.release()
        return idx, sc, lens

    def topk_probed(self, q: np.ndarray, probe_offsets, probe_labels, k: int, metric: int):
        """(idx uint32 (m, k), scores float32 (m, k), lens uint32 (m,)) of
        pmm_topk_f32_probed on a partitioned f32 handle: row i searched in the
        union of the groups ``probe_labels[probe_offsets[i]:probe_offsets[i +
        1]]`` (``NO_GROUP`` entries, labels of empty segments and repeats are
        skipped); its first ``lens[i]`` slots are the exact top-k of that
        union in the PARENT's numbering, ties to the lower parent row, the
        rest hold index 0xFFFFFFFF and score 0.  k <= 128."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError("dimension mismatch")
        m = q.shape[0]
        po, pl = _probe_lists(probe_offsets, probe_labels, m)
        idx = np.empty((m, k), dtype=np.uint32)
        sc = np.empty((m, k), dtype=np.float32)
        lens = np.empty(m, dtype=np.uint32)
        self.acquire()
        try:
            check(_lib.pmm_topk_f32_probed(self._h, ptr(q), m, ptr(po), ptr(pl), k, metric, ptr(idx), ptr(sc),
                                           ptr(lens)))
        finally:
            self.release()
        return idx, sc, lens

    def index_map(self):
        """A derived handle's parent row numbers (uint32, ascending), one per
        row; None for a handle that is not derived."""
        s = ctypes.c_int64(0)
        self.acquire()
        try:
            check(_lib.pmm_corpus_index_map(self._h, None, 0, ctypes.byref(s)))
            if s.value == 0:
                return None
            ids = np.empty(s.value, dtype=np.uint32)
            check(_lib.pmm_corpus_index_map(self._h, ptr(ids), ids.size, ctypes.byref(s)))
            return ids
        finally:
            self.release()

    def _destroy(self) -> None:  # with self._lock held
        if self._h:
            _lib.pmm_corpus_destroy(self._h)
            self._h = ctypes.c_void_p()

    @property
    def shards(self) -> int:
        """Device shards of this corpus (pmm_corpus_shards)."""
        n = ctypes.c_int(0)
        check(_lib.pmm_corpus_shards(self._h, ctypes.byref(n)))
        return n.value

    @property
    def device_dtype(self) -> int:
        """DTYPE_F32 / DTYPE_F64 / DTYPE_BF16 as the library reports it (pmm_corpus_dtype)."""
        v = ctypes.c_int(-1)
        check(_lib.pmm_corpus_dtype(self._h, ctypes.byref(v)))
        return v.value

    @property
    def closed(self) -> bool:
        return not self._h

    def close(self) -> None:
        with self._lock:
            self._closing = True
            if self._refs == 0:
                self._destroy()

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass
