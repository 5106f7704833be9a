"""``polars_matmul._polars_matmul`` -- the extension-module surface of the reference
(src/lib.rs:15-62, module path pyproject.toml:114), re-implemented over the HIP
C ABI.  Exports ``_topk(left, right, k, metric)`` and ``_matmul(left, right)``
with the reference's argument meaning, result dtypes, error texts and edge
rules (``_topk`` also takes ``compute="bf16"``, an extension: both columns read
as f32, searched on the bf16 MFMA path against a cached bf16 corpus handle):

* input extraction / marshalling ..... src/matmul.rs:12-286
* ``_matmul`` -> ``matmul_impl`` ...... src/matmul.rs:295-417
* ``_topk``   -> ``topk_impl`` ........ src/matmul.rs:420-519

Inputs may be a Polars ``Series`` (``List``/``Array`` of floats; converted with
``rechunk().to_arrow()``, zero-copy for ``Array[f32|f64]``), a pyarrow
``(Large)List`` / ``FixedSizeList`` array or chunked array, or a 2-D numpy
array.  The result is a Polars ``Series`` when Polars is importable and the
query input was a Polars ``Series``, otherwise a pyarrow array of the same
logical type:

* ``_topk``   -> ``List[Struct{index: UInt32, score: Float64}]`` named "topk"
* ``_matmul`` -> ``Array[Float32|Float64, N]`` named "matmul"

Errors: the reference maps ``PolarsError`` to ``RuntimeError`` (src/lib.rs:28,
53); the same message texts are raised here.  A negative ``k`` raises
``OverflowError`` (pyo3's usize conversion); a List row longer than the first
row raises ``PanicException`` (the reference panics on the ndarray index,
src/matmul.rs:276-283).
"""
from __future__ import annotations

import collections
import os
import threading
import time

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from . import _native

try:  # Polars is optional: the HIP path does not need it.
    import polars as _pl  # type: ignore
except Exception:  # pragma: no cover - polars is not installed in this image
    _pl = None


# Host-side phase timer for bench.py's end-to-end breakdown: when set to a
# dict, _topk / _matmul add the seconds of each phase (extract: Arrow/numpy ->
# contiguous matrices; device: the C-ABI call -- upload, kernels, download;
# assemble: result dtype widening and Arrow assembly).  None (default): off.
PHASES = None


def _lap(name: str, t0: float) -> float:
    t = time.perf_counter()
    ph = PHASES
    if ph is not None:
        ph[name] = ph.get(name, 0.0) + (t - t0)
    return t


class PanicException(BaseException):
    """Mirror of pyo3's PanicException (a BaseException subclass)."""


def _compute_error(msg: str) -> RuntimeError:
    return RuntimeError(msg)


# ---------------------------------------------------------------------------
# Input normalisation
# ---------------------------------------------------------------------------
def _is_polars_series(obj) -> bool:
    return _pl is not None and isinstance(obj, _pl.Series)


def _to_arrow(obj):
    """Return a single-chunk pyarrow Array (List / LargeList / FixedSizeList) or a
    2-D numpy array."""
    if _is_polars_series(obj):
        obj = obj.rechunk().to_arrow()
    if isinstance(obj, np.ndarray):
        if obj.ndim != 2:
            raise TypeError(f"expected a 2-D array of embeddings, got shape {obj.shape}")
        return obj
    if isinstance(obj, pa.ChunkedArray):
        obj = obj.combine_chunks() if obj.num_chunks != 1 else obj.chunk(0)
    if isinstance(obj, pa.Array):
        return obj
    if isinstance(obj, (list, tuple)):
        return pa.array(obj)
    raise TypeError(f"unsupported embedding container: {type(obj).__name__}")


def _is_f32(arr) -> bool:
    """src/matmul.rs:13-19: List[f32] or Array[f32, d]."""
    if isinstance(arr, np.ndarray):
        return arr.dtype == np.float32
    t = arr.type
    if pa.types.is_list(t) or pa.types.is_large_list(t) or pa.types.is_fixed_size_list(t):
        return t.value_type == pa.float32()
    return False


def _is_i8(arr) -> bool:
    """List[i8] / Array[i8, d] / an int8 matrix: rows of signed bytes."""
    if isinstance(arr, np.ndarray):
        return arr.dtype == np.int8
    t = arr.type
    if pa.types.is_list(t) or pa.types.is_large_list(t) or pa.types.is_fixed_size_list(t):
        return t.value_type == pa.int8()
    return False


def _is_u8(arr) -> bool:
    """List[u8] / Array[u8, w] / a uint8 matrix: rows of packed bits."""
    if isinstance(arr, np.ndarray):
        return arr.dtype == np.uint8
    t = arr.type
    if pa.types.is_list(t) or pa.types.is_large_list(t) or pa.types.is_fixed_size_list(t):
        return t.value_type == pa.uint8()
    return False


def _nrows(arr) -> int:
    return arr.shape[0] if isinstance(arr, np.ndarray) else len(arr)


def _values_numpy(values: pa.Array, np_dtype) -> np.ndarray:
    """Child values cast to the compute dtype, nulls -> 0.0 (src/matmul.rs:192, 224)."""
    if np_dtype == np.int8:  # (only int8 children come here: borrowed as they are)
        target, zero = pa.int8(), 0
    elif np_dtype == np.uint8:  # (packed bit rows, _topk_hamming: only uint8 children)
        target, zero = pa.uint8(), 0
    else:
        target, zero = (pa.float32() if np_dtype == np.float32 else pa.float64()), 0.0
    if values.type != target:
        values = pc.cast(values, target)
    if values.null_count:
        values = values.fill_null(zero)
    return values.to_numpy(zero_copy_only=False)


def _series_to_matrix(arr, np_dtype) -> np.ndarray:
    """series_to_matrix{,_f32} (src/matmul.rs:131-286): a C-contiguous (rows, d)
    matrix of the compute dtype.  Zero-copy when the input is already a
    contiguous Array of that dtype (src/matmul.rs:22-95)."""
    n = _nrows(arr)
    if n == 0:
        raise _compute_error("Empty series")
    if isinstance(arr, np.ndarray):
        if arr.shape[1] == 0:
            raise _compute_error("Zero-dimensional vectors")
        return np.ascontiguousarray(arr, dtype=np_dtype)
    t = arr.type
    if pa.types.is_fixed_size_list(t):
        d = t.list_size
        if d == 0:
            raise _compute_error("Zero-dimensional vectors")
        child = arr.values.slice(arr.offset * d, n * d)
        if arr.null_count == 0:
            vals = _values_numpy(child, np_dtype)
            return np.ascontiguousarray(vals.reshape(n, d))
        # null outer rows carry null children in Polars: they read as zeros
        vals = _values_numpy(child, np_dtype).reshape(n, d).copy()
        valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
        vals[~valid] = 0
        return vals
    if pa.types.is_list(t) or pa.types.is_large_list(t):
        if not arr[0].is_valid:
            raise _compute_error("First element is null")
        offsets = np.asarray(arr.offsets.to_numpy(zero_copy_only=False), dtype=np.int64)
        lens = np.diff(offsets)
        d = int(lens[0])
        if d == 0:
            raise _compute_error("Zero-dimensional vectors")
        valid = (
            np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
            if arr.null_count
            else np.ones(n, dtype=bool)
        )
        lens = np.where(valid, lens, 0)
        if np.any(lens > d):
            bad = int(np.argmax(lens > d))
            raise PanicException(
                f"ndarray: index out of bounds: row {bad} has {int(lens[bad])} elements, "
                f"the first row has {d}"
            )
        lo, hi = int(offsets[0]), int(offsets[-1])
        vals = _values_numpy(arr.values.slice(lo, hi - lo), np_dtype)
        if valid.all() and np.all(lens == d):
            return np.ascontiguousarray(vals.reshape(n, d))
        out = np.zeros((n, d), dtype=np_dtype)
        rows = np.repeat(np.arange(n), lens)
        starts = offsets[:-1] - lo
        cols = np.arange(rows.size) - np.repeat(np.cumsum(lens) - lens, lens)
        src = np.repeat(starts, lens) + cols
        out[rows, cols] = vals[src]
        return out
    raise _compute_error(f"expected List or Array of numbers, got {t}")


def _dim_mismatch(dl: int, dr: int) -> RuntimeError:
    return _compute_error(
        f"Dimension mismatch: left has {dl} dimensional vectors, "
        f"right has {dr} dimensional vectors"
    )


def _as_usize(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"'{type(k).__name__}' object cannot be interpreted as an integer")
    k = int(k)
    if k < 0:
        raise OverflowError("can't convert negative int to unsigned")
    return k


# ---------------------------------------------------------------------------
# Device-resident corpus cache, for both branches of the
# reference (f32 and f64 rows; src/matmul.rs:427-468).  Polars' map_batches may
# call _topk repeatedly with the same corpus Series.  Only corpora that came
# in as Polars Series or Arrow arrays are cached (their buffers persist across
# calls; a Python list or numpy matrix is rebuilt or mutable, so it would only
# fill the cache), identified by the buffers' addresses and sizes while the
# cache holds a reference to the Arrow array (the addresses cannot be reused
# meanwhile).  Arrow data is immutable by contract: a Series that shares
# memory with a numpy array the caller then writes to in place gives stale
# cached results -- clear_corpus_cache() or PMM_CORPUS_CACHE=0 in that case.
# PMM_CORPUS_CACHE_BYTES bounds the HBM the cache holds (default 8 GiB), and
# a corpus is cached only while it takes at most half of the device's free HBM
# (pmm_device_memory), so the cache never crowds out the searches themselves.
# Handles are reference-counted (DeviceCorpus.acquire/release), so evicting
# or clearing never frees a corpus another thread is searching.
# ---------------------------------------------------------------------------

_cache_lock = threading.Lock()
_cache: "collections.OrderedDict" = collections.OrderedDict()
_CACHE_ON = os.environ.get("PMM_CORPUS_CACHE", "1") != "0"
_CACHE_BYTES = int(os.environ.get("PMM_CORPUS_CACHE_BYTES", str(8 << 30)))
_CACHE_MIN_BYTES = 1 << 20  # small corpora are cheaper to upload than to cache


def _fits_device(nbytes: int) -> bool:
    try:
        free, _ = _native.device_memory()
    except _native.PmmError:
        return False
    return nbytes <= free // 2


def _arrow_key(arr):
    if not isinstance(arr, pa.Array):
        return None
    bufs = tuple((b.address, b.size) if b is not None else None for b in arr.buffers())
    return (str(arr.type), arr.offset, len(arr), bufs)


def _persistent_key(original, arrow):
    """``_arrow_key`` of an input whose Arrow buffers persist across calls,
    else None: a single-chunk Polars Series (rechunk() then returns the same
    buffers; a multi-chunk one is concatenated into a fresh buffer on every
    call, whose address key would never hit while each miss pinned host and
    device memory), an Arrow array, or a single-chunk ChunkedArray."""
    if _is_polars_series(original):
        if original.n_chunks() != 1:
            return None
    elif not (isinstance(original, pa.Array)
              or (isinstance(original, pa.ChunkedArray) and original.num_chunks == 1)):
        return None
    return _arrow_key(arrow)


def _handle_bytes(c: np.ndarray, compute: str, doc_offsets=None) -> int:
    """HBM the cached handle of c holds; compute "bits" (the key mode of
    ``_topk_hamming``, not a ``compute=`` value): c is packed bit rows;
    compute "maxsim" (the key mode of ``_topk_maxsim``): c is the token rows
    of a multi-vector column and ``doc_offsets`` its documents' bounds."""
    if compute == "bits":
        return _native.bits_device_bytes(c.shape[0], c.shape[1])
    if compute == "maxsim":
        return _native.corpus_device_bytes(c.shape[0], c.shape[1], c.dtype, "f32") + 8 * int(doc_offsets.size)
    return _native.corpus_device_bytes(c.shape[0], c.shape[1], c.dtype, compute)


def _corpus_key(original, rv, c: np.ndarray, compute: str, numpy_ok: bool = False, doc_offsets=None):
    """The cache key of this corpus, or None when it is not cacheable.
    numpy_ok (the numpy-level ``within``): a numpy matrix that is searched as
    it is (C-contiguous, already of the compute dtype) is keyed by its address
    and shape while the cache holds a reference to it; a caller that writes to
    it in place gets stale results, as with Arrow buffers (above)."""
    key = _persistent_key(original, rv)
    if key is None and numpy_ok and isinstance(original, np.ndarray) and c is original:
        key = ("ndarray", c.ctypes.data, c.shape)
    if key is not None:
        # the compute dtype: an f32 column searched by f64 queries runs the
        # f64 branch (src/matmul.rs:427) on an f64 copy of the same buffers;
        # a handle is sharded over the device list of its creation; an f32
        # and a bf16 handle of one column are two entries
        key = key + (c.dtype.str, tuple(_native.get_devices()), compute)
    dev_bytes = _handle_bytes(c, compute, doc_offsets)
    if not _CACHE_ON or key is None or c.nbytes < _CACHE_MIN_BYTES or dev_bytes > _CACHE_BYTES:
        return None
    return key


def _cached_corpus(original, rv, c: np.ndarray, compute: str = "f32", numpy_ok: bool = False, doc_offsets=None):
    """An ACQUIRED DeviceCorpus for this corpus (the caller releases it), or
    None when the corpus is not cacheable.  compute "maxsim": the multi-vector
    handle of the token rows c and their documents' bounds ``doc_offsets``."""
    key = _corpus_key(original, rv, c, compute, numpy_ok, doc_offsets)
    if key is None:
        return None
    dev_bytes = _handle_bytes(c, compute, doc_offsets)
    with _cache_lock:
        hit = _cache.get(key)
        if hit is not None:
            _cache.move_to_end(key)
            return hit[1].acquire()
        if not _fits_device(dev_bytes):
            return None
        dc = (_native.DeviceCorpus.bits(c) if compute == "bits" else
              _native.DeviceCorpus.multivector(c, doc_offsets) if compute == "maxsim" else
              _native.DeviceCorpus.int8(c) if c.dtype == np.int8 and compute == "f32" else
              _native.DeviceCorpus(c) if compute == "f32" else _native.DeviceCorpus(c, compute=compute))
        _cache[key] = (rv, dc)
        total = sum(v[1].nbytes for v in _cache.values())
        while total > _CACHE_BYTES and len(_cache) > 1:
            _, (_, old) = _cache.popitem(last=False)
            total -= old.nbytes
            old.close()  # freed now, or by its last in-flight user
        return dc.acquire()


def _cache_hit(original, rv, c: np.ndarray, compute: str = "f32"):
    """The ACQUIRED cached handle of this corpus when the cache holds one (the
    caller releases it), else None: nothing is created or uploaded."""
    key = _corpus_key(original, rv, c, compute)
    if key is None:
        return None
    with _cache_lock:
        hit = _cache.get(key)
        return hit[1].acquire() if hit is not None else None


def _reaccount_cache(used) -> None:
    """After a call on the cached handle ``used``: an f32 handle grows when its
    first screened cosine call builds its screen image (DeviceCorpus.nbytes
    reports the library's figure), so the cache is summed again and
    least-recently-used OTHER entries leave while it holds more than
    PMM_CORPUS_CACHE_BYTES.  The entry in use stays."""
    with _cache_lock:
        total = sum(v[1].nbytes for v in _cache.values())
        for key in list(_cache):  # least recently used first
            if total <= _CACHE_BYTES:
                break
            old = _cache[key][1]
            if old is used:
                continue
            del _cache[key]
            total -= old.nbytes
            old.close()  # freed now, or by its last in-flight user


def clear_corpus_cache() -> None:
    with _cache_lock:
        while _cache:
            _, (_, dc) = _cache.popitem()
            dc.close()


# ---------------------------------------------------------------------------
# subset=: search only some rows of the corpus (an extension; the reference
# filters the corpus frame on the host, which here would miss the cache,
# upload the kept rows again and number the result by the filtered frame).
# The selection becomes a handle derived on the device from the cached parent
# (DeviceCorpus.subset), cached beside it under the parent's key plus the
# selection's buffers.
# ---------------------------------------------------------------------------
class _Selection:
    """A checked ``subset=`` argument: ``mask`` (an Arrow Boolean array of
    len(corpus) without nulls) or ``ids`` (uint32, ascending, unique), the
    number of selected rows, and -- when the argument's buffers persist across
    calls -- their ``_arrow_key`` with the array that keeps them alive."""

    __slots__ = ("mask", "ids", "count", "key", "keep")

    def __init__(self, mask, ids, count, key, keep):
        self.mask, self.ids, self.count, self.key, self.keep = mask, ids, count, key, keep

    def row_ids(self) -> np.ndarray:
        if self.ids is None:
            self.ids = np.flatnonzero(self.mask.to_numpy(zero_copy_only=False)).astype(np.uint32)
        return self.ids


def _check_subset(subset, n: int) -> _Selection:
    """TypeError / ValueError for a selection of the wrong kind or length, the
    compute error for an empty one or an id outside the corpus: all before
    any device work."""
    original = subset
    if _is_polars_series(subset):
        subset = subset.rechunk().to_arrow()
    if isinstance(subset, pa.ChunkedArray):
        subset = subset.combine_chunks() if subset.num_chunks != 1 else subset.chunk(0)
    if isinstance(subset, (list, tuple)):
        subset = np.asarray(subset)
    key = keep = mask = ids = None
    if isinstance(subset, pa.Array):
        key, keep = _persistent_key(original, subset), subset
        if pa.types.is_boolean(subset.type):
            mask = subset
        elif pa.types.is_integer(subset.type):
            ids = (subset.drop_null() if subset.null_count else subset).to_numpy(zero_copy_only=False)
        else:
            raise TypeError(f"subset must be a Boolean mask or integer row ids, got {subset.type}")
    elif isinstance(subset, np.ndarray):
        if subset.dtype == np.bool_:
            if subset.ndim != 1:
                raise ValueError(f"subset mask must be 1-D, got shape {subset.shape}")
            mask = pa.array(subset)
        elif subset.dtype.kind in "iu":
            ids = subset
        else:
            raise TypeError(f"subset must be a Boolean mask or integer row ids, got {subset.dtype}")
    else:
        raise TypeError(f"subset must be a Series or array (a Boolean mask or integer row ids), "
                        f"got {type(original).__name__}")
    if mask is not None:
        if len(mask) != n:
            raise ValueError(f"subset mask has {len(mask)} rows, the corpus has {n}")
        if mask.null_count:  # nulls count as false
            mask = mask.fill_null(False)
        count = mask.true_count
    else:
        try:
            ids = _native.ascending_ids(ids, n)
        except ValueError as e:
            raise _compute_error(str(e)) from None
        count = int(ids.size)
    if count == 0:
        raise _compute_error("Empty series")  # what an empty corpus raises
    return _Selection(mask, ids, count, key, keep)


def _cached_subset(parent, parent_key, sel: _Selection, c: np.ndarray, compute: str):
    """(an ACQUIRED derived DeviceCorpus for ``sel`` of the cached ``parent``,
    transient) -- the caller releases it, and closes it when ``transient`` (a
    selection whose buffers do not persist is derived per call and not
    cached) -- or (None, False) when it would not fit in half of the free HBM."""
    key = None if sel.key is None else parent_key + ("subset", sel.key)
    need = _native.subset_device_bytes(sel.count, c.shape[1], c.dtype, compute)
    with _cache_lock:
        hit = _cache.get(key) if key is not None else None
        if hit is not None:
            _cache.move_to_end(key)
            return hit[1].acquire(), False
        if not _fits_device(need):
            return None, False
        dc = parent.subset(sel.mask if sel.mask is not None else sel.ids)
        if key is None or need > _CACHE_BYTES:
            return dc.acquire(), True
        _cache[key] = ((sel.keep, sel.mask), dc)  # the entry keeps the selection's buffers alive
        total = sum(v[1].nbytes for v in _cache.values())
        while total > _CACHE_BYTES and len(_cache) > 1:
            _, (_, old) = _cache.popitem(last=False)
            total -= old.nbytes
            old.close()  # freed now, or by its last in-flight user
        return dc.acquire(), False


def _topk_subset(q, c, original, rv, sel: _Selection, kk: int, metric_id: int, compute: str):
    """Top-kk of q among the selected rows of c, indices numbering c.  On the
    device from the cached corpus handle when there is one (one GPU); else the
    host fallback: the selected rows taken on the host, the uncached search,
    and the indices mapped back through the ids."""
    dc, transient = None, False
    if len(_native.get_devices()) <= 1:
        parent_key = _corpus_key(original, rv, c, compute)
        parent = _cached_corpus(original, rv, c, compute) if parent_key is not None else None
        if parent is not None:
            try:
                dc, transient = _cached_subset(parent, parent_key, sel, c, compute)
            finally:
                parent.release()
    if dc is not None:
        try:
            idx, sc = dc.topk(q, kk, metric_id)
            if not transient:
                _reaccount_cache(dc)
        finally:
            dc.release()
            if transient:
                dc.close()
        return idx, sc
    ids = sel.row_ids()
    idx, sc = _native.topk_host(q, np.ascontiguousarray(c[ids]), kk, metric_id,
                                compute=_native.COMPUTE_BF16 if compute == "bf16" else _native.COMPUTE_F32)
    return ids[idx], sc


# ---------------------------------------------------------------------------
# groups=: search every query row among the corpus rows of its own label (an
# extension: Polars' over() / group_by on a search; with subset= it takes one
# derived handle, three launches and one Python iteration per distinct label).
# The labels of both sides are encoded on the host, the corpus' labels become
# a handle derived on the device from the cached parent whose rows are stored
# group by group (DeviceCorpus.partition), cached beside it under the parent's
# key plus the label array's buffers, and one call searches every query in its
# group's segment (DeviceCorpus.topk_grouped).
# Probed search: when the left side holds one LIST of labels per query row (an
# Arrow List / LargeList / FixedSizeList, or a 2-D integer matrix), every row is
# searched in the union of its labels' segments on the same partitioned handle
# (DeviceCorpus.topk_probed) -- IVF with nprobe lists, rows visible in several
# groups.
# ---------------------------------------------------------------------------
class _Groups:
    """A checked ``groups=`` argument: uint32 labels of the query rows and of
    the corpus rows in [0, G) (``_native.NO_GROUP``: matches nothing), the
    corpus rows per label, and -- when the corpus labels' buffers persist
    across calls -- their ``_arrow_key`` with the array that keeps them alive.
    Probed search (a list of labels per query row): ``probe_offsets`` (int64,
    m + 1) cuts ``qlabels``, the flattened labels, into the rows' lists."""

    __slots__ = ("qlabels", "clabels", "G", "sizes", "key", "keep", "probe_offsets")

    def __init__(self, qlabels, clabels, G, key, keep, probe_offsets=None):
        self.qlabels, self.clabels, self.G, self.key, self.keep = qlabels, clabels, G, key, keep
        self.probe_offsets = probe_offsets
        self.sizes = np.bincount(clabels[clabels != _native.NO_GROUP], minlength=G).astype(np.int64)

    def probe_pairs(self) -> np.ndarray:
        """Probed search: the distinct (label, query row) pairs with a
        non-empty segment, int64 (pairs, 2), sorted by label, then row."""
        rows = np.repeat(np.arange(self.probe_offsets.size - 1, dtype=np.int64), np.diff(self.probe_offsets))
        keep = self.qlabels != _native.NO_GROUP
        keep[keep] = self.sizes[self.qlabels[keep]] > 0
        pairs = np.stack([self.qlabels[keep].astype(np.int64), rows[keep]], axis=1)
        return np.unique(pairs, axis=0) if pairs.size else pairs

    def searched_max(self) -> int:
        """Rows of the largest segment (probed search: union of segments)
        some query searches (0: none does)."""
        if self.probe_offsets is not None:
            pairs = self.probe_pairs()
            if not pairs.size:
                return 0
            return int(np.bincount(pairs[:, 1], weights=self.sizes[pairs[:, 0]]).max())
        ql = self.qlabels[self.qlabels != _native.NO_GROUP]
        return int(self.sizes[ql].max()) if ql.size else 0


def _probe_lists(obj):
    """(offsets int64 (m + 1,), the flattened labels) when ``obj`` holds one
    list of labels per row -- an Arrow List / LargeList / FixedSizeList (a
    null list is empty) or a 2-D integer matrix [m, P] -- else None."""
    if isinstance(obj, np.ndarray) and obj.ndim == 2:
        if obj.dtype.kind not in "iu":
            raise TypeError(f"a matrix of probe labels must hold integers, got {obj.dtype}")
        m, P = obj.shape
        return np.arange(m + 1, dtype=np.int64) * P, np.ascontiguousarray(obj).reshape(-1)
    if _is_polars_series(obj):
        obj = obj.rechunk().to_arrow()
    if isinstance(obj, pa.ChunkedArray):
        obj = obj.combine_chunks() if obj.num_chunks != 1 else obj.chunk(0)
    if not isinstance(obj, pa.Array):
        return None
    t = obj.type
    if not (pa.types.is_list(t) or pa.types.is_large_list(t) or pa.types.is_fixed_size_list(t)):
        return None
    lens = pc.fill_null(pc.list_value_length(obj), 0).to_numpy(zero_copy_only=False).astype(np.int64)
    if obj.null_count:  # (a null list's slots leave with it)
        obj = obj.filter(obj.is_valid())
    offsets = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return offsets, obj.flatten()


def _label_array(obj, what: str):
    """(the labels as one Arrow array of a plain hashable type, the array
    whose buffers the caller passed)."""
    if _is_polars_series(obj):
        obj = obj.rechunk().to_arrow()
    if isinstance(obj, pa.ChunkedArray):
        obj = obj.combine_chunks() if obj.num_chunks != 1 else obj.chunk(0)
    if isinstance(obj, np.ndarray):
        if obj.ndim != 1:
            raise ValueError(f"{what} labels must be 1-D, got shape {obj.shape}")
        obj = pa.array(obj)
    elif isinstance(obj, (list, tuple)):
        obj = pa.array(obj)
    if not isinstance(obj, pa.Array):
        raise TypeError(f"{what} labels must be a Series or array, got {type(obj).__name__}")
    arr = obj
    if pa.types.is_dictionary(arr.type):  # a categorical: compared by value
        arr = arr.dictionary_decode()
    t = arr.type
    if pa.types.is_string(t) or (hasattr(pa.types, "is_string_view") and pa.types.is_string_view(t)):
        arr = pc.cast(arr, pa.large_string())
    elif pa.types.is_binary(t):
        arr = pc.cast(arr, pa.large_binary())
    t = arr.type
    if pa.types.is_nested(t) or pa.types.is_floating(t) or pa.types.is_null(t):
        raise TypeError(f"{what} labels must be of a hashable type (integers, strings, categoricals), got {t}")
    return arr, obj


def _check_groups(groups, m: int, n: int) -> _Groups:
    """TypeError for labels of the wrong kind or of two different types,
    ValueError for a wrong length: all before any device work.  The corpus
    labels are dictionary-encoded, the query labels looked up in that
    dictionary; a null on either side matches nothing, and a query label the
    corpus does not have searches nothing."""
    if not isinstance(groups, (tuple, list)) or len(groups) != 2:
        raise TypeError("groups must be a pair (left_labels, right_labels)")
    right_original = groups[1]
    probes = _probe_lists(groups[0])  # a list of labels per row: probed search
    left, _ = _label_array(groups[0] if probes is None else probes[1], "left")
    right, right_arrow = _label_array(groups[1], "right")
    if left.type != right.type:
        raise TypeError(f"groups labels must have one type, got {left.type} (left) and {right.type} (right)")
    if (len(left) if probes is None else probes[0].size - 1) != m:
        raise ValueError(f"left labels have {len(left) if probes is None else probes[0].size - 1} rows, "
                         f"the queries have {m}")
    if len(right) != n:
        raise ValueError(f"right labels have {len(right)} rows, the corpus has {n}")
    enc = right.dictionary_encode()
    none = pa.scalar(_native.NO_GROUP, type=pa.uint32())
    clabels = pc.fill_null(pc.cast(enc.indices, pa.uint32()), none).to_numpy(zero_copy_only=False)
    qlabels = pc.fill_null(pc.cast(pc.index_in(left, value_set=enc.dictionary), pa.uint32()), none)
    qlabels = qlabels.to_numpy(zero_copy_only=False)
    return _Groups(np.ascontiguousarray(qlabels, dtype=np.uint32), np.ascontiguousarray(clabels, dtype=np.uint32),
                   len(enc.dictionary), _persistent_key(right_original, right_arrow), right_arrow,
                   None if probes is None else probes[0])


def _cached_partition(parent, parent_key, grp: _Groups, c: np.ndarray, compute: str):
    """(an ACQUIRED partitioned DeviceCorpus of the cached ``parent`` for the
    corpus labels of ``grp``, transient) as ``_cached_subset``, or (None,
    False) when it would not fit in half of the free HBM."""
    key = None if grp.key is None else parent_key + ("groups", grp.key)
    need = _native.partitioned_device_bytes(int(grp.sizes.sum()), c.shape[1], grp.G, c.dtype, compute)
    with _cache_lock:
        hit = _cache.get(key) if key is not None else None
        if hit is not None:
            _cache.move_to_end(key)
            return hit[1].acquire(), False
        if not _fits_device(need):
            return None, False
        dc = parent.partition(grp.clabels, grp.G)
        if key is None or need > _CACHE_BYTES:
            return dc.acquire(), True
        _cache[key] = (grp.keep, dc)  # the entry keeps the label array's buffers alive
        total = sum(v[1].nbytes for v in _cache.values())
        while total > _CACHE_BYTES and len(_cache) > 1:
            _, (_, old) = _cache.popitem(last=False)
            total -= old.nbytes
            old.close()  # freed now, or by its last in-flight user
        return dc.acquire(), False


def _partitioned_handle(c, original, rv, grp: _Groups, compute: str):
    """(an ACQUIRED partitioned DeviceCorpus for ``grp``'s corpus labels,
    transient), or (None, False): no cacheable parent, several devices, bf16
    compute, a sharded parent, or a handle that does not fit."""
    dc, transient = None, False
    if len(_native.get_devices()) <= 1 and compute != "bf16" and grp.sizes.sum() > 0:
        parent_key = _corpus_key(original, rv, c, compute)
        parent = _cached_corpus(original, rv, c, compute) if parent_key is not None else None
        if parent is not None:
            try:
                if parent.shards == 1:
                    dc, transient = _cached_partition(parent, parent_key, grp, c, compute)
            finally:
                parent.release()
    return dc, transient


_PROBED_MAX_K = 128  # pmm_topk_f32_probed's list length (the grouped kernel's)


def _merge_probed(cand_row, cand_id, cand_sc, m: int, kk: int, euclidean: bool, dtype):
    """Per query row the best kk of its candidates (flat arrays: row, corpus
    row, score) under the library's order -- best score first, NaN last, equal
    scores to the lower corpus row -- as (idx (m, kk), scores, lens)."""
    idx = np.full((m, kk), 0xFFFFFFFF, dtype=np.uint32)
    sc = np.zeros((m, kk), dtype=dtype)
    lens = np.zeros(m, dtype=np.uint32)
    if cand_row.size == 0:
        return idx, sc, lens
    nan = np.isnan(cand_sc)
    rank = np.where(nan, 0, cand_sc if euclidean else -cand_sc)  # ascending = best first; the zeros tie
    order = np.lexsort((cand_id, rank, nan, cand_row))
    rows = cand_row[order]
    start = np.searchsorted(rows, np.arange(m))
    pos = np.arange(rows.size) - start[rows]
    take = pos < kk
    idx[rows[take], pos[take]] = cand_id[order][take]
    sc[rows[take], pos[take]] = cand_sc[order][take]
    lens[:] = np.minimum(np.bincount(rows, minlength=m), kk)
    return idx, sc, lens


def _topk_probed(q, c, original, rv, grp: _Groups, kk: int, metric_id: int, compute: str):
    """(idx (m, kk), scores (m, kk), lens (m,)): row i's first lens[i] slots
    are its top-kk among the corpus rows of ALL its labels, indices numbering
    c, ties to the lower corpus row.  On the device in one call on the
    partitioned handle ``groups=`` caches (f32 rows, kk <= 128); else on the
    host: one uncached search per distinct label for the rows that probe it
    and a per-row merge by (score, corpus row) -- the same bits for f32."""
    dc, transient = None, False
    if q.dtype == np.float32 and kk <= _PROBED_MAX_K:
        dc, transient = _partitioned_handle(c, original, rv, grp, compute)
    if dc is not None:
        try:
            idx, sc, lens = dc.topk_probed(q, grp.probe_offsets, grp.qlabels, kk, metric_id)
            if not transient:
                _reaccount_cache(dc)
        finally:
            dc.release()
            if transient:
                dc.close()
        return idx, sc, lens
    m = q.shape[0]
    mode = _native.COMPUTE_BF16 if compute == "bf16" else _native.COMPUTE_F32
    pairs = grp.probe_pairs()
    cr, ci, cs = [np.zeros(0, np.int64)], [np.zeros(0, np.uint32)], [np.zeros(0, q.dtype)]
    cuts = np.flatnonzero(np.diff(pairs[:, 0])) + 1 if pairs.size else np.zeros(0, np.int64)
    for part in np.split(pairs, cuts) if pairs.size else []:
        ids = np.flatnonzero(grp.clabels == part[0, 0]).astype(np.uint32)
        rows = part[:, 1]
        kg = min(kk, int(ids.size))
        gi, gs = _native.topk_host(np.ascontiguousarray(q[rows]), np.ascontiguousarray(c[ids]), kg, metric_id,
                                   compute=mode)
        cr.append(np.repeat(rows, kg))
        ci.append(ids[gi].reshape(-1))
        cs.append(np.asarray(gs, dtype=q.dtype).reshape(-1))
    return _merge_probed(np.concatenate(cr), np.concatenate(ci), np.concatenate(cs), m, kk,
                         metric_id == _native.METRIC_EUCLIDEAN, q.dtype)


def _topk_grouped(q, c, original, rv, grp: _Groups, kk: int, metric_id: int, compute: str):
    """(idx (m, kk), scores (m, kk), lens (m,)): row i's first lens[i] slots
    are its top-kk among the corpus rows of its label, indices numbering c.  On
    the device from a partitioned handle of the cached corpus when there is
    one (one GPU, f32 or f64 rows); else the host fallback: one uncached
    search per distinct label on that label's rows, mapped back."""
    if grp.probe_offsets is not None:
        return _topk_probed(q, c, original, rv, grp, kk, metric_id, compute)
    dc, transient = _partitioned_handle(c, original, rv, grp, compute)
    if dc is not None:
        try:
            idx, sc, lens = dc.topk_grouped(q, grp.qlabels, kk, metric_id)
            if not transient:
                _reaccount_cache(dc)
        finally:
            dc.release()
            if transient:
                dc.close()
        return idx, sc, lens
    m = q.shape[0]
    idx = np.full((m, kk), 0xFFFFFFFF, dtype=np.uint32)
    sc = np.zeros((m, kk), dtype=q.dtype)
    lens = np.zeros(m, dtype=np.uint32)
    mode = _native.COMPUTE_BF16 if compute == "bf16" else _native.COMPUTE_F32
    for g in np.unique(grp.qlabels[grp.qlabels != _native.NO_GROUP]):
        ids = np.flatnonzero(grp.clabels == g).astype(np.uint32)
        if ids.size == 0:
            continue
        rows = np.flatnonzero(grp.qlabels == g)
        kg = min(kk, int(ids.size))
        gi, gs = _native.topk_host(np.ascontiguousarray(q[rows]), np.ascontiguousarray(c[ids]), kg, metric_id,
                                   compute=mode)
        idx[rows, :kg] = ids[gi]
        sc[rows, :kg] = gs
        lens[rows] = kg
    return idx, sc, lens


# ---------------------------------------------------------------------------
# candidates=: every query row brings its own list of corpus rows (an
# extension: the second stage of a hybrid or two-stage search, per-row
# permissions).  The lists are checked, sorted and de-duplicated on the host
# in one vectorised pass and searched in ONE call on the cached f32 handle
# (DeviceCorpus.topk_candidates); there is no per-row loop anywhere.
# ---------------------------------------------------------------------------
def _candidates_f32_only(what: str) -> TypeError:
    return TypeError(
        f"candidate search runs on Float32 columns ({what}); cast the embeddings first, e.g. "
        "pl.col('embedding').cast(pl.List(pl.Float32)) or array.astype(numpy.float32)"
    )


class _Candidates:
    """A checked ``candidates=`` argument in the library's form: ``offsets``
    (int64, m + 1) and ``ids`` (uint32), every row's ids strictly ascending
    and below n; ``maxlen`` is the longest list."""

    __slots__ = ("offsets", "ids", "maxlen")

    def __init__(self, offsets, ids):
        self.offsets, self.ids = offsets, ids
        self.maxlen = int(np.diff(offsets).max()) if offsets.size > 1 else 0


def _check_candidates(candidates, m: int, n: int) -> _Candidates:
    """TypeError for lists of the wrong kind, ValueError for a wrong number
    of lists or an id that is null, negative or no row of the corpus (naming
    the query row): all before any device work.  A null list is empty."""
    if isinstance(candidates, (tuple, list)) and len(candidates) == 2 and all(
            isinstance(x, np.ndarray) for x in candidates):
        offsets, vals = candidates
        if offsets.dtype.kind not in "iu" or vals.dtype.kind not in "iu":
            raise TypeError(f"candidates (offsets, ids) must be integer arrays, got {offsets.dtype} and {vals.dtype}")
        if offsets.ndim != 1 or vals.ndim != 1:
            raise ValueError("candidates (offsets, ids) must be 1-D arrays")
        if offsets.size != m + 1:
            raise ValueError(f"candidates hold {max(offsets.size - 1, 0)} lists, the queries have {m} rows")
        offsets = offsets.astype(np.int64)
        lens = np.diff(offsets)
        if offsets[0] != 0 or np.any(lens < 0) or offsets[-1] != vals.size:
            raise ValueError("candidates offsets must start at 0, not descend and end at len(ids)")
        null = None
    else:
        arr = candidates
        if _is_polars_series(arr):
            arr = arr.rechunk().to_arrow()
        if isinstance(arr, pa.ChunkedArray):
            arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
        if not isinstance(arr, pa.Array):
            raise TypeError("candidates must be a Series or Arrow List of integer row ids, or a pair (offsets, ids) "
                            f"of numpy arrays, got {type(candidates).__name__}")
        t = arr.type
        if not (pa.types.is_list(t) or pa.types.is_large_list(t)) or not pa.types.is_integer(t.value_type):
            raise TypeError(f"candidates must be a List of integer row ids, got {t}")
        if len(arr) != m:
            raise ValueError(f"candidates hold {len(arr)} lists, the queries have {m} rows")
        raw = np.asarray(arr.offsets.to_numpy(zero_copy_only=False), dtype=np.int64)
        lens = np.diff(raw)
        if arr.null_count:  # a null list is empty (whatever extent it has)
            valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
            lens = np.where(valid, lens, 0)
        lo, hi = (int(raw[0]), int(raw[-1])) if m else (0, 0)
        child = arr.values.slice(lo, hi - lo)
        null = np.asarray(child.is_null().to_numpy(zero_copy_only=False), dtype=bool) if child.null_count else None
        vals = (child.fill_null(0) if child.null_count else child).to_numpy(zero_copy_only=False)
        if int(lens.sum()) != vals.size:  # null lists with an extent: take the valid lists' values
            pos = np.repeat(raw[:-1] - lo, lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
            vals = vals[pos]
            null = null[pos] if null is not None else None
    rows = np.repeat(np.arange(m, dtype=np.int64), lens)
    bad = (vals >= n) if vals.dtype.kind == "u" else ((vals < 0) | (vals >= n))
    if null is not None:
        bad = bad | null
    if bad.any():
        at = int(np.argmax(bad))
        what = "null" if null is not None and null[at] else str(int(vals[at]))
        raise ValueError(f"candidates of row {int(rows[at])} hold the id {what}: "
                         f"not a row of the corpus ({n} rows)")
    # one pass over the (row, id) pairs: sorted by row, then id, duplicates dropped
    pairs = rows * np.int64(max(n, 1)) + vals.astype(np.int64)
    if pairs.size > 1 and not np.all(np.diff(pairs) > 0):
        pairs = np.unique(pairs)
        rows = pairs // np.int64(max(n, 1))
    offsets = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=m)[:m], out=offsets[1:])
    ids = np.ascontiguousarray(pairs - rows * np.int64(max(n, 1)), dtype=np.uint32)
    return _Candidates(offsets, ids)


def _candidates_union(cand: _Candidates):
    """(U, local): the sorted union of all listed ids and the lists renumbered
    by their place in it -- a monotone map, so order and ties are kept."""
    U = np.unique(cand.ids)
    return U, np.searchsorted(U, cand.ids).astype(np.uint32)


def _topk_candidates(q, c, original, rv, cand: _Candidates, kk: int, metric_id: int):
    """(idx (m, kk), scores f32 (m, kk), lens (m,)): row i's first lens[i]
    slots are its top-kk among its own candidates, indices numbering c.  On
    the cached f32 handle of the corpus when there is one of one shard (one
    GPU); else on a handle made for the call from the rows some list names
    (their sorted union), the lists renumbered into it and the result mapped
    back -- one search either way."""
    dc = None
    devs = _native.get_devices()
    if len(devs) <= 1:
        dc = _cached_corpus(original, rv, c, "f32")
        if dc is not None and dc.shards != 1:
            dc.release()
            dc = None
    if dc is not None:
        try:
            out = dc.topk_candidates(q, cand.offsets, cand.ids, kk, metric_id)
            _reaccount_cache(dc)
        finally:
            dc.release()
        return out
    U, local = _candidates_union(cand)
    rows = np.ascontiguousarray(c[U])
    if len(devs) > 1:
        # the entry takes a handle of one shard: made on the list's first device
        with _cache_lock:
            _native.set_devices(devs[:1])
            try:
                tmp = _native.DeviceCorpus(rows)
            finally:
                _native.set_devices(devs)
    else:
        tmp = _native.DeviceCorpus(rows)
    tmp.acquire()
    try:
        idx, sc, lens = tmp.topk_candidates(q, cand.offsets, local, kk, metric_id)
    finally:
        tmp.release()
        tmp.close()
    used = idx != 0xFFFFFFFF
    idx[used] = U[idx[used]]
    return idx, sc, lens


def _ragged_topk_arrow(idx: np.ndarray, scores: np.ndarray, lens: np.ndarray) -> pa.Array:
    """The lists' first lens[i] entries as LargeList<Struct>: no padding reaches Arrow."""
    keep = np.arange(idx.shape[1], dtype=np.int64)[None, :] < lens.astype(np.int64)[:, None]
    struct = pa.StructArray.from_arrays(
        [pa.array(idx[keep], type=pa.uint32()), pa.array(scores[keep].astype(np.float64, copy=False), type=pa.float64())],
        fields=list(_TOPK_STRUCT),
    )
    offsets = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return pa.LargeListArray.from_arrays(pa.array(offsets, type=pa.int64()), struct)


# ---------------------------------------------------------------------------
# Device list (multi-GPU through the drop-in: include/pmm.h pmm_set_devices).
# PMM_DEVICES = "all" or a comma list is applied on the first top-k call (not
# at import: counting devices initialises the HIP runtime).
# ---------------------------------------------------------------------------
_devices_env_done = False


def _parse_devices(spec: str, count: int):
    spec = spec.strip().lower()
    if spec in ("", "0-0"):
        return []
    if spec == "all":
        return list(range(count))
    return [int(x) for x in spec.split(",") if x.strip()]


def _apply_devices_env() -> None:
    global _devices_env_done
    if _devices_env_done:
        return
    _devices_env_done = True
    spec = os.environ.get("PMM_DEVICES")
    if spec:
        set_devices(_parse_devices(spec, _native.device_count()))


def set_devices(ids) -> None:
    """Row-shard the corpus of later top-k calls over these GPUs (results
    merged on the first, identical to one GPU's); [] = one GPU."""
    global _devices_env_done
    _devices_env_done = True  # an explicit choice overrides PMM_DEVICES
    _native.set_devices(list(ids))


def get_devices():
    return _native.get_devices()


# ---------------------------------------------------------------------------
# Output builders
# ---------------------------------------------------------------------------
_TOPK_STRUCT = pa.struct([("index", pa.uint32()), ("score", pa.float64())])


def _topk_arrow(idx: np.ndarray, scores: np.ndarray, m: int, k: int) -> pa.Array:
    struct = pa.StructArray.from_arrays(
        [pa.array(idx.reshape(-1), type=pa.uint32()), pa.array(scores.reshape(-1), type=pa.float64())],
        fields=list(_TOPK_STRUCT),
    )
    offsets = np.arange(m + 1, dtype=np.int64) * k
    return pa.LargeListArray.from_arrays(pa.array(offsets, type=pa.int64()), struct)


def _wrap(arrow_arr: pa.Array, name: str, polars_out: bool):
    if polars_out:
        return _pl.Series(name, arrow_arr)
    return arrow_arr


# ---------------------------------------------------------------------------
# Public extension functions
# ---------------------------------------------------------------------------
def _topk(left, right, k, metric, compute="f32", subset=None, groups=None, candidates=None):
    """src/lib.rs:33-55 -> src/matmul.rs:473-519 topk_impl.  compute="bf16"
    (an extension): both columns are read as f32 whatever their dtype and
    searched on the bf16 path (the numpy-level ``topk``'s compute="bf16").
    subset (an extension): search only the selected rows of ``right`` -- a
    Boolean Series / Arrow array / numpy mask of len(right) (nulls count as
    false) or integer row ids (sorted and de-duplicated here).  The returned
    ``index`` values number ``right``, k clips to the number of selected rows
    (the reference's clip-to-n rule on the searched rows), and an empty
    selection raises what an empty corpus raises.
    groups (an extension): ``(left_labels, right_labels)`` -- Series, Arrow
    arrays or numpy arrays of one hashable type (integers, strings,
    categoricals), one label per row of ``left`` and of ``right``.  Every query
    row is searched only among the corpus rows with its own label; a null label
    on either side matches nothing.  The lists are ragged: row i holds
    min(k, corpus rows of its label) entries, none when the corpus has no such
    label.  Not together with ``subset``.  ``left_labels`` holding one LIST of
    labels per row (an Arrow List / LargeList / FixedSizeList of the right
    side's label type, or a 2-D integer matrix) runs probed search: the row is
    searched in the union of its labels' corpus rows, ties to the lower corpus
    row; a null element or an unseen label is skipped, a null or empty list
    gives an empty result.
    candidates (an extension): one list of corpus row ids per row of ``left``
    -- a Series or Arrow List / LargeList of any integer type (a null list is
    empty), or a pair ``(offsets, ids)`` of numpy arrays.  Every query row is
    searched only among its own list (sorted and de-duplicated here); a null
    or negative id or one that is no row of ``right`` raises ValueError.  The
    lists are ragged: row i holds min(k, its candidates) entries, exact f32
    scores.  Float32 columns only; not together with ``subset`` or ``groups``."""
    k = _as_usize(k)
    if not isinstance(metric, str):
        raise TypeError(f"argument 'metric': '{type(metric).__name__}' object cannot be converted to 'PyString'")
    bf16 = _native.check_compute(compute) == "bf16"
    polars_out = _is_polars_series(left)
    t = time.perf_counter()
    lv = _to_arrow(left)
    rv = _to_arrow(right)
    if groups is not None and subset is not None:
        raise ValueError("groups= and subset= cannot be combined: give the rows to leave out a null label")
    cand = None
    if candidates is not None:
        if subset is not None or groups is not None:
            raise ValueError("candidates= cannot be combined with subset= or groups=: "
                             "leave the rows a query must not see out of its list")
        if bf16:
            raise _candidates_f32_only('compute="bf16" has no candidate search')
        if not (_is_f32(lv) and _is_f32(rv)):
            raise _candidates_f32_only("got a column of another type")
        cand = _check_candidates(candidates, _nrows(lv), _nrows(rv))
    sel = _check_subset(subset, _nrows(rv)) if subset is not None else None
    grp = _check_groups(groups, _nrows(lv), _nrows(rv)) if groups is not None else None
    if _nrows(lv) == 0:  # src/matmul.rs:480-487
        empty = pa.array([], type=pa.large_list(_TOPK_STRUCT))
        return _wrap(empty, "topk", polars_out)
    try:
        metric_id = _native.metric_from_str(metric)
    except _native.PmmError as e:  # src/metrics.rs:25 text
        raise _compute_error(str(e)) from None
    use_f32 = bf16 or (_is_f32(lv) and _is_f32(rv))  # src/matmul.rs:427
    dt = np.float32 if use_f32 else np.float64
    # Signed bytes on both sides (an extension in speed only): the reference
    # widens them to f64 (src/matmul.rs:143, :179) and so did this function;
    # the int8 route returns those bits from the int8 MFMA (pmm_topk_i8).
    # Everything else -- mixed dtypes, UInt8, wider integers, compute="bf16",
    # subset=, groups=, a device list -- keeps the f64 route.
    i8 = not bf16 and sel is None and grp is None and _is_i8(lv) and _is_i8(rv)
    if i8:
        dt = np.int8
    q = _series_to_matrix(lv, dt)
    c = _series_to_matrix(rv, dt)
    t = _lap("extract", t)
    if q.shape[1] != c.shape[1]:  # src/matmul.rs:433-441
        raise _dim_mismatch(q.shape[1], c.shape[1])
    kk = min(k, c.shape[0] if sel is None else sel.count)  # src/matmul.rs:443
    m = q.shape[0]
    if cand is not None:
        kk = min(k, cand.maxlen)  # the clip-to-n rule on the longest list
        if kk == 0:
            idx, sc = np.zeros((m, 0), dtype=np.uint32), np.zeros((m, 0), dtype=np.float64)
            lens = np.zeros(m, dtype=np.uint32)
        else:
            _apply_devices_env()
            idx, sc, lens = _topk_candidates(q, c, right, rv, cand, kk, metric_id)
            t = _lap("device", t)
        out = _wrap(_ragged_topk_arrow(idx, sc, lens), "topk", polars_out)
        _lap("assemble", t)
        return out
    if grp is not None:
        kk = min(k, grp.searched_max())  # the clip-to-n rule on the largest searched segment
        if kk == 0:
            idx, sc = np.zeros((m, 0), dtype=np.uint32), np.zeros((m, 0), dtype=np.float64)
            lens = np.zeros(m, dtype=np.uint32)
        else:
            _apply_devices_env()
            idx, sc, lens = _topk_grouped(q, c, right, rv, grp, kk, metric_id, compute)
            t = _lap("device", t)
        out = _wrap(_ragged_topk_arrow(idx, sc, lens), "topk", polars_out)
        _lap("assemble", t)
        return out
    if kk == 0:
        idx = np.zeros((m, 0), dtype=np.uint32)
        sc = np.zeros((m, 0), dtype=np.float64)
    elif sel is not None:
        _apply_devices_env()
        idx, sc = _topk_subset(q, c, right, rv, sel, kk, metric_id, compute)
        t = _lap("device", t)
        sc = sc.astype(np.float64, copy=False)
    else:
        _apply_devices_env()
        if i8 and len(_native.get_devices()) > 1:  # int8 rows are not sharded: the f64 route
            q, c, i8 = q.astype(np.float64), c.astype(np.float64), False
        # (an f32 or bf16 handle sharded over several GPUs serves k <= 1024;
        # larger k runs on one GPU, the device list's first.  An f64 handle is
        # sharded the same way and serves any k.)
        dc = (_cached_corpus(right, rv, c, compute)
              if (not use_f32 or kk <= 1024 or len(_native.get_devices()) <= 1) else None)
        if dc is not None:
            try:
                idx, sc = dc.topk(q, kk, metric_id)
                _reaccount_cache(dc)
            finally:
                dc.release()
        elif i8:
            idx, sc = _native.topk_i8_host(q, c, kk, metric_id)
        else:
            idx, sc = _native.topk_host(q, c, kk, metric_id,
                                        compute=_native.COMPUTE_BF16 if bf16 else _native.COMPUTE_F32)
        t = _lap("device", t)
        sc = sc.astype(np.float64, copy=False)  # src/matmul.rs:447 (f32 -> f64)
    out = _wrap(_topk_arrow(idx, sc, m, kk), "topk", polars_out)
    _lap("assemble", t)
    return out


# ---------------------------------------------------------------------------
# Late interaction (an extension; no reference counterpart): a row of either
# column is a LIST of token vectors, and the score of a (query, document) pair
# is MaxSim -- the sum over the query's tokens of the best pair score in the
# document (DeviceCorpus.topk_maxsim).  The documents column is cached as a
# multi-vector handle like any corpus; the lists go through ``candidates=``'s
# normaliser as they are.
# ---------------------------------------------------------------------------
_MAXSIM_SYNTH_MAX = 1 << 24  # candidates=None: the full lists are written out up to m * n_docs of this


def _maxsim_f32_only(what: str) -> TypeError:
    return TypeError(
        f"MaxSim search runs on Float32 token columns ({what}); cast the tokens first, e.g. "
        "pl.col('tokens').cast(pl.List(pl.Array(pl.Float32, d))) or array.astype(numpy.float32)"
    )


def _maxsim_metric(metric) -> int:
    """The metric id, without the library: cosine or dot."""
    if not isinstance(metric, str):
        raise TypeError(f"argument 'metric': '{type(metric).__name__}' object cannot be converted to 'PyString'")
    name = metric.lower()
    if name in ("euclidean", "l2"):
        raise ValueError("MaxSim takes metric 'cosine' or 'dot': a maximum over euclidean distances is not a similarity")
    if name == "cosine":
        return _native.METRIC_COSINE
    if name == "dot":
        return _native.METRIC_DOT
    raise ValueError(f"Unknown metric: {metric}. Use 'cosine' or 'dot'")


def _token_lists(obj, what: str, docs: bool):
    """(tokens float32 [T, d], offsets int64 [rows + 1], arrow array or None)
    of a multi-vector column: a pair ``(tokens, offsets)`` of numpy arrays, or
    a Series / Arrow List whose rows are Array[Float32, d] or List[Float32]
    lists of one width.  A null query row has no tokens; a null or empty
    document raises ValueError (docs=True)."""
    if isinstance(obj, (tuple, list)) and len(obj) == 2 and all(isinstance(x, np.ndarray) for x in obj):
        tokens, offsets = obj
        if tokens.ndim != 2:
            raise TypeError(f"{what}: expected a 2-D array of token vectors, got shape {tokens.shape}")
        if tokens.dtype != np.float32:
            raise _maxsim_f32_only(f"{what} hold {tokens.dtype} tokens")
        if offsets.dtype.kind not in "iu" or offsets.ndim != 1 or offsets.size < 1:
            raise TypeError(f"{what}: the offsets must be a 1-D integer array of rows + 1 entries")
        offsets = offsets.astype(np.int64)
        if offsets[0] != 0 or np.any(np.diff(offsets) < 0) or offsets[-1] != tokens.shape[0]:
            raise ValueError(f"{what}: the offsets must start at 0, not descend and end at len(tokens)")
        arr = None
    else:
        arr = obj
        if _is_polars_series(arr):
            arr = arr.rechunk().to_arrow()
        if isinstance(arr, pa.ChunkedArray):
            arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
        if not isinstance(arr, pa.Array):
            raise TypeError(f"{what} must be a Series or Arrow List of token vectors, or a pair (tokens, offsets) of "
                            f"numpy arrays, got {type(obj).__name__}")
        t = arr.type
        outer = pa.types.is_list(t) or pa.types.is_large_list(t)
        it = t.value_type if outer else None
        inner = outer and (pa.types.is_list(it) or pa.types.is_large_list(it) or pa.types.is_fixed_size_list(it))
        if not inner:
            raise TypeError(f"{what} must be a List of Array[Float32, d] or List[Float32] token vectors, got {t}")
        if it.value_type != pa.float32():
            raise _maxsim_f32_only(f"{what} hold {it.value_type} tokens")
        n = len(arr)
        raw = np.asarray(arr.offsets.to_numpy(zero_copy_only=False), dtype=np.int64)
        lens = np.diff(raw)
        if arr.null_count:
            valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
            if docs:
                raise ValueError(f"{what}: document {int(np.argmin(valid))} is null")
            lens = np.where(valid, lens, 0)
        lo, hi = (int(raw[0]), int(raw[-1])) if n else (0, 0)
        child = arr.values.slice(lo, hi - lo)  # the token vectors
        if pa.types.is_fixed_size_list(it):
            d = it.list_size
            vals = _values_numpy(child.values.slice(child.offset * d, len(child) * d), np.float32)
        else:
            craw = np.asarray(child.offsets.to_numpy(zero_copy_only=False), dtype=np.int64)
            widths = np.diff(craw)
            if child.null_count:
                raise ValueError(f"{what}: a token vector is null")
            d = int(widths[0]) if widths.size else 0
            if widths.size and np.any(widths != d):
                bad = int(np.argmax(widths != d))
                raise ValueError(f"{what}: token {bad} has width {int(widths[bad])}, the first token has {d}: "
                                 "every token vector must have one width")
            vals = _values_numpy(child.values.slice(int(craw[0]), int(craw[-1] - craw[0])), np.float32) if widths.size \
                else np.zeros(0, dtype=np.float32)
        tokens = np.ascontiguousarray(vals.reshape(len(child), d)) if d else np.zeros((0, 0), dtype=np.float32)
        if int(lens.sum()) != len(child):  # null rows with an extent: the valid rows' tokens
            pos = np.repeat(raw[:-1] - lo, lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
            tokens = np.ascontiguousarray(tokens[pos])
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
    if docs:
        lens = np.diff(offsets)
        if lens.size and np.any(lens == 0):
            raise ValueError(f"{what}: document {int(np.argmax(lens == 0))} is empty (a document needs a token)")
    return tokens, offsets, arr


def _maxsim_device(qt, qo, dt, do, original, rv, cand: _Candidates, kk: int, metric_id: int):
    """(idx (m, kk), scores f32 (m, kk), lens (m,)), indices numbering the
    documents.  On the cached multi-vector handle of the documents column when
    it is cacheable and fits; else on a handle made for the call from the
    documents some list names (their sorted union), the lists renumbered into
    it and the result mapped back -- one search either way."""
    dc = _cached_corpus(original, rv, dt, "maxsim", doc_offsets=do) if rv is not None else None
    if dc is not None:
        try:
            out = dc.topk_maxsim(qt, qo, cand.offsets, cand.ids, kk, metric_id)
            _reaccount_cache(dc)
        finally:
            dc.release()
        return out
    U, local = _candidates_union(cand)
    lens = (do[1:] - do[:-1])[U]
    uo = np.zeros(U.size + 1, dtype=np.int64)
    np.cumsum(lens, out=uo[1:])
    rows = np.repeat(do[:-1][U], lens) + (np.arange(int(uo[-1])) - np.repeat(uo[:-1], lens))
    tmp = _native.DeviceCorpus.multivector(np.ascontiguousarray(dt[rows]), uo)
    tmp.acquire()
    try:
        idx, sc, ln = tmp.topk_maxsim(qt, qo, cand.offsets, local, kk, metric_id)
    finally:
        tmp.release()
        tmp.close()
    used = idx != 0xFFFFFFFF
    idx[used] = U[idx[used]]
    return idx, sc, ln


def _maxsim_search(left, right, k, metric, candidates, compute):
    """The checks (all before any library call) and the search behind
    ``_topk_maxsim`` and ``polars_matmul.topk_maxsim``: (idx, f32 scores, lens,
    kk), or None for a query column without rows."""
    k = _as_usize(k)
    if compute is not None and compute != "f32":
        raise _maxsim_f32_only(f"compute={compute!r} has no MaxSim search")
    metric_id = _maxsim_metric(metric)
    qt, qo, _ = _token_lists(left, "the queries", False)
    dt, do, rv = _token_lists(right, "the documents", True)
    m, nd = qo.size - 1, do.size - 1
    if candidates is not None:
        cand = _check_candidates(candidates, m, nd)
    else:
        if m * nd > _MAXSIM_SYNTH_MAX:
            raise ValueError(f"candidates=None scores every document for every row: {m} rows x {nd} documents is more "
                             f"than {_MAXSIM_SYNTH_MAX} pairs; give candidates= (a first stage's hits per row)")
        cand = _Candidates(np.arange(m + 1, dtype=np.int64) * nd, np.tile(np.arange(nd, dtype=np.uint32), m))
    if m == 0:
        return None
    if nd == 0:
        raise _compute_error("Empty series")
    if qt.shape[0] and qt.shape[1] != dt.shape[1]:
        raise _dim_mismatch(qt.shape[1], dt.shape[1])
    if qt.shape[0] == 0:
        qt = np.zeros((0, dt.shape[1]), dtype=np.float32)
    kk = min(k, cand.maxlen)  # the clip-to-n rule on the longest list
    if kk == 0:
        return (np.zeros((m, 0), dtype=np.uint32), np.zeros((m, 0), dtype=np.float32), np.zeros(m, dtype=np.uint32), 0)
    _apply_devices_env()
    idx, sc, lens = _maxsim_device(qt, qo, dt, do, right, rv, cand, kk, metric_id)
    return idx, sc, lens, kk


def _topk_maxsim(left, right, k, metric="cosine", candidates=None, compute=None):
    """Late-interaction top-k (an extension): ``left`` and ``right`` are
    columns of token lists -- List[Array[Float32, d]] or List[List[Float32]]
    of one width (Series or Arrow), or pairs ``(tokens [T, d], offsets)`` of
    numpy arrays.  Row i of the result ranks the documents of its list
    (``candidates``, as ``_topk``'s: sorted and de-duplicated here; None means
    every document, while rows x documents stays within 2^24) by MaxSim(Q, D) =
    sum over the query's tokens of the max over the document's tokens of the
    cosine or dot pair score, exact f32: List[Struct{index: u32, score: f64}],
    ragged, min(k, listed documents) long; a query without tokens has an empty
    list.  Float32 only (Float64, Int8 and compute= raise TypeError); euclidean
    raises ValueError, as do a null or empty document and token vectors of
    more than one width -- all before any library call."""
    polars_out = _is_polars_series(left)
    t = time.perf_counter()
    r = _maxsim_search(left, right, k, metric, candidates, compute)
    if r is None:
        return _wrap(pa.array([], type=pa.large_list(_TOPK_STRUCT)), "topk_maxsim", polars_out)
    idx, sc, lens, _ = r
    t = _lap("device", t)
    out = _wrap(_ragged_topk_arrow(idx, sc, lens), "topk_maxsim", polars_out)
    _lap("assemble", t)
    return out


# ---------------------------------------------------------------------------
# Bit columns (an extension; no reference counterpart): the sign of every
# component packed one bit per dimension, searched by Hamming distance -- the
# cheap first stage whose survivors ``candidates=`` re-scores exactly.
# ---------------------------------------------------------------------------
def pack_sign(x) -> np.ndarray:
    """The sign bits of the rows of x, (rows, ceil(d / 8)) uint8: bit j of a
    row -- (byte[j >> 3] >> (j & 7)) & 1 -- is 1 iff x[j] > 0, so both zeros,
    negatives, -inf and NaN give 0; the bits from d up are 0.  The statement
    the device packing (pmm_pack_sign_device) is tested against."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise TypeError(f"expected a 2-D array of embeddings, got shape {x.shape}")
    return np.packbits(x > 0, axis=1, bitorder="little")


def _bits_only(what: str) -> TypeError:
    return TypeError(
        f"Hamming search runs on UInt8 columns of packed bits ({what}); make them with .pmm.sign_bits() / "
        "polars_matmul.pack_sign(array), or numpy.packbits(bits, axis=1, bitorder='little')"
    )


def _topk_hamming(left, right, k):
    """Exact Hamming top-k of two bit columns: List[u8] / Array[u8, w] or uint8
    matrices of w packed bytes a row (a null row reads as zeros).
    List[Struct{index: u32, score: f64}] per row of ``left``: the min(k,
    len(right)) rows of ``right`` of least distance popcount(l XOR r), ascending
    by (distance, index)."""
    k = _as_usize(k)
    polars_out = _is_polars_series(left)
    lv = _to_arrow(left)
    rv = _to_arrow(right)
    if not (_is_u8(lv) and _is_u8(rv)):
        t = [str(a.dtype if isinstance(a, np.ndarray) else a.type) for a in (lv, rv)]
        raise _bits_only(f"got {t[0]} and {t[1]}")
    if _nrows(lv) == 0:
        return _wrap(pa.array([], type=pa.large_list(_TOPK_STRUCT)), "topk_hamming", polars_out)
    q = _series_to_matrix(lv, np.uint8)
    c = _series_to_matrix(rv, np.uint8)
    if q.shape[1] != c.shape[1]:
        raise _dim_mismatch(q.shape[1], c.shape[1])
    kk = min(k, c.shape[0])
    m = q.shape[0]
    if kk == 0:
        idx, sc = np.zeros((m, 0), dtype=np.uint32), np.zeros((m, 0), dtype=np.float64)
    else:
        _apply_devices_env()
        dc = _cached_corpus(right, rv, c, "bits")
        if dc is not None:
            try:
                idx, sc = dc.topk(q, kk)
            finally:
                dc.release()
        else:
            idx, sc = _native.topk_bits_host(q, c, kk)
    return _wrap(_topk_arrow(idx, sc, m, kk), "topk_hamming", polars_out)


def _sign_bits(col):
    """A Float32 column's sign bits as Array[u8, ceil(d / 8)] (``pack_sign`` of
    its rows; a null row packs to zeros).  A column whose f32 handle is in the
    corpus cache (a ``topk`` corpus) is packed on the device from the resident
    rows (pmm_corpus_sign_bits) and only the bits come back; any other column
    is packed with NumPy.  The same bytes either way."""
    polars_out = _is_polars_series(col)
    v = _to_arrow(col)
    if not _is_f32(v):
        t = str(v.dtype if isinstance(v, np.ndarray) else v.type)
        raise TypeError(f"sign_bits takes a Float32 column (got {t}); cast the embeddings first, e.g. "
                        "pl.col('embedding').cast(pl.List(pl.Float32)) or array.astype(numpy.float32)")
    x = _series_to_matrix(v, np.float32)
    dc = _cache_hit(col, v, x) if len(_native.get_devices()) <= 1 else None  # (a sharded handle has no sign bits)
    if dc is not None:
        try:
            sb = dc.sign_bits()
            try:
                bits = sb.bit_rows()
            finally:
                sb.close()
        finally:
            dc.release()
    else:
        bits = pack_sign(x)
    out = pa.FixedSizeListArray.from_arrays(pa.array(bits.reshape(-1), type=pa.uint8()), bits.shape[1])
    return _wrap(out, "sign_bits", polars_out)


# ---------------------------------------------------------------------------
# within: range search (an extension; no reference counterpart).  Every corpus
# row whose score passes a threshold, per query row: ragged lists, best first.
# It runs on f32 handles only (include/pmm.h pmm_range_f32_corpus) -- the
# cached handle of the corpus, a derived one for ``subset=``, or a handle made
# for the call when the corpus is not cacheable.  There is no host path.
# ---------------------------------------------------------------------------
def _within_f32_only(what: str) -> TypeError:
    return TypeError(
        f"range search runs on Float32 columns ({what}); cast the embeddings first, e.g. "
        "pl.col('embedding').cast(pl.List(pl.Float32)) or array.astype(numpy.float32)"
    )


def _csr_arrow(offsets: np.ndarray, idx: np.ndarray, scores: np.ndarray) -> pa.Array:
    """LargeList<Struct{index: u32, score: f64}> straight from CSR arrays: row i
    is entries [offsets[i], offsets[i + 1]); the scores widen to f64 as ``_topk``'s."""
    struct = pa.StructArray.from_arrays(
        [pa.array(np.asarray(idx), type=pa.uint32()),
         pa.array(np.asarray(scores).astype(np.float64, copy=False), type=pa.float64())],
        fields=list(_TOPK_STRUCT),
    )
    return pa.LargeListArray.from_arrays(pa.array(np.asarray(offsets, dtype=np.int64), type=pa.int64()), struct)


def _within_device(q, c, original, rv, sel, threshold: float, metric_id: int, numpy_ok: bool = False):
    """(offsets, idx, scores f32) of the range search of q against c (both
    f32), or against its selected rows, indices numbering c.  With a device
    list the handle is sharded and the library's unsupported error surfaces."""
    parent_key = _corpus_key(original, rv, c, "f32", numpy_ok)
    parent = _cached_corpus(original, rv, c, "f32", numpy_ok) if parent_key is not None else None
    own_parent = parent is None
    if own_parent:
        parent = _native.DeviceCorpus(c).acquire()
    dc, transient = parent, False
    try:
        if sel is not None:
            if own_parent:
                dc, transient = parent.subset(sel.mask if sel.mask is not None else sel.ids).acquire(), True
            else:
                dc, transient = _cached_subset(parent, parent_key, sel, c, "f32")
                if dc is None:
                    raise _compute_error("the selected corpus rows do not fit in half of the free device memory")
        try:
            return dc.range(q, threshold, metric_id)
        finally:
            if dc is not parent:
                dc.release()
                if transient:
                    dc.close()
    finally:
        parent.release()
        if own_parent:
            parent.close()


def _within(left, right, threshold, metric, subset=None, compute="f32"):
    """Range search (an extension): for every row of ``left`` the rows of
    ``right`` whose score is >= ``threshold`` (cosine, dot) or <= ``threshold``
    (euclidean), as List[Struct{index: UInt32, score: Float64}] named "within",
    best first, ragged (a row without hits is an empty list).  The extraction,
    null and dimension rules and error texts are ``_topk``'s; ``subset`` as
    there.  Float32 columns only: Float64 columns and compute="bf16" raise
    TypeError."""
    if not isinstance(metric, str):
        raise TypeError(f"argument 'metric': '{type(metric).__name__}' object cannot be converted to 'PyString'")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise TypeError(f"threshold must be a number, not {type(threshold).__name__}")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    if _native.check_compute(compute) == "bf16":
        raise _within_f32_only('compute="bf16" has no range search')
    polars_out = _is_polars_series(left)
    lv = _to_arrow(left)
    rv = _to_arrow(right)
    if not (_is_f32(lv) and _is_f32(rv)):
        raise _within_f32_only("got a column of another type")
    sel = _check_subset(subset, _nrows(rv)) if subset is not None else None
    if _nrows(lv) == 0:
        return _wrap(pa.array([], type=pa.large_list(_TOPK_STRUCT)), "within", polars_out)
    try:
        metric_id = _native.metric_from_str(metric)
    except _native.PmmError as e:  # src/metrics.rs:25 text
        raise _compute_error(str(e)) from None
    q = _series_to_matrix(lv, np.float32)
    c = _series_to_matrix(rv, np.float32)
    if q.shape[1] != c.shape[1]:
        raise _dim_mismatch(q.shape[1], c.shape[1])
    _apply_devices_env()
    offsets, idx, sc = _within_device(q, c, right, rv, sel, threshold, metric_id)
    return _wrap(_csr_arrow(offsets, idx, sc), "within", polars_out)


# ---------------------------------------------------------------------------
# Self search (an extension; no reference counterpart): one column against
# itself -- near-duplicate pairs (``_within_self``) and the k-nearest-neighbour
# graph of its rows (``_topk_self``).  The column's cached f32 handle is its
# own query side (include/pmm.h pmm_range_f32_self, pmm_topk_f32_self): nothing
# but the corpus is uploaded, and that once.
# ---------------------------------------------------------------------------
def _self_f32_only(what: str) -> TypeError:
    return TypeError(
        f"self search runs on Float32 columns ({what}); cast the embeddings first, e.g. "
        "pl.col('embedding').cast(pl.List(pl.Float32)) or array.astype(numpy.float32)"
    )


def _self_device(c, original, rv, run, numpy_ok: bool = False):
    """``run(handle)`` on the cached f32 handle of c, or on one made for the
    call when c is not cacheable.  With a device list the handle is sharded and
    the library's unsupported error surfaces."""
    dc = _cached_corpus(original, rv, c, "f32", numpy_ok)
    own = dc is None
    if own:
        dc = _native.DeviceCorpus(c).acquire()
    try:
        out = run(dc)
        if not own:
            _reaccount_cache(dc)
        return out
    finally:
        dc.release()
        if own:
            dc.close()


def _self_column(col, metric):
    """(polars_out, arrow column) of a self entry's Float32 column."""
    if not isinstance(metric, str):
        raise TypeError(f"argument 'metric': '{type(metric).__name__}' object cannot be converted to 'PyString'")
    polars_out = _is_polars_series(col)
    rv = _to_arrow(col)
    if not _is_f32(rv):
        raise _self_f32_only("got a column of another type")
    return polars_out, rv


def _self_metric(metric: str) -> int:
    try:
        return _native.metric_from_str(metric)
    except _native.PmmError as e:  # src/metrics.rs:25 text
        raise _compute_error(str(e)) from None


def _within_self(col, threshold, metric):
    """Self range search (an extension): for every row i of ``col`` the rows
    j > i whose score with it is >= ``threshold`` (cosine, dot) or <=
    ``threshold`` (euclidean), as List[Struct{index: UInt32, score: Float64}]
    named "within_self", best first, ragged: ``_within(col, col, ...)`` with
    each pair kept once, under its lower row, and no row paired with itself.
    (The dropped (j, i) has the same score bits, for every metric.)  Float32
    columns only."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise TypeError(f"threshold must be a number, not {type(threshold).__name__}")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    polars_out, rv = _self_column(col, metric)
    if _nrows(rv) == 0:
        return _wrap(pa.array([], type=pa.large_list(_TOPK_STRUCT)), "within_self", polars_out)
    metric_id = _self_metric(metric)
    c = _series_to_matrix(rv, np.float32)
    _apply_devices_env()
    offsets, idx, sc = _self_device(c, col, rv, lambda dc: dc.range_self(threshold, metric_id))
    return _wrap(_csr_arrow(offsets, idx, sc), "within_self", polars_out)


def _duplicate_groups(col, threshold, metric):
    """Duplicate groups (an extension): the connected components of
    ``_within_self(col, threshold, metric)``'s pairs, as a UInt32 column named
    "duplicate_groups": every row carries the number of the first row of its
    group, and a row with no near-duplicate its own.  The pairs are united on
    the device where they are found, so no pair list is built: the memory of
    the call does not grow with the number of duplicates.  Float32 columns
    only."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise TypeError(f"threshold must be a number, not {type(threshold).__name__}")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    polars_out, rv = _self_column(col, metric)
    if _nrows(rv) == 0:
        return _wrap(pa.array([], type=pa.uint32()), "duplicate_groups", polars_out)
    metric_id = _self_metric(metric)
    c = _series_to_matrix(rv, np.float32)
    _apply_devices_env()
    labels = _self_device(c, col, rv, lambda dc: dc.components_self(threshold, metric_id))[0]
    return _wrap(pa.array(labels, type=pa.uint32()), "duplicate_groups", polars_out)


def _topk_self(col, k, metric):
    """Self top-k (an extension): for every row of ``col`` its min(k, n - 1)
    best OTHER rows, as List[Struct{index: UInt32, score: Float64}] named
    "topk_self": the row's ranked list of the whole column without the row
    itself -- so an exact duplicate stays, whichever of the two has the lower
    row number.  A column of one row gives one empty list.  Float32 columns
    only."""
    k = _as_usize(k)
    polars_out, rv = _self_column(col, metric)
    n = _nrows(rv)
    if n == 0:
        return _wrap(pa.array([], type=pa.large_list(_TOPK_STRUCT)), "topk_self", polars_out)
    metric_id = _self_metric(metric)
    c = _series_to_matrix(rv, np.float32)
    _apply_devices_env()
    idx, sc = _self_device(c, col, rv, lambda dc: dc.topk_self(k, metric_id))
    return _wrap(_topk_arrow(idx, sc.astype(np.float64), n, idx.shape[1]), "topk_self", polars_out)


# ---------------------------------------------------------------------------
# k-means (an extension; no reference counterpart): Lloyd's iteration on one
# Float32 column, on its cached f32 handle (include/pmm.h
# pmm_kmeans_f32_corpus).  The labels feed ``corpus_by=`` and the centroids
# ``.pmm.topk(centroids, nprobe)``: the coarse quantiser of a grouped search.
# ---------------------------------------------------------------------------
def _kmeans_f32_only(what: str) -> TypeError:
    return TypeError(
        f"k-means runs on Float32 columns ({what}); cast the embeddings first, e.g. "
        "pl.col('embedding').cast(pl.List(pl.Float32)) or array.astype(numpy.float32)"
    )


def _kmeans_metric(metric) -> int:
    """The metric id, without the library: euclidean or cosine."""
    if not isinstance(metric, str):
        raise TypeError(f"argument 'metric': '{type(metric).__name__}' object cannot be converted to 'PyString'")
    name = metric.lower()
    if name == "dot":
        raise ValueError("k-means takes metric 'euclidean' or 'cosine': a mean does not maximise a dot product")
    if name in ("euclidean", "l2"):
        return _native.METRIC_EUCLIDEAN
    if name == "cosine":
        return _native.METRIC_COSINE
    raise ValueError(f"Unknown metric: {metric}. Use 'euclidean' or 'cosine'")


def _kmeans_init(c: np.ndarray, K: int, init, seed) -> np.ndarray:
    """The K x d float32 initial centroids: ``init`` as a [K, d] matrix, as K
    distinct row ids of c, or None -- the rows
    ``np.sort(np.random.RandomState(seed).choice(n, K, replace=False))``."""
    n, d = c.shape
    if init is None:
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise TypeError(f"seed must be an integer, not {type(seed).__name__}")
        ids = np.sort(np.random.RandomState(int(seed)).choice(n, K, replace=False))
        return np.ascontiguousarray(c[ids])
    a = np.asarray(init)
    if a.ndim == 2:
        if a.dtype.kind != "f":
            raise TypeError(f"init as a matrix must hold floats, got {a.dtype}")
        if a.shape != (K, d):
            raise ValueError(f"init has shape {a.shape}, n_clusters={K} centroids of dimension {d} need ({K}, {d})")
        return np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim == 1 and a.dtype.kind in "iu":
        if a.shape[0] != K:
            raise ValueError(f"init holds {a.shape[0]} row ids, n_clusters is {K}")
        ids = a.astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            bad = int(ids[(ids < 0) | (ids >= n)][0])
            raise ValueError(f"init holds the row id {bad}: not a row of the column ({n} rows)")
        if np.unique(ids).size != K:
            raise ValueError("init holds a row id twice: the initial centroids must be distinct rows")
        return np.ascontiguousarray(c[ids])
    raise TypeError("init must be a [n_clusters, d] float matrix, a 1-D integer array of n_clusters distinct row ids, "
                    "or None")


def _kmeans_search(c, original, rv, n_clusters, metric, max_iter, init, seed, compute, numpy_ok=False):
    """The checks (all before any library call) and the call behind ``_kmeans``
    and ``polars_matmul.kmeans`` on the (n, d) float32 matrix c: (centroids,
    labels, scores float32, updates, converged)."""
    if compute is not None and compute != "f32":
        raise _kmeans_f32_only(f"compute={compute!r} has no k-means")
    metric_id = _kmeans_metric(metric)
    K = _as_usize(n_clusters)
    max_iter = _as_usize(max_iter)
    n = c.shape[0]
    if K < 1:
        raise ValueError("n_clusters must be >= 1")
    if K > n:
        raise ValueError(f"n_clusters ({K}) must be <= the rows of the column ({n})")
    c0 = _kmeans_init(c, K, init, seed)
    _apply_devices_env()
    return _self_device(c, original, rv, lambda dc: dc.kmeans(c0, metric_id, max_iter), numpy_ok)


def _kmeans_column(col):
    """(polars_out, arrow column, matrix) of a k-means Float32 column."""
    polars_out = _is_polars_series(col)
    rv = _to_arrow(col)
    if not _is_f32(rv):
        raise _kmeans_f32_only("got a column of another type")
    return polars_out, rv, _series_to_matrix(rv, np.float32)


def _kmeans(col, n_clusters, metric="euclidean", max_iter=25, init=None, seed=0, compute=None):
    """k-means (an extension) of a Float32 column (Series, Arrow or numpy
    matrix): Lloyd's iteration from ``init`` -- a [n_clusters, d] matrix, an
    array of n_clusters distinct row ids, or None for
    ``np.sort(np.random.RandomState(seed).choice(n, n_clusters, replace=False))``
    -- for at most ``max_iter`` updates, stopped early once an assignment
    repeats the previous labels.  Returns (centroids float32 [K, d], labels
    uint32 [n], scores float32 [n], updates, converged): the labels and scores
    are the exact f32 top-1 of every row among the returned centroids, ties to
    the lower centroid; a row whose best score is NaN has the label 0xFFFFFFFF.
    The update is an ordered f64 sum (include/pmm.h), so the result is
    reproducible bit for bit.  euclidean or cosine (spherical k-means: the mean
    of the members' unit vectors); dot raises ValueError.  Float32 only
    (Float64, Int8 and compute= raise TypeError).  The column's cached f32
    handle is used, under ``_topk``'s key: a column that is already a cached
    corpus is not uploaded again."""
    _, rv, c = _kmeans_column(col)
    return _kmeans_search(c, col, rv, n_clusters, metric, max_iter, init, seed, compute)


def _kmeans_labels(col, n_clusters, metric="euclidean", max_iter=25, init=None, seed=0, compute=None):
    """``_kmeans``'s labels as a UInt32 column named "kmeans"; a row in no
    cluster (label 0xFFFFFFFF) is null."""
    polars_out, rv, c = _kmeans_column(col)
    labels = _kmeans_search(c, col, rv, n_clusters, metric, max_iter, init, seed, compute)[1]
    none = labels == _native.NO_GROUP
    arr = pa.array(labels, type=pa.uint32(), mask=none if none.any() else None)
    return _wrap(arr, "kmeans", polars_out)


def _matmul(left, right):
    """src/lib.rs:15-30 -> src/matmul.rs:295-417 matmul_impl."""
    polars_out = _is_polars_series(left)
    t = time.perf_counter()
    lv = _to_arrow(left)
    rv = _to_arrow(right)
    use_f32 = _is_f32(lv) and _is_f32(rv)  # src/matmul.rs:298, :308
    dt = np.float32 if use_f32 else np.float64
    pa_t = pa.float32() if use_f32 else pa.float64()
    if _nrows(lv) == 0:  # src/matmul.rs:297-305: empty List (not Array)
        return _wrap(pa.array([], type=pa.large_list(pa_t)), "matmul", polars_out)
    q = _series_to_matrix(lv, dt)
    c = _series_to_matrix(rv, dt)
    t = _lap("extract", t)
    if q.shape[1] != c.shape[1]:
        raise _dim_mismatch(q.shape[1], c.shape[1])
    out = _native.matmul_host(q, c)
    t = _lap("device", t)
    n = c.shape[0]
    arr = pa.FixedSizeListArray.from_arrays(pa.array(out.reshape(-1), type=pa_t), n)
    res = _wrap(arr, "matmul", polars_out)
    _lap("assemble", t)
    return res


__all__ = ["_matmul", "_topk", "_within", "PanicException", "clear_corpus_cache", "set_devices", "get_devices"]
