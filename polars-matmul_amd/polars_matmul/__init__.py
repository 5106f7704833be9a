"""
polars-matmul (MI355X-native): similarity search for Polars embedding columns.

Drop-in for the reference package ``polars_matmul`` (NivekNey/polars-matmul
v0.1.4): importing it registers the ``pmm`` expression namespace on Polars
(python/polars_matmul/__init__.py:39 in the reference) with the same
``topk(corpus, k, metric)`` and ``matmul(corpus, flatten)`` methods, result
dtypes and errors.  An extension: ``.pmm.topk(corpus, k, metric,
compute="bf16")`` (and ``_topk(..., compute="bf16")``) reads both columns as
f32 and searches them on the bf16 MFMA path; the corpus stays on the device
as a bf16 handle (half an f32 handle's HBM) while its Series is reused.
``subset=`` (an extension, on all three) searches only the selected corpus rows
-- a Boolean mask Series or integer row ids -- from a handle derived on the
device, and returns indices that number the full corpus.  ``groups=`` (an
extension; ``by=`` / ``corpus_by=`` on the namespace) searches every query row
only among the corpus rows that carry its own label, all labels in one call
against a handle whose rows are stored group by group.  ``candidates=`` (an
extension, on all three) gives every query row its own list of corpus row ids
-- the second stage of a hybrid or two-stage search -- and searches all rows in
one call, exact f32 scores, on Float32 columns.  ``.pmm.within(corpus,
threshold, metric)`` (an extension; ``within`` / ``_within`` without Polars) is
range search: every corpus row whose score passes the threshold, as ragged
lists, on Float32 columns.  ``.pmm.within_self(threshold, metric)`` and
``.pmm.topk_self(k, metric)`` (extensions; ``within_self`` / ``topk_self`` and
``_within_self`` / ``_topk_self`` without Polars) search one column against
itself -- every near-duplicate pair once, and the k-nearest-neighbour graph of
its rows -- with the column's cached handle as its own query side;
``.pmm.duplicate_groups(threshold, metric)`` (``duplicate_groups`` /
``_duplicate_groups`` without Polars) labels every row with the first row of
its near-duplicate group, the pairs united on the device, none stored.
``.pmm.topk_maxsim(docs, k, metric, candidates=)`` (an extension;
``topk_maxsim`` / ``_topk_maxsim`` without Polars) is late-interaction search:
both columns hold lists of token vectors and a pair scores MaxSim, the sum
over the query's tokens of the best pair score in the document.
``.pmm.kmeans(n_clusters, metric, max_iter, init=, seed=)`` (an extension;
``kmeans`` / ``_kmeans`` without Polars) clusters one Float32 column on its
cached handle -- Lloyd's iteration, euclidean or spherical -- into the labels
that ``corpus_by=`` takes and the centroids that ``.pmm.topk`` probes.  The
numerics run on MI355X through hand-written HIP
kernels (``libpmm.so``, C ABI in ``include/pmm.h``); there is no CPU path.

Usage:
    >>> import polars as pl
    >>> import polars_matmul  # registers the .pmm namespace
    >>> queries.with_columns(pl.col("embedding").pmm.topk(corpus["embedding"], k=2))

Without Polars, the same extension functions accept pyarrow arrays or numpy
matrices (``polars_matmul._polars_matmul._topk``), and ``topk`` / ``matmul``
below are numpy-level conveniences.

Multi-GPU (an extension; the reference is single-process): ``set_devices([0,
1, ..., 7])`` -- or ``PMM_DEVICES=all`` / ``PMM_DEVICES=0,1,2,3`` in the
environment -- row-shards the corpus of every later ``.pmm.topk`` over those
GPUs inside the one Polars process and merges the per-GPU lists on the first
(include/pmm.h ``pmm_set_devices``); results are identical to one GPU's.
"""
from __future__ import annotations

from typing import Literal

import numpy as np

from polars_matmul._polars_matmul import (  # noqa: F401
    PanicException,
    _check_groups,
    _check_subset,
    _kmeans,
    _kmeans_labels,
    _matmul,
    _topk,
    _topk_self,
    _topk_maxsim,
    _within,
    _within_self,
    _duplicate_groups,
    _sign_bits,
    _topk_hamming,
    pack_sign,
    get_devices,
    set_devices,
)
from polars_matmul import _native

__version__ = "0.1.4"
__all__ = ["PmmNamespace", "topk", "topk_maxsim", "within", "within_self", "topk_self", "duplicate_groups", "matmul",
           "set_devices", "get_devices", "pack_sign", "topk_hamming", "kmeans"]

Metric = Literal["cosine", "dot", "euclidean"]
Compute = Literal["f32", "bf16"]

try:
    import polars as pl  # type: ignore
except Exception:  # polars is optional (not installable in this image)
    pl = None


def topk(queries: np.ndarray, corpus: np.ndarray, k: int, metric: Metric = "cosine",
         compute: Compute = "f32", subset=None, groups=None, candidates=None):
    """numpy-level top-k: returns (indices uint32 [m, k'], scores float64 [m, k'])
    with k' = min(k, len(corpus)); f32 compute iff both inputs are float32
    (src/matmul.rs:427), scores widened to f64 (src/matmul.rs:447).
    compute="bf16" (an extension, not in the reference): f32 inputs rounded to
    bf16 on the device, bf16 MFMA with f32 accumulation (include/pmm.h
    PMM_COMPUTE_BF16: the bf16 kernels up to d = 768 and k = 960, the rounded
    rows widened to f32 beyond).
    subset (an extension): a bool mask of len(corpus) or integer row ids; only
    those rows are searched (taken on the host: a numpy corpus has no cached
    handle), k' = min(k, rows selected), and the indices number ``corpus``.
    groups (an extension): ``(query_labels, corpus_labels)``, one label per
    row; every query is searched only among the corpus rows of its own label
    (per label on the host rows: a numpy corpus has no cached handle).
    k' = min(k, largest searched segment); a row whose segment is shorter (or
    empty: a null or unseen label) ends in unused slots -- index 0xFFFFFFFF,
    score NaN.  Not together with ``subset``.  ``query_labels`` as a 2-D
    integer matrix [m, P] or an Arrow List array gives every query a LIST of
    labels (probed search): it is searched in the union of those labels' rows,
    ties to the lower corpus row; k' = min(k, largest searched union).
    candidates (an extension): one list of corpus row ids per query row, as an
    Arrow List array or a pair ``(offsets, ids)`` of numpy arrays; every query
    is searched only among its own list, all rows in one call.  float32
    inputs only.  k' = min(k, longest list); a shorter list ends in unused
    slots -- index 0xFFFFFFFF, score NaN.  Not together with ``subset`` or
    ``groups``."""
    q = np.asarray(queries)
    c = np.asarray(corpus)
    _native.check_compute(compute)
    if candidates is not None:
        from polars_matmul._polars_matmul import _candidates_f32_only, _check_candidates, _topk_candidates

        if subset is not None or groups is not None:
            raise ValueError("candidates= cannot be combined with subset= or groups=: "
                             "leave the rows a query must not see out of its list")
        if compute == "bf16":
            raise _candidates_f32_only('compute="bf16" has no candidate search')
        if q.dtype != np.float32 or c.dtype != np.float32:
            raise _candidates_f32_only(f"got {q.dtype} queries and a {c.dtype} corpus")
        if q.ndim != 2 or c.ndim != 2:
            raise TypeError(f"expected 2-D arrays of embeddings, got shapes {q.shape} and {c.shape}")
        cand = _check_candidates(candidates, q.shape[0], c.shape[0])
        if q.shape[1] != c.shape[1]:
            raise RuntimeError(
                f"Dimension mismatch: left has {q.shape[1]} dimensional vectors, "
                f"right has {c.shape[1]} dimensional vectors"
            )
        kk = min(int(k), cand.maxlen)
        if kk <= 0 or q.shape[0] == 0:
            return np.zeros((q.shape[0], 0), dtype=np.uint32), np.zeros((q.shape[0], 0), dtype=np.float64)
        cc = np.ascontiguousarray(c)
        idx, sc, lens = _topk_candidates(np.ascontiguousarray(q), cc, None, cc, cand, kk,
                                         _native.metric_from_str(metric))
        sc = sc.astype(np.float64)
        sc[np.arange(kk)[None, :] >= lens[:, None].astype(np.int64)] = np.nan
        return idx, sc
    if groups is not None:
        if subset is not None:
            raise ValueError("groups= and subset= cannot be combined: give the rows to leave out a null label")
        grp = _check_groups(groups, q.shape[0], c.shape[0])
    if (q.dtype == np.int8 and c.dtype == np.int8 and compute == "f32" and subset is None and groups is None
            and q.ndim == 2 and c.ndim == 2 and len(_native.get_devices()) <= 1):
        # signed bytes on both sides: the int8 MFMA, the f64 route's bits (pmm_topk_i8)
        if q.shape[1] != c.shape[1]:
            raise RuntimeError(
                f"Dimension mismatch: left has {q.shape[1]} dimensional vectors, "
                f"right has {c.shape[1]} dimensional vectors"
            )
        return _native.topk_i8_host(q, c, min(int(k), c.shape[0]), _native.metric_from_str(metric))
    dt = np.float32 if (q.dtype == np.float32 and c.dtype == np.float32) else np.float64
    if compute == "bf16":
        dt = np.float32
    q = np.ascontiguousarray(q, dtype=dt)
    c = np.ascontiguousarray(c, dtype=dt)
    if q.shape[1] != c.shape[1]:
        raise RuntimeError(
            f"Dimension mismatch: left has {q.shape[1]} dimensional vectors, "
            f"right has {c.shape[1]} dimensional vectors"
        )
    if groups is not None:
        from polars_matmul._polars_matmul import _topk_grouped

        kk = min(int(k), grp.searched_max())
        if kk == 0:
            return np.zeros((q.shape[0], 0), dtype=np.uint32), np.zeros((q.shape[0], 0), dtype=np.float64)
        idx, sc, lens = _topk_grouped(q, c, None, c, grp, kk, _native.metric_from_str(metric), compute)
        sc = sc.astype(np.float64)
        sc[np.arange(kk)[None, :] >= lens[:, None].astype(np.int64)] = np.nan
        return idx, sc
    ids = _check_subset(subset, c.shape[0]).row_ids() if subset is not None else None
    if ids is not None:
        c = np.ascontiguousarray(c[ids])
    kk = min(int(k), c.shape[0])
    mode = _native.COMPUTE_BF16 if compute == "bf16" else _native.COMPUTE_F32
    idx, sc = _native.topk_host(q, c, kk, _native.metric_from_str(metric), compute=mode)
    if ids is not None:
        idx = ids[idx]
    return idx, sc.astype(np.float64, copy=False)


def topk_maxsim(queries, docs, k: int, metric: Metric = "cosine", candidates=None):
    """numpy-level late-interaction top-k (an extension): ``queries`` and
    ``docs`` are pairs ``(tokens float32 [T, d], offsets [rows + 1])`` -- row i
    holds the token vectors ``tokens[offsets[i]:offsets[i + 1]]`` (Arrow
    columns of token lists work too).  Every query is searched among the
    documents of its list (``candidates`` as in ``topk``; None: every
    document, while rows x documents stays within 2^24) by MaxSim = the sum
    over its tokens of the best cosine or dot pair score in the document.
    Returns (indices uint32 [m, k'], scores float64 [m, k']), k' = min(k,
    longest list); a shorter list ends in unused slots -- index 0xFFFFFFFF,
    score NaN.  float32 only; euclidean raises ValueError."""
    from polars_matmul._polars_matmul import _maxsim_search

    r = _maxsim_search(queries, docs, k, metric, candidates, None)
    if r is None:
        return np.zeros((0, 0), dtype=np.uint32), np.zeros((0, 0), dtype=np.float64)
    idx, sc, lens, kk = r
    sc = sc.astype(np.float64)
    sc[np.arange(kk)[None, :] >= lens[:, None].astype(np.int64)] = np.nan
    return idx, sc


def topk_hamming(queries_u8: np.ndarray, corpus_u8: np.ndarray, k: int):
    """numpy-level exact Hamming top-k (an extension) of packed bit rows --
    (m, w) and (n, w) uint8, ``pack_sign``'s output: (indices uint32 [m, k'],
    scores float64 [m, k']), k' = min(k, n), the integer distances
    popcount(q XOR c), least first, ties to the lower index.  A numpy corpus
    has no cached handle (as in ``topk``); ``_topk_hamming`` on an Arrow or
    Polars column searches the cached bit handle of the corpus."""
    from polars_matmul._polars_matmul import _bits_only

    q, c = np.asarray(queries_u8), np.asarray(corpus_u8)
    if q.dtype != np.uint8 or c.dtype != np.uint8:
        raise _bits_only(f"got {q.dtype} queries and a {c.dtype} corpus")
    if q.ndim != 2 or c.ndim != 2:
        raise TypeError(f"expected 2-D arrays of packed bits, got shapes {q.shape} and {c.shape}")
    if q.shape[1] != c.shape[1]:
        raise RuntimeError(
            f"Dimension mismatch: left has {q.shape[1]} dimensional vectors, "
            f"right has {c.shape[1]} dimensional vectors"
        )
    kk = min(int(k), c.shape[0])
    if kk <= 0 or q.shape[0] == 0:
        return np.zeros((q.shape[0], 0), dtype=np.uint32), np.zeros((q.shape[0], 0), dtype=np.float64)
    return _native.topk_bits_host(q, np.ascontiguousarray(c), kk)


def within(queries: np.ndarray, corpus: np.ndarray, threshold: float, metric: Metric = "cosine", subset=None,
           compute: Compute = "f32"):
    """numpy-level range search (an extension): every corpus row whose score
    is >= ``threshold`` (cosine, dot) or <= ``threshold`` (euclidean), per query
    row.  Returns CSR arrays (offsets int64 [m + 1], indices uint32 [total],
    scores float64 [total]): row i's hits are entries [offsets[i],
    offsets[i + 1]), best first, the f32 scores widened as ``topk``'s.
    Float32 matrices only (Float64 input and compute="bf16" raise TypeError).
    The corpus goes through the corpus cache: a C-contiguous float32 matrix of
    at least 1 MiB is uploaded once and found again by its address while the
    cache holds it (do not write to it in place meanwhile;
    ``_polars_matmul.clear_corpus_cache()`` forgets it).
    subset: a bool mask of len(corpus) or integer row ids; only those rows are
    searched, from a handle derived on the device, and the indices number
    ``corpus``."""
    from polars_matmul._polars_matmul import _within_device, _within_f32_only

    q = np.asarray(queries)
    c = np.asarray(corpus)
    if _native.check_compute(compute) == "bf16":
        raise _within_f32_only('compute="bf16" has no range search')
    if q.dtype != np.float32 or c.dtype != np.float32:
        raise _within_f32_only(f"got {q.dtype} queries and a {c.dtype} corpus")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    if q.ndim != 2 or c.ndim != 2:
        raise TypeError(f"expected 2-D arrays of embeddings, got shapes {q.shape} and {c.shape}")
    if q.shape[1] != c.shape[1]:
        raise RuntimeError(
            f"Dimension mismatch: left has {q.shape[1]} dimensional vectors, "
            f"right has {c.shape[1]} dimensional vectors"
        )
    sel = _check_subset(subset, c.shape[0]) if subset is not None else None
    metric_id = _native.metric_from_str(metric)
    if q.shape[0] == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float64)
    if c.shape[0] == 0:
        raise RuntimeError("Empty series")
    cc = np.ascontiguousarray(c)
    # (cached only when the caller's own matrix is what is uploaded: a copy
    # made here would never be found again)
    offsets, idx, sc = _within_device(np.ascontiguousarray(q), cc, cc, cc, sel, threshold, metric_id,
                                      numpy_ok=cc is corpus)
    return offsets, idx, sc.astype(np.float64)


def _self_matrix(corpus) -> np.ndarray:
    from polars_matmul._polars_matmul import _self_f32_only

    c = np.asarray(corpus)
    if c.dtype != np.float32:
        raise _self_f32_only(f"got a {c.dtype} matrix")
    if c.ndim != 2:
        raise TypeError(f"expected a 2-D array of embeddings, got shape {c.shape}")
    return c


def within_self(corpus: np.ndarray, threshold: float, metric: Metric = "cosine", compute: Compute = "f32"):
    """numpy-level self range search (an extension): the near-duplicate pairs
    of one matrix.  Returns CSR arrays (offsets int64 [n + 1], indices uint32
    [total], scores float64 [total]): row i's entries are ``within(corpus,
    corpus, ...)``'s for row i without those at j <= i -- each pair once, under
    its lower row, never a row with itself -- same scores, best first.  (The
    dropped (j, i) has the same score bits as the kept (i, j), for every
    metric.)  The rows are uploaded once, as the cached handle, and are their
    own queries.  Float32 matrices only (Float64 input and compute="bf16" raise
    TypeError); the corpus cache as in ``within``."""
    from polars_matmul._polars_matmul import _self_device, _self_f32_only

    if _native.check_compute(compute) == "bf16":
        raise _self_f32_only('compute="bf16" has no self search')
    c = _self_matrix(corpus)
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    metric_id = _native.metric_from_str(metric)
    if c.shape[0] == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float64)
    cc = np.ascontiguousarray(c)
    offsets, idx, sc = _self_device(cc, cc, cc, lambda dc: dc.range_self(threshold, metric_id),
                                    numpy_ok=cc is corpus)
    return offsets, idx, sc.astype(np.float64)


def duplicate_groups(corpus: np.ndarray, threshold: float, metric: Metric = "cosine", compute: Compute = "f32"):
    """numpy-level duplicate groups (an extension): labels uint32 [n], the
    connected components of ``within_self(corpus, threshold, metric)``'s pairs.
    ``labels[i]`` is the smallest row number in row i's group; a row with no
    near-duplicate labels itself, so ``labels == arange(n)`` marks the one row
    to keep of every group.  The pairs are united on the device where they are
    found: no pair list is built, and the memory of the call does not grow
    with the number of duplicates.  Float32 matrices only (Float64 input and
    compute="bf16" raise TypeError); the corpus cache as in ``within``."""
    from polars_matmul._polars_matmul import _self_device, _self_f32_only

    if _native.check_compute(compute) == "bf16":
        raise _self_f32_only('compute="bf16" has no self search')
    c = _self_matrix(corpus)
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    metric_id = _native.metric_from_str(metric)
    if c.shape[0] == 0:
        return np.zeros(0, dtype=np.uint32)
    cc = np.ascontiguousarray(c)
    return _self_device(cc, cc, cc, lambda dc: dc.components_self(threshold, metric_id), numpy_ok=cc is corpus)[0]


def topk_self(corpus: np.ndarray, k: int, metric: Metric = "cosine", compute: Compute = "f32"):
    """numpy-level self top-k (an extension): the k-nearest-neighbour graph of
    one matrix.  Returns (indices uint32 [n, k'], scores float64 [n, k']) with
    k' = min(k, n - 1): row i's ranked list of all rows without row i itself --
    not ``topk(corpus, corpus, k + 1)`` minus rank 0, which drops the wrong
    entry when an exact duplicate with a lower row number ties with the row.
    Float32 matrices only; the corpus cache as in ``within``."""
    from polars_matmul._polars_matmul import _self_device, _self_f32_only

    if _native.check_compute(compute) == "bf16":
        raise _self_f32_only('compute="bf16" has no self search')
    c = _self_matrix(corpus)
    metric_id = _native.metric_from_str(metric)
    if c.shape[0] == 0:
        return np.zeros((0, 0), dtype=np.uint32), np.zeros((0, 0), dtype=np.float64)
    cc = np.ascontiguousarray(c)
    idx, sc = _self_device(cc, cc, cc, lambda dc: dc.topk_self(int(k), metric_id), numpy_ok=cc is corpus)
    return idx, sc.astype(np.float64)


def kmeans(x: np.ndarray, n_clusters: int, metric: Metric = "euclidean", max_iter: int = 25, init=None, seed: int = 0,
           compute=None):
    """numpy-level k-means (an extension) of the rows of one float32 matrix:
    Lloyd's iteration on the GPU from ``init`` -- a [n_clusters, d] matrix, an
    array of n_clusters distinct row ids, or None for the rows
    ``np.sort(np.random.RandomState(seed).choice(n, n_clusters, replace=False))``
    -- for at most ``max_iter`` updates, stopped once an assignment repeats the
    previous labels.  Returns (centroids float32 [K, d], labels uint32 [n],
    scores float32 [n], updates, converged): labels and scores are the exact
    f32 top-1 of every row among the returned centroids (ties to the lower
    centroid; label 0xFFFFFFFF and a NaN score for a row whose best score is
    NaN), the update an ordered f64 sum, so the result is reproducible bit for
    bit.  metric "euclidean" or "cosine" (spherical k-means); "dot" raises
    ValueError.  Float32 matrices only (Float64, Int8 and compute= raise
    TypeError); the corpus cache as in ``within``.  The labels are what
    ``topk(..., corpus_by=labels)`` takes, with ``by=`` from ``topk(queries,
    centroids, 1)``."""
    from polars_matmul._polars_matmul import _kmeans_f32_only, _kmeans_search

    c = np.asarray(x)
    if c.dtype != np.float32:
        raise _kmeans_f32_only(f"got a {c.dtype} matrix")
    if c.ndim != 2:
        raise TypeError(f"expected a 2-D array of embeddings, got shape {c.shape}")
    cc = np.ascontiguousarray(c)
    return _kmeans_search(cc, cc, cc, n_clusters, metric, max_iter, init, seed, compute, numpy_ok=cc is x)


def matmul(queries: np.ndarray, corpus: np.ndarray) -> np.ndarray:
    """numpy-level Q @ C^T on the GPU (f32 iff both inputs are float32)."""
    q = np.asarray(queries)
    c = np.asarray(corpus)
    dt = np.float32 if (q.dtype == np.float32 and c.dtype == np.float32) else np.float64
    return _native.matmul_host(np.ascontiguousarray(q, dtype=dt), np.ascontiguousarray(c, dtype=dt))


if pl is not None:

    @pl.api.register_expr_namespace("pmm")
    class PmmNamespace:
        """Polars Expression API for similarity search (reference
        python/polars_matmul/__init__.py:39-196)."""

        def __init__(self, expr: "pl.Expr"):
            self._expr = expr

        def topk(self, corpus: "pl.Series", k: int, metric: Metric = "cosine",
                 compute: Compute = "f32", subset: "pl.Series | None" = None,
                 by: "pl.Expr | str | None" = None, corpus_by: "pl.Series | None" = None,
                 candidates: "pl.Expr | str | None" = None) -> "pl.Expr":
            """Top-k matches per embedding: List[Struct{index: u32, score: f64}].
            compute="bf16" (an extension): both columns read as f32 and
            searched on the bf16 MFMA path, the corpus kept on the device as a
            bf16 handle between calls.
            subset (an extension): a Boolean Series of len(corpus) (nulls count
            as false) or a Series of integer row ids; only those corpus rows
            are searched, ``index`` still numbers ``corpus``, and k clips to
            the number of selected rows.
            by / corpus_by (an extension, both or neither): ``by`` an
            expression or column name of the query frame, ``corpus_by`` a
            Series aligned with ``corpus``.  Every row is searched only among
            the corpus rows whose ``corpus_by`` equals its ``by`` (null matches
            nothing); the lists are ragged, min(k, rows of that label) long.
            A ``by`` column of List type (one list of labels per row, e.g. the
            nprobe nearest k-means clusters) searches the union of those
            labels' rows -- probed search, ties to the lower corpus row.
            candidates (an extension): an expression or column name of the
            query frame holding one List of corpus row ids per row (any integer
            type; a null list is empty).  Every row is searched only among its
            own list -- a lexical retriever's hits, a cheaper search's 4 k best,
            the documents it may see -- with exact f32 scores; the lists are
            ragged, min(k, candidates) long.  Float32 columns only; not with
            ``subset``, ``by`` or compute="bf16"."""
            if isinstance(corpus, pl.Expr):
                raise TypeError(
                    "corpus must be a Polars Series, not an Expression. "
                    "Use corpus['column_name'] or corpus.get_column('column_name')."
                )
            if isinstance(subset, pl.Expr):
                raise TypeError(
                    "subset must be a Polars Series, not an Expression. "
                    "Use frame['column_name'] or frame.get_column('column_name')."
                )
            if isinstance(corpus_by, pl.Expr):
                raise TypeError(
                    "corpus_by must be a Polars Series, not an Expression. "
                    "Use frame['column_name'] or frame.get_column('column_name')."
                )
            if (by is None) != (corpus_by is None):
                raise ValueError("by= and corpus_by= go together: the query rows' labels and the corpus rows' labels")
            _native.check_compute(compute)
            # (the default stays the reference's four-argument call)
            extra = {} if compute == "f32" else {"compute": compute}
            if subset is not None:
                extra["subset"] = subset
            if candidates is not None:
                if by is not None or subset is not None:
                    raise ValueError("candidates= cannot be combined with subset= or by=: "
                                     "leave the rows a query must not see out of its list")
                # the embedding and its list travel as one struct column, as by= does
                cand_expr = pl.col(candidates) if isinstance(candidates, str) else candidates
                packed = pl.struct(self._expr.alias("embedding"), cand_expr.alias("candidates"))
                return packed.map_batches(
                    lambda s: _topk(s.struct.field("embedding"), corpus, k, metric,
                                    candidates=s.struct.field("candidates"), **extra),
                    is_elementwise=True,
                    return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
                )
            if by is not None:
                # the embedding and its label travel as one struct column: rows
                # are independent, so the batches stay elementwise
                by_expr = pl.col(by) if isinstance(by, str) else by
                packed = pl.struct(self._expr.alias("embedding"), by_expr.alias("by"))
                return packed.map_batches(
                    lambda s: _topk(s.struct.field("embedding"), corpus, k, metric,
                                    groups=(s.struct.field("by"), corpus_by), **extra),
                    is_elementwise=True,
                    return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
                )
            return self._expr.map_batches(
                lambda s: _topk(s, corpus, k, metric, **extra),
                is_elementwise=True,
                return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
            )

        def within(self, corpus: "pl.Series", threshold: float, metric: Metric = "cosine",
                   subset: "pl.Series | None" = None, compute: Compute = "f32") -> "pl.Expr":
            """Range search (an extension): every corpus row whose score is
            >= ``threshold`` (cosine, dot) or <= ``threshold`` (euclidean), per
            embedding: List[Struct{index: u32, score: f64}], best first, as
            long as the row has hits.  Float32 columns only: a Float64 column
            (cast it: ``pl.col(...).cast(pl.List(pl.Float32))``) and
            compute="bf16" raise TypeError.  ``subset`` as in ``topk``."""
            if isinstance(corpus, pl.Expr):
                raise TypeError(
                    "corpus must be a Polars Series, not an Expression. "
                    "Use corpus['column_name'] or corpus.get_column('column_name')."
                )
            if isinstance(subset, pl.Expr):
                raise TypeError(
                    "subset must be a Polars Series, not an Expression. "
                    "Use frame['column_name'] or frame.get_column('column_name')."
                )
            if _native.check_compute(compute) == "bf16":
                from polars_matmul._polars_matmul import _within_f32_only

                raise _within_f32_only('compute="bf16" has no range search')
            extra = {} if subset is None else {"subset": subset}
            return self._expr.map_batches(
                lambda s: _within(s, corpus, threshold, metric, **extra),
                is_elementwise=True,
                return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
            )

        def within_self(self, threshold: float, metric: Metric = "cosine", compute: Compute = "f32") -> "pl.Expr":
            """Self range search (an extension): for every embedding the LATER
            rows of the same column whose score with it is >= ``threshold``
            (cosine, dot) or <= ``threshold`` (euclidean):
            List[Struct{index: u32, score: f64}], best first -- every
            near-duplicate pair of the column once, no row with itself.  The
            column is uploaded once and is its own query side.  A row's list
            depends on the whole column, so the expression is not elementwise.
            Float32 columns only."""
            if _native.check_compute(compute) == "bf16":
                from polars_matmul._polars_matmul import _self_f32_only

                raise _self_f32_only('compute="bf16" has no self search')
            return self._expr.map_batches(
                lambda s: _within_self(s, threshold, metric),
                is_elementwise=False,
                return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
            )

        def duplicate_groups(self, threshold: float, metric: Metric = "cosine",
                             compute: Compute = "f32") -> "pl.Expr":
            """Duplicate groups (an extension): for every embedding the number
            of the first row of its near-duplicate group -- the connected
            components of ``within_self(threshold, metric)``'s pairs -- as
            UInt32; a row with no near-duplicate carries its own number, so
            comparing with the row index keeps one row per group.  No pair
            list is built: memory does not grow with the number of duplicates.
            Not elementwise; Float32 columns only."""
            if _native.check_compute(compute) == "bf16":
                from polars_matmul._polars_matmul import _self_f32_only

                raise _self_f32_only('compute="bf16" has no self search')
            return self._expr.map_batches(
                lambda s: _duplicate_groups(s, threshold, metric),
                is_elementwise=False,
                return_dtype=pl.UInt32,
            )

        def topk_self(self, k: int, metric: Metric = "cosine", compute: Compute = "f32") -> "pl.Expr":
            """Self top-k (an extension): for every embedding its min(k, n - 1)
            best OTHER rows of the same column:
            List[Struct{index: u32, score: f64}] -- the k-nearest-neighbour
            graph.  The row itself is removed from its ranked list, so an exact
            duplicate stays whichever of the two comes first.  Not
            elementwise; Float32 columns only."""
            if _native.check_compute(compute) == "bf16":
                from polars_matmul._polars_matmul import _self_f32_only

                raise _self_f32_only('compute="bf16" has no self search')
            return self._expr.map_batches(
                lambda s: _topk_self(s, k, metric),
                is_elementwise=False,
                return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
            )

        def kmeans(self, n_clusters: int, metric: Metric = "euclidean", max_iter: int = 25, init=None,
                   seed: int = 0, compute=None) -> "pl.Expr":
            """k-means (an extension) of a Float32 embedding column: the UInt32
            cluster label of every row after Lloyd's iteration (``init``,
            ``seed`` and ``max_iter`` as ``polars_matmul.kmeans``), null for a
            row in no cluster (its best score is NaN).  euclidean or cosine.
            The labels depend on the whole column, so the expression is not
            elementwise; ``polars_matmul.kmeans`` also returns the centroids."""
            from polars_matmul._polars_matmul import _kmeans_f32_only, _kmeans_metric

            if compute is not None and compute != "f32":
                raise _kmeans_f32_only(f"compute={compute!r} has no k-means")
            _kmeans_metric(metric)
            return self._expr.map_batches(
                lambda s: _kmeans_labels(s, n_clusters, metric, max_iter, init, seed),
                is_elementwise=False,
                return_dtype=pl.UInt32,
            )

        def topk_maxsim(self, docs: "pl.Series", k: int, metric: Metric = "cosine",
                        candidates: "pl.Expr | str | None" = None) -> "pl.Expr":
            """Late-interaction top-k (an extension) of a column of token
            lists -- List[Array[Float32, d]] -- against a documents column of
            the same kind: List[Struct{index: u32, score: f64}], the documents
            ranked by MaxSim (the sum over the row's tokens of the best cosine
            or dot pair score in the document), exact f32.  candidates: an
            expression or column name holding one List of document ids per
            row, as in ``topk``; without it every row scores every document
            (rows x documents up to 2^24)."""
            if isinstance(docs, pl.Expr):
                raise TypeError(
                    "docs must be a Polars Series, not an Expression. "
                    "Use docs['column_name'] or docs.get_column('column_name')."
                )
            if candidates is not None:
                # the tokens and their list travel as one struct column, as topk's candidates= do
                cand_expr = pl.col(candidates) if isinstance(candidates, str) else candidates
                packed = pl.struct(self._expr.alias("tokens"), cand_expr.alias("candidates"))
                return packed.map_batches(
                    lambda s: _topk_maxsim(s.struct.field("tokens"), docs, k, metric,
                                           candidates=s.struct.field("candidates")),
                    is_elementwise=True,
                    return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
                )
            return self._expr.map_batches(
                lambda s: _topk_maxsim(s, docs, k, metric),
                is_elementwise=True,
                return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
            )

        def topk_hamming(self, corpus: "pl.Series", k: int) -> "pl.Expr":
            """Exact Hamming top-k (an extension) of a bit column -- UInt8
            lists or arrays of packed bits, ``sign_bits``' output -- against a
            bit corpus: List[Struct{index: u32, score: f64}], the k rows of
            least distance popcount(row XOR corpus row), ascending by
            (distance, index).  The cheap first stage of a two-stage search:
            its ids feed ``topk(..., candidates=)``."""
            if isinstance(corpus, pl.Expr):
                raise TypeError(
                    "corpus must be a Polars Series, not an Expression. "
                    "Use corpus['column_name'] or corpus.get_column('column_name')."
                )
            return self._expr.map_batches(
                lambda s: _topk_hamming(s, corpus, k),
                is_elementwise=True,
                return_dtype=pl.List(pl.Struct({"index": pl.UInt32, "score": pl.Float64})),
            )

        def sign_bits(self) -> "pl.Expr":
            """The sign of every component packed one bit per dimension (an
            extension): Array[UInt8, ceil(d / 8)], bit j of a row set iff
            component j is > 0.  Float32 columns only.  No ``return_dtype``
            is declared: the width ceil(d / 8) comes from the rows' length,
            which a List column's dtype does not carry, so a lazy frame learns
            the column's type when the expression runs."""
            return self._expr.map_batches(lambda s: _sign_bits(s), is_elementwise=True)

        def matmul(self, corpus: "pl.Series", flatten: bool = False) -> "pl.Expr":
            """All pairwise dot products: Array[f32|f64, N] per row, or one flat
            column (row-major) with flatten=True."""
            if isinstance(corpus, pl.Expr):
                raise TypeError(
                    "corpus must be a Polars Series, not an Expression. "
                    "Use corpus['column_name'] or corpus.get_column('column_name')."
                )
            n_corpus = len(corpus)
            try:
                is_f32 = corpus.dtype.inner == pl.Float32
            except Exception:
                is_f32 = False
            if flatten:
                inner_dtype = pl.Float32 if is_f32 else pl.Float64

                def _matmul_flatten(s: "pl.Series") -> "pl.Series":
                    return _matmul(s, corpus).explode()

                return self._expr.map_batches(
                    _matmul_flatten, is_elementwise=False, return_dtype=inner_dtype
                )
            dtype = pl.Array(pl.Float32 if is_f32 else pl.Float64, n_corpus)
            return self._expr.map_batches(
                lambda s: _matmul(s, corpus), is_elementwise=True, return_dtype=dtype
            )

else:

    class PmmNamespace:  # type: ignore[no-redef]
        """Placeholder: Polars is not importable, so no namespace is registered."""

        def __init__(self, *_a, **_k):
            raise ImportError("polars is not installed; use polars_matmul._topk / topk instead")
