/*
 * pmm.h -- C ABI of the MI355X-native similarity-search engine (libpmm.so).
 *
 * Drop-in boundary for the reference's `.pmm.topk` / `.pmm.matmul` hot path
 * (NivekNey/polars-matmul v0.1.4).  The reference binds its Rust numerics to
 * Python through pyo3 (src/lib.rs:15-62); the numerics themselves are
 * src/matmul.rs:295-519, src/metrics.rs:38-393 and src/topk.rs:1-75.  Every
 * entry point below names the reference function it replaces.  Plain pointers
 * and sizes only: no torch / Arrow / Polars types cross this boundary.
 *
 * Conventions
 *   - Matrices are row-major.  Q is m x d (queries), C is n x d (corpus).
 *   - Return value: PMM_OK (0) or a PMM_ERR_* code; the message of the last
 *     failure on the calling thread is available from pmm_last_error().
 *   - Thread safety: every entry point may be called concurrently from
 *     different threads (each thread owns its HIP stream and scratch).  The
 *     reference runs two `.pmm` expressions concurrently inside one Polars
 *     plan (tests/test_polars_matmul.py:551-572).
 *   - Result order per query row: best first (descending score for cosine /
 *     dot, ascending distance for euclidean); equal scores break to the lower
 *     corpus index; NaN scores rank last.  The reference leaves the order of
 *     equal scores unspecified (src/topk.rs:55-59, partial_cmp -> Equal).
 */
#ifndef PMM_H_
#define PMM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMM_OK 0
#define PMM_ERR_ARG 1         /* invalid argument (sizes, pointers, metric) */
#define PMM_ERR_HIP 2         /* HIP runtime error (message has the HIP text) */
#define PMM_ERR_UNSUPPORTED 3 /* combination not supported by this build */
#define PMM_ERR_NODEVICE 4    /* no gfx950 device visible */

/* Metric ids; src/metrics.rs:10-18 `enum Metric`. */
#define PMM_METRIC_COSINE 0
#define PMM_METRIC_DOT 1
#define PMM_METRIC_EUCLIDEAN 2

/* Arithmetic the top-k GEMM runs in (f32 inputs).  F32 = exact f32 MFMA
 * (v_mfma_f32_32x32x2_f32), the reference's precision.  BF16 = inputs rounded
 * to bf16 (round to nearest even) on device, products accumulated in f32
 * (v_mfma_f32_16x16x32_bf16), norms of the rounded rows in f32: the result is
 * the top-k of the bf16-rounded embeddings (BASELINE configs[3]).  The bf16
 * MFMA kernels take d <= 768, k <= 960 and n < 2^27; beyond (configs[4]'s
 * d = 1024, larger k) the rounded rows are widened to f32 exactly and
 * searched by the f32 path: the same bar (exact top-k of the rounded rows up
 * to f32 accumulation order) at the f32 MFMA rate. */
#define PMM_COMPUTE_F32 0
#define PMM_COMPUTE_BF16 1

const char *pmm_version(void);

/* Message of the last failing call on this thread ("" if none). */
const char *pmm_last_error(void);

/* Replaces Metric::from_str (src/metrics.rs:20-27): case-insensitive
 * "cosine" | "dot" | "euclidean" | "l2".  Unknown names return PMM_ERR_ARG with
 * pmm_last_error() = "Unknown metric: '<s>'. Supported: cosine, dot, euclidean"
 * (the reference's text, src/metrics.rs:25). */
int pmm_metric_from_str(const char *s, int *metric);

/* Replaces Metric::higher_is_better (src/metrics.rs:30-35). */
int pmm_metric_higher_is_better(int metric);

int pmm_device_count(int *count);
/* Free and total HBM of the device this thread's host calls run on
 * (hipMemGetInfo); the corpus cache sizes itself by it.  No reference
 * counterpart (the reference has no device memory). */
int pmm_device_memory(size_t *free_bytes, size_t *total_bytes);
/* Selects the HIP device that later HOST-buffer calls on this thread run on
 * (pmm_topk_f32*, pmm_topk_f64, pmm_matmul_*, pmm_corpus_create_f32,
 * pmm_device_memory); they restore the caller's current device on return.
 * Device-pointer entry points (*_device) ignore it and run on the caller's
 * current HIP device (hipSetDevice), where their pointers live. */
int pmm_set_device(int device);

/* Multi-GPU through the drop-in boundary (no reference
 * counterpart -- the reference is single-process, src/lib.rs:33-55).  With a
 * list of n >= 2 devices, pmm_topk_f32 / pmm_topk_f32_ex (k <= 1024) and
 * corpora created afterwards by pmm_corpus_create_f32 row-shard the corpus
 * over the list, one contiguous shard per entry (sizes differ by <= 1; at most
 * n shards).  Every device runs the fused top-k on its shard with global
 * indices, the per-shard [2][m][k] lists are copied peer to peer (xGMI) to
 * ids[0] and k-way merged there: the result equals the one-device result bit
 * with f32 compute (PMM_COMPUTE_F32): a shard's list is the exact top-k of
 * its rows under the total order (score, then lower index), so the merged
 * list equals the one-device result bit for bit.  With PMM_COMPUTE_BF16 the
 * result is the exact top-k of the bf16-rounded rows up to f32 accumulation
 * order, as on one device; the shard size can change which bf16 kernel and
 * threshold seed run, so near-ties may resolve differently than on one device
 * (tests assert > 99% index agreement).  A device may be listed more than once
 * (one shard per entry).  A one-entry list moves every host call to that
 * device.  The f64 entries (pmm_topk_f64, pmm_corpus_create_f64 /
 * pmm_topk_f64_corpus; any k) shard the same way: each device runs the f64
 * top-k on its shard (k_g = min(k, shard rows), padded with empty slots), the
 * [m][k] (index, f64 score) lists meet on ids[0] and are k-way merged there,
 * bit-equal to one device (indices and f64 scores).  Work that is not sharded
 * (f32 k > 1024, pmm_matmul_*) runs on ids[0].  Process-wide; n = 0 (or ids = NULL) returns to one device
 * (pmm_set_device's).
 * VERIFIED ON ONE GPU ONLY: the one-GPU test box lists device 0 repeatedly,
 * which plans all shards onto one stream; the distinct-device branch
 * (concurrent devices, cross-device event waits, peer copies over xGMI) has
 * not run on a multi-GPU node yet (tests/test_gpu_parity.py
 * test_set_devices_distinct_gpus runs it where >= 2 GPUs are visible). */
int pmm_set_devices(const int *ids, int n);
/* The current device list: *n entries, the first min(cap, *n) copied to ids. */
int pmm_get_devices(int *ids, int cap, int *n);
/* Diagnostics (no reference counterpart; no HIP call, runs without a GPU):
 * the memory plan the sharded search uses for G shards of an n-row corpus
 * over devs[0..G-1] (shard g = rows [n g / G, n (g + 1) / G)).  One plan per
 * DISTINCT device: plan_of[g] = the plan running shard g, *n_plans plans with
 * plan_dev[j] its device and plan_bytes[j] its device-memory bytes (queries,
 * host_rows ? uploaded shard rows : nothing, per-shard [2][m][k] lists at
 * list_offsets[g] inside the plan, one workspace; the root plan, plan_of[0],
 * also the gathered [G][2][m][k] lists and the merged output).  All output
 * arrays hold G entries. */
int pmm_shard_plan(const int *devs, int G, int64_t m, int64_t n, int64_t d, int64_t k, int metric, int compute,
                   int host_rows, int *plan_of, int *plan_dev, uint64_t *plan_bytes, uint64_t *list_offsets,
                   int *n_plans);

/* ---------------------------------------------------------------------------
 * Host-buffer entry points (what `_topk` / `_matmul` call; src/lib.rs:15-55).
 * Inputs are borrowed for the duration of the call and copied to HBM; outputs
 * are caller-allocated host buffers.
 * ------------------------------------------------------------------------- */

/* Replaces compute_topk_indices_scores, f32 branch (src/matmul.rs:429-448):
 * compute_similarity_matrix_f32 (src/metrics.rs:314-365) +
 * select_topk_with_scores_f32 (src/topk.rs:42-75), fused so the m x n score
 * matrix is never materialised.  k is clipped to n (src/matmul.rs:443) by the
 * caller; out_idx / out_score hold m*k entries.  Scores are f32 here; the
 * Python layer widens them to f64 as src/matmul.rs:447 does. */
int pmm_topk_f32(const float *q, int64_t m, const float *c, int64_t n, int64_t d, int64_t k,
                 int metric, uint32_t *out_idx, float *out_score);

/* Same with an explicit compute mode (PMM_COMPUTE_F32 / PMM_COMPUTE_BF16). */
int pmm_topk_f32_ex(const float *q, int64_t m, const float *c, int64_t n, int64_t d, int64_t k,
                    int metric, int compute, uint32_t *out_idx, float *out_score);

/* Replaces compute_topk_indices_scores, f64 branch (src/matmul.rs:449-468):
 * compute_similarity_matrix (src/metrics.rs:258-311) +
 * select_topk_with_scores (src/topk.rs:6-39). */
int pmm_topk_f64(const double *q, int64_t m, const double *c, int64_t n, int64_t d, int64_t k,
                 int metric, uint32_t *out_idx, double *out_score);

/* The same f64 top-k on device rows (row strides >= roundup(d, 16) and
 * multiples of 2 -- the GEMM stages rows with 16-byte loads; an odd stride is
 * PMM_ERR_ARG -- zero-padded, 16-byte-aligned bases) on the caller's stream,
 * in the thread's cached buffer (see "Device-resident entry points" for what
 * that means for streams); out_idx / out_score
 * are device buffers of m*k entries, indices offset by index_base.  k <=
 * 1024 and an m x n score matrix of 256 MB or more: fused (f64 MFMA GEMM whose
 * epilogue appends each element that beats its row's running k-th to a
 * candidate buffer, the corpus scanned in growing column chunks with the k-th
 * raised between chunks: no m x n matrix), else (or when a row's buffer
 * overflows) the materialised GEMM + row select.  The fused scan
 * synchronises the stream before returning (its overflow check); the
 * materialised path returns with the work queued on the stream. */
int pmm_topk_f64_device(const double *q, int64_t ldq, int64_t m, const double *c, int64_t ldc, int64_t n,
                        int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *out_idx,
                        double *out_score, void *stream);

/* Replaces matmul_slice_f32 / matmul_f32 (src/metrics.rs:160-202, :204-255):
 * out (m x n, row-major) = Q * C^T. */
int pmm_matmul_f32(const float *q, int64_t m, const float *c, int64_t n, int64_t d, float *out);

/* Page-locked host memory for results (hipHostMalloc, portable to every
 * device).  `.pmm.matmul` returns an m x n matrix (40 MB at the reference
 * benchmark's size): written into a fresh pageable buffer, the call pays that
 * buffer's page faults and the runtime's staging; into a page-locked one the
 * D2H copy runs at link rate.  The Python layer keeps a pool of these and
 * hands them to Arrow as foreign buffers (the reference moves its result Vec
 * into the Series the same way, src/matmul.rs:116-124).  No reference
 * counterpart of the allocation itself. */
int pmm_host_alloc(size_t bytes, void **out);
int pmm_host_free(void *p);

/* Replaces matmul_slice_f64 / matmul_f64 (src/metrics.rs:111-157, :40-97). */
int pmm_matmul_f64(const double *q, int64_t m, const double *c, int64_t n, int64_t d,
                   double *out);

/* ---------------------------------------------------------------------------
 * Device-resident entry points: inputs already in HBM, work enqueued on the
 * caller's HIP stream (NULL = the HIP default stream, as in the HIP API), no
 * host synchronisation.
 * Used by the benchmark and the multi-GPU (corpus-sharded) path.
 *
 * The stream.  Every kernel, fill and copy of an entry goes to `stream` and
 * nowhere else, so the entry reads what the stream produced before the call
 * and its outputs are ready for whatever the caller enqueues behind it.  The
 * entry returns with the work queued, except in the places below, where the
 * host needs a word from the device and waits for the stream (the results are
 * the same; only the host's progress differs):
 *   - pmm_topk_f32_device on the screened route (f32 cosine with
 *     PMM_F32_SCREEN in force): it reads back the screen's scalars -- the rows
 *     to re-run, an unsafe corpus -- before it decides on the f32 re-run;
 *   - pmm_topk_f64_device on the fused scan: its overflow flag;
 *   - pmm_topk_i8_device and pmm_topk_bits_device: the count of rows whose
 *     buffer overflowed, and again after a re-run, whose allocation is freed;
 *   - workspace = NULL (and pmm_topk_f64_device, which has no workspace
 *     argument) when the thread's cached buffer has to grow: the old buffer is
 *     freed once its last use and the stream have finished.
 * Not synchronising: the fused, materialised and global-sort routes of
 * pmm_topk_f32_device, every route of pmm_topk_bf16_device (the widened one
 * included), the materialised route of pmm_topk_f64_device, pmm_norms_*,
 * pmm_round_bf16_device, pmm_screen_prepare_device, pmm_pack_sign_device and
 * the three merge entries.  (pmm_timing_enable does not change this.)
 *   The thread's cached buffer is shared by all streams the thread passes: a
 * use on another stream than the last one waits, on the device, for an event
 * recorded at the end of that use, and so does a host entry or a handle call
 * of the same thread.  Two calls on two streams that both pass workspace =
 * NULL therefore run one after the other; give each its own workspace to
 * overlap them.
 *
 * Alignment.  Operand bases are 16-byte aligned and rows start 16-byte
 * aligned: strides are multiples of 4 (f32), 8 (bf16), 2 (f64) or 16 (int8
 * and bit rows) elements, at least the padded width.  The rows of the norms,
 * rounding, preparing and sign-packing entries need their element's alignment
 * only.  out_idx and out_score need their element's alignment.  A caller's
 * workspace for the f32 and bf16 entries is 16-byte aligned (its regions
 * start at multiples of 256 bytes from it and hold 64-bit keys, 16-byte fills
 * and staged rows), for the int8 and bit entries 256-byte aligned.  What an
 * entry cannot take it refuses with PMM_ERR_ARG before it enqueues anything,
 * naming the value; it never runs a misaligned access.
 *
 * Largest row stride.  pmm_topk_f32_device and pmm_topk_bf16_device take ldq
 * and ldc of at most 8388592 bytes (2097148 floats, 4194296 bf16 elements):
 * their kernels read up to 256 rows (a corpus tile, a wave's query rows)
 * through one buffer descriptor of 2^31 - 1 bytes with 32-bit offsets, and a
 * read past a descriptor returns zeros.  A longer stride is PMM_ERR_ARG before
 * anything is enqueued; the message names the stride and this limit.  A
 * threshold seed reads its whole sample through one descriptor: where
 * sample rows x ldc pass 2^31 - 1 bytes the call runs unseeded, with the same
 * lists.  pmm_topk_workspace_bytes takes no stride and promises no route the
 * entry then refuses.  The f64, int8 and bit top-k and the merges take any
 * stride, and the norms, rounding, preparing and sign-packing entries any
 * input stride, spans past 2^32 bytes included: they index with 64-bit
 * products (tests/test_gpu_wide_strides.py; their output strides are not
 * tested past 2^31 bytes).
 * ------------------------------------------------------------------------- */

/* Scratch bytes pmm_topk_f32_device (compute F32) or pmm_topk_bf16_device
 * (compute BF16) needs for this problem, for the path the call will take
 * with the environment as it is now (the screened f32 cosine path,
 * PMM_F32_SCREEN, adds the bf16 images of both operands). */
size_t pmm_topk_workspace_bytes(int64_t m, int64_t n, int64_t d, int64_t k, int metric,
                                int compute);

/* Algorithmic bytes of the last fused top-k's merge pass (merge_kernel) for
 * this problem and workspace, read after the call completed: the split
 * counts, the candidates the GEMM left, the shared thresholds and the m x k
 * output; after a screened f32 call also the exact finish's traffic (every
 * kept candidate read and rewritten, its f32 corpus row gathered).
 * Measurement only (the HBM-roofline line of the reduction);
 * synchronous.  Call it with the environment the top-k call ran under. */
int pmm_topk_merge_bytes(const void *workspace, int64_t m, int64_t n, int64_t d, int64_t k,
                         int metric, int compute, uint64_t *bytes);

/* Fused top-k over device buffers.  d is the logical dimension; ldq / ldc are
 * row strides in elements, multiples of 4 and >= roundup(d, 32), with columns
 * d..roundup(d, 32)-1 zero-filled and 16-byte-aligned bases (pmm_topk_f32 pads
 * host inputs itself).  Norms use exactly d elements in the reference's order
 * (ndarray unrolled_dot).  index_base is added to every
 * returned corpus index (global index of corpus row 0 of this shard).  For
 * k <= 1024, k may exceed n (a small shard): slots past n are empty (index
 * 0xFFFFFFFF, score NaN).  workspace may be NULL (a per-thread cached buffer
 * is used); a caller's workspace holds at least pmm_topk_workspace_bytes at a
 * 16-byte-aligned address (less of either: PMM_ERR_ARG; here and for
 * pmm_topk_bf16_device). */
int pmm_topk_f32_device(const float *q, int64_t ldq, int64_t m, const float *c, int64_t ldc,
                        int64_t n, int64_t d, int64_t k, int metric, int compute,
                        uint32_t index_base, uint32_t *out_idx, float *out_score,
                        void *workspace, size_t workspace_bytes, void *stream);

/* The bf16 compute path over device-resident bf16 rows (bit patterns, e.g. a
 * torch.bfloat16 tensor): d is the logical dimension; ldq / ldc >=
 * roundup(d, 128), multiples of 8, columns d..roundup(d, 128)-1 zero-filled,
 * 16-byte-aligned bases (any d and k: past the bf16 kernels' limits, the
 * widened f32 path of PMM_COMPUTE_BF16).  As for f32 rows, whatever lies in a
 * row's stride at and past the padded width is the caller's: it is never
 * read.  Scores are f32; k may exceed n as in pmm_topk_f32_device. */
int pmm_topk_bf16_device(const uint16_t *q, int64_t ldq, int64_t m, const uint16_t *c,
                         int64_t ldc, int64_t n, int64_t d, int64_t k, int metric,
                         uint32_t index_base, uint32_t *out_idx, float *out_score,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Row norms over device rows, the first stage of the metric pipeline:
 * replaces compute_norms_f32 / compute_squared_norms_f32
 * (src/metrics.rs:382-393; f64: compute_norms / compute_squared_norms,
 * :368-379).  out[r] = sqrt(row.row) (squared = 0, cosine) or row.row
 * (squared = 1, euclidean), accumulated in ndarray's unrolled_dot order
 * over exactly d elements with no FMA contraction -- the values the fused
 * top-k kernels use.  a has `rows` rows of stride ld elements (ld >= d). */
int pmm_norms_f32_device(const float *a, int64_t ld, int64_t rows, int64_t d, int squared,
                         float *out, void *stream);
int pmm_norms_f64_device(const double *a, int64_t ld, int64_t rows, int64_t d, int squared,
                         double *out, void *stream);

/* f32 device rows rounded to bf16 and, in the same pass, their norms: what a
 * caller holding f32 rows needs before pmm_topk_bf16_device (and what
 * pmm_corpus_create_bf16 / pmm_topk_bf16_corpus run).  a has `rows` rows of
 * stride ld >= d floats (any alignment; 16-byte loads when a is 16-byte
 * aligned and ld a multiple of 4).  out takes the bf16 bit patterns at row
 * stride ldo >= d, a multiple of 8 (roundup(d, 128) for the top-k entry),
 * 16-byte-aligned base; columns d..ldo-1 are written as zero.  Rounding is to
 * nearest even, NaN stays NaN.  Each of the four per-row arrays may be NULL
 * (skipped): norm = sqrt(sum), inv_norm = norm > 1e-6 ? 1 / norm : 0 (the
 * cosine pre-filter factor with the reference's zero-norm rule), sq = sum,
 * sq_factor = sum * (1 - 2^-18) (the euclidean pre-filter factor), all from
 * one sum of squares of the ROUNDED values in ndarray's unrolled_dot order
 * with no FMA contraction: bit-equal to pmm_norms_f32_device on the rounded
 * rows widened to f32, and to the norms the bf16 top-k computes itself.  One
 * launch; every f32 element is read once and every bf16 element written once
 * (6 bytes per element).  No reference counterpart. */
int pmm_round_bf16_device(const float *a, int64_t ld, int64_t rows, int64_t d, uint16_t *out,
                          int64_t ldo, float *norm, float *inv_norm, float *sq, float *sq_factor,
                          void *stream);

/* f32 device rows prepared for the screened f32 cosine top-k (the bf16 screen
 * with an exact f32 re-score) in one read of the rows: what the handle's
 * screened call runs over its queries and the handle's image build over the
 * corpus.  a, ld, out and ldo as for pmm_round_bf16_device (any alignment of
 * a; out 16-byte aligned, ldo >= d a multiple of 8, columns d..ldo-1 zero;
 * round to nearest even, NaN stays NaN).  Each per-row array may be NULL
 * (skipped):
 *   norm, inv_norm: the cosine norm and pre-filter factor of the UNROUNDED
 *     row, bit-equal to pmm_norms_f32_device (squared = 0) and to
 *     norm > 1e-6 ? 1 / norm : 0;
 *   rel: an upper bound of ||x - bf16(x)|| / ||x||, the measured ratio
 *     inflated by 2^-9 and capped at 2^-8 (2^-8 for an unsafe row);
 *   unsafe: 1 when the screen's bound does not hold for the row -- an element
 *     that is not finite or, unless zero, lies outside [2^-48, 2^48], a norm
 *     at or below 1e-6, a zero sum of squares -- else 0.
 * scalars (NULL, or two words the caller zeroed): [0] takes the maximum rel
 * over the safe rows (f32 bits, atomically), [1] is set when any row is
 * unsafe.  One launch, 6 bytes of traffic per element.  No reference
 * counterpart. */
int pmm_screen_prepare_device(const float *a, int64_t ld, int64_t rows, int64_t d, uint16_t *out,
                              int64_t ldo, float *norm, float *inv_norm, float *rel,
                              uint32_t *unsafe, uint32_t *scalars, void *stream);

/* k-way merge of per-shard top-k lists: idx/score are [m][lists][k_in] (the
 * lists in any order; idx 0xFFFFFFFF marks an empty slot).  Writes the best k_out of each row to out_idx/out_score
 * [m][k_out].  This is the merge step after the RCCL gather of the
 * corpus-sharded path (no reference counterpart: the reference is
 * single-process). */
int pmm_merge_topk_device(const uint32_t *idx, const float *score, int64_t m, int64_t lists,
                          int64_t k_in, int64_t k_out, int metric, uint32_t *out_idx,
                          float *out_score, void *stream);

/* The same merge over any list layout: entry i of list s of row r is
 * idx[r * row_stride + s * list_stride + i] (and the same offset in score).
 * pmm_merge_topk_device is (lists * k_in, k_in).  The sharded path gathers
 * each rank's [idx plane | score plane] (2 x m x k_in 32-bit words) straight
 * into a [ranks][2][m][k_in] buffer with ONE collective and merges it in
 * place: idx = buffer, score = buffer + m * k_in, row_stride = k_in,
 * list_stride = 2 * m * k_in (no re-layout copy). */
int pmm_merge_topk_strided_device(const uint32_t *idx, const float *score, int64_t m,
                                  int64_t lists, int64_t k_in, int64_t row_stride,
                                  int64_t list_stride, int64_t k_out, int metric,
                                  uint32_t *out_idx, float *out_score, void *stream);

/* The same merge of lists that are each best-first under the total order
 * (score, then lower index; empty slots last) -- as every pmm_topk_* and merge
 * output is.  A row's answer is then a prefix of each list: the kernel reads
 * the first 256 / lists entries of each and reads on only for a row whose
 * prefixes cannot hold its k_out best (lists <= 64, k_out <= 256; otherwise
 * the general merge).  Unsorted input gives unspecified results.  The
 * sharded paths (in-process and RCCL) merge with this entry. */
int pmm_merge_sorted_topk_strided_device(const uint32_t *idx, const float *score, int64_t m,
                                         int64_t lists, int64_t k_in, int64_t row_stride,
                                         int64_t list_stride, int64_t k_out, int metric,
                                         uint32_t *out_idx, float *out_score, void *stream);

/* ---------------------------------------------------------------------------
 * Device-resident corpus: upload a corpus once and run many top-k calls
 * against it (Polars' map_batches may call `_topk` repeatedly with the same
 * corpus Series: python/polars_matmul/__init__.py:115-119).  The handle keeps
 * the padded rows in HBM and the norms of every metric (src/metrics.rs:368-393,
 * computed once at creation).  A handle may be used from several threads
 * concurrently; it is bound to the device current at creation, or sharded over
 * the device list (pmm_set_devices) in effect then.  Its row type is fixed at
 * creation: an f32 handle serves pmm_topk_f32_corpus (the reference's f32
 * branch, src/matmul.rs:429-448), an f64 handle pmm_topk_f64_corpus (the f64
 * branch, src/matmul.rs:449-468 -- what Polars' default Float64 columns take),
 * a bf16 handle pmm_topk_bf16_corpus (PMM_COMPUTE_BF16 of pmm_topk_f32_ex, no
 * reference counterpart).
 * ------------------------------------------------------------------------- */
typedef struct pmm_corpus pmm_corpus;

#define PMM_DTYPE_F32 0
#define PMM_DTYPE_F64 1
#define PMM_DTYPE_BF16 2
#define PMM_DTYPE_I8 3
#define PMM_DTYPE_BITS 4

int pmm_corpus_create_f32(const float *c, int64_t n, int64_t d, pmm_corpus **out);
/* An f64 corpus: rows kept in f64 (stride roundup(d, 16), zero-padded) with
 * their f64 norms of both metrics; with pmm_set_devices in effect, row-sharded
 * over the list like an f32 corpus (pmm_topk_f64_corpus merges the shards). */
int pmm_corpus_create_f64(const double *c, int64_t n, int64_t d, pmm_corpus **out);
/* A bf16 corpus: host f32 rows in; per shard the rows are uploaded and one
 * pass (pmm_round_bf16_device's kernel) leaves the rows rounded to bf16 at
 * stride roundup(d, 128), zero-padded, and the f32 norms of the rounded rows
 * for both metrics (norm, 1 / norm, squared norm, squared norm * (1 - 2^-18):
 * 16 bytes per row).  The f32 staging is freed before the call returns, so a
 * handle holds n * roundup(d, 128) * 2 + 16 n bytes: half an f32 handle's
 * rows.  Sharded over a device list like an f32 corpus; the f32 creator's
 * argument errors and texts. */
int pmm_corpus_create_bf16(const float *c, int64_t n, int64_t d, pmm_corpus **out);
/* An int8 corpus: rows of signed bytes kept as they are (stride roundup(d, 64)
 * bytes, zero-padded) with each row's integer sum of squares (u32) and the f32
 * factor 1 / sqrt(sum) (0 for a zero row): n * roundup(d, 64) + 8 n bytes, an
 * eighth of the f64 handle the same column took before.  d < 65536, else
 * PMM_ERR_UNSUPPORTED.  Never sharded: with pmm_set_devices in effect the
 * handle lives on the list's first device.  pmm_corpus_subset_*,
 * pmm_corpus_partition and pmm_range_f32_corpus refuse it with
 * PMM_ERR_UNSUPPORTED. */
int pmm_corpus_create_i8(const int8_t *c, int64_t n, int64_t d, pmm_corpus **out);
/* PMM_DTYPE_F32, PMM_DTYPE_F64, PMM_DTYPE_BF16, PMM_DTYPE_I8 or PMM_DTYPE_BITS. */
int pmm_corpus_dtype(const pmm_corpus *corpus, int *dtype);
int pmm_corpus_destroy(pmm_corpus *corpus);
int pmm_corpus_info(const pmm_corpus *corpus, int64_t *n, int64_t *d, int *device);
/* Number of device shards of a corpus handle (1, or the device list's length
 * capped at n when pmm_set_devices was in effect at creation). */
int pmm_corpus_shards(const pmm_corpus *corpus, int *shards);
/* HBM the handle holds now: its rows and norm arrays and, once an f32 handle
 * has built it (pmm_topk_f32_corpus), its screen image. */
int pmm_corpus_bytes(const pmm_corpus *corpus, size_t *bytes);

/* A handle derived on the device from a resident handle and a set of allowed
 * rows: subset search ("filter, then search") without a second upload.  ids
 * is a host array of s parent row numbers, strictly ascending, each < n,
 * 1 <= s <= n; it is validated on the host in O(s) and a violation is
 * PMM_ERR_ARG naming the first offending position.  The derived handle holds
 * those rows densely at the parent's stride, the parent's norms of both
 * metrics for them (gathered, not recomputed: the bits the norm kernels
 * produce), a uint32[s] index map and, when an f32 parent has its screen image
 * and the gathered image fits in half of the free HBM, that image's rows,
 * residuals and flags with the parent's maximum residual (an upper bound over
 * a superset of the rows: it only widens the screen's slack).  A gathered
 * unsafe flag drops the gathered image and the derived handle never screens;
 * a parent's own "never screens" state is not inherited (the subset may leave
 * the unsafe row out), and without a parent image the derived handle builds
 * its own on its first screened call.  No row crosses PCIe and no norm is
 * recomputed.  The result is an ordinary pmm_corpus of the parent's row type
 * with n = s, independent of the parent (pmm_corpus_destroy frees it), and
 * every pmm_topk_*_corpus entry serves it through its usual routes -- but
 * returns the PARENT's row numbers: ascending ids keep "lower index first"
 * the same order in both numberings, so the lists are the exact top-k among
 * the allowed rows, ties included.  One-shard f32, f64 and bf16 parents; a
 * sharded parent is PMM_ERR_UNSUPPORTED, a null or derived parent PMM_ERR_ARG.
 * Runs on the calling thread's stream and synchronises before it returns; a
 * failed allocation is PMM_ERR_HIP with the HIP text and leaks nothing (a
 * failed allocation of the optional image: no image, no error).  No reference
 * counterpart. */
int pmm_corpus_subset_ids(const pmm_corpus *parent, const uint32_t *ids, int64_t s, pmm_corpus **out);

/* pmm_corpus_subset_ids with the rows given as an Arrow validity-style bitmap
 * (host memory, least significant bit first): row r of the parent is allowed
 * iff bit bit_offset + r is set, r in [0, n); bit_offset >= 0, any value (a
 * sliced Arrow Boolean array's offset).  The bitmap's bytes are uploaded and
 * compacted into the ascending index map on the device; the count is read back
 * once to size the allocations.  An empty selection is PMM_ERR_ARG.  No
 * reference counterpart. */
int pmm_corpus_subset_mask(const pmm_corpus *parent, const uint8_t *bitmap, int64_t bit_offset,
                           pmm_corpus **out);

/* A derived handle's index map copied to the host: *s takes its length and ids
 * (may be NULL when cap is 0) its first min(cap, s) entries.  A handle that is
 * not derived: *s = 0.  No reference counterpart. */
int pmm_corpus_index_map(const pmm_corpus *corpus, uint32_t *ids, int64_t cap, int64_t *s);

/* ---------------------------------------------------------------------------
 * Grouped search: every query row is searched only among the corpus rows that
 * carry its own label (Polars' over() / group_by on a search).  A label is a
 * uint32 in [0, G); PMM_NO_GROUP marks a row that is in no group.  No
 * reference counterpart (the reference has one filter per call, on the host).
 * ------------------------------------------------------------------------- */
#define PMM_NO_GROUP 0xFFFFFFFFu

/* The plan of a partition: a stable counting sort of the row numbers 0..n-1
 * by label.  Host only -- it touches no device and runs without one.
 * labels[i] is in [0, G) or PMM_NO_GROUP (the row is dropped); any other
 * value is PMM_ERR_ARG naming the first offending position.  perm (room for n
 * entries) takes the kept rows group by group, strictly ascending inside a
 * group; offsets (G + 1 entries) the groups' bounds in perm -- group g is
 * perm[offsets[g] .. offsets[g + 1]); *kept = offsets[G].  G >= 0,
 * n < 2^32 - 1. */
int pmm_partition_plan(const uint32_t *labels, int64_t n, int64_t G, uint32_t *perm, int64_t *offsets,
                       int64_t *kept);

/* A handle derived on the device from a resident handle whose rows are stored
 * grouped by label: pmm_partition_plan on the host (labels: n entries, one per
 * parent row; G >= 1), the permutation uploaded as the handle's index map, the
 * rows and the parent's norm arrays gathered by pmm_corpus_subset_ids' kernel
 * (f32, f64 and bf16 parents alike; no row crosses PCIe, no norm is
 * recomputed), and the groups' offsets kept on the host and on the device
 * (pmm_corpus_bytes counts them).  The parent limits are pmm_corpus_subset_ids':
 * one shard (else PMM_ERR_UNSUPPORTED), not itself derived or partitioned
 * (PMM_ERR_ARG).  Every row dropped: PMM_ERR_ARG.  No screen image is gathered
 * and the handle never screens.  Its index map ascends only inside a group,
 * so an ungrouped search would break the tie order: pmm_topk_*_corpus and
 * pmm_corpus_subset_* on a partitioned handle return PMM_ERR_ARG and say so.
 * An f32 handle serves pmm_topk_f32_grouped, an f64 handle
 * pmm_topk_f64_grouped; a bf16 handle can be partitioned but has no grouped
 * entry here (the Python layer searches bf16 corpora per label instead).
 * Independent of the parent (pmm_corpus_destroy frees it); synchronises
 * before it returns. */
int pmm_corpus_partition(const pmm_corpus *parent, const uint32_t *labels, int64_t G, pmm_corpus **out);

/* A partitioned handle's groups, the read-back counterpart of
 * pmm_corpus_index_map (which returns its permutation): *G takes the number
 * of groups and offsets (may be NULL when cap is 0) the first min(cap, G + 1)
 * segment bounds.  A handle that is not partitioned: *G = 0. */
int pmm_corpus_groups(const pmm_corpus *corpus, int64_t *G, int64_t *offsets, int64_t cap);

/* Grouped top-k against a partitioned f32 handle (host queries in, host
 * results out; any k >= 0).  Query row i is searched only against the segment
 * of group qlabels[i] (in [0, G), or PMM_NO_GROUP; another value is
 * PMM_ERR_ARG).  out_len[i] = min(k, rows of that segment), 0 for
 * PMM_NO_GROUP or an empty segment.  The first out_len[i] slots of row i
 * (row stride k in out_idx / out_score) are the exact top-k among that
 * group's rows -- the PARENT's row numbers, best first, the total order of
 * every pmm_topk_* entry (inside a group ascending partition row is ascending
 * parent row, so ties break as a search of the group's rows alone breaks
 * them); the remaining slots hold index 0xFFFFFFFF and score 0.  Indices and
 * score bits equal pmm_topk_f32 on the group's rows.
 * The queries are uploaded once, grouped by label on the device and cut into
 * (query range, segment) pairs.  Pairs with k <= 128, roundup(d, 32) <= 1024
 * and a segment of at most PMM_GROUPED_SEG_MAX rows (read per call) all run
 * in ONE launch of the grouped kernel; the others run one after another
 * through the route pmm_topk_f32_corpus takes for the pair's shape, unscreened.
 * PMM_GROUPED=kernel | loop (per call) forces a path where its limits allow.
 * One more launch maps the lists to the parent's numbering and the caller's
 * query order.  A handle that is not partitioned, or holds other rows:
 * PMM_ERR_ARG; a bf16 handle: PMM_ERR_UNSUPPORTED. */
int pmm_topk_f32_grouped(const pmm_corpus *corpus, const float *q, int64_t m, const uint32_t *qlabels, int64_t k,
                         int metric, uint32_t *out_idx, float *out_score, uint32_t *out_len);

/* The same against a partitioned f64 handle: every pair runs through
 * pmm_topk_f64_corpus' paths (there is no grouped f64 kernel), exact against
 * pmm_topk_f64 on the group's rows. */
int pmm_topk_f64_grouped(const pmm_corpus *corpus, const double *q, int64_t m, const uint32_t *qlabels, int64_t k,
                         int metric, uint32_t *out_idx, double *out_score, uint32_t *out_len);

/* The plan of a probed search: (query row, probe list) into work slots.  Host
 * only -- it touches no device and runs without one.  Query row i carries the
 * labels probe_labels[probe_offsets[i] .. probe_offsets[i + 1])
 * (probe_offsets: m + 1 entries from 0, never decreasing); group_offsets
 * (G + 1 entries) are the partition's segment bounds (pmm_corpus_groups).  A
 * label is in [0, G) or PMM_NO_GROUP; any other value is PMM_ERR_ARG naming the
 * position and the query row.  PMM_NO_GROUP entries and labels of empty
 * segments are skipped and a repeated label counts once.  The kept
 * (row, label) slots leave stably sorted by label -- ascending query row inside
 * a label: slot s is query row slot_row[s] in group slot_label[s].  Row i's
 * slot numbers, ascending by label, are row_slots[row_offsets[i] ..
 * row_offsets[i + 1]) (row_offsets: m + 1 entries); *slots = row_offsets[m].
 * out_len[i] = min(k, rows of row i's segments).  slot_row, slot_label and
 * row_slots have room for probe_offsets[m] entries (row_slots is also the
 * plan's scratch).  m, G < 2^32 - 1, 0 <= k < 2^31.  A plan whose slots x k
 * would pass 2^31 list entries: PMM_ERR_UNSUPPORTED (split the call). */
int pmm_probe_plan(const int64_t *probe_offsets, const uint32_t *probe_labels, int64_t m,
                   const int64_t *group_offsets, int64_t G, int64_t k, uint32_t *slot_row, uint32_t *slot_label,
                   int64_t *row_offsets, uint32_t *row_slots, uint32_t *out_len, int64_t *slots);

/* Probed top-k against a partitioned f32 handle (host queries in, host
 * results out; 0 <= k <= 128): query row i is searched in the union of the
 * groups its probe list names (pmm_probe_plan's reading of probe_offsets /
 * probe_labels) -- IVF with several probes, a row visible in several groups.
 * With ids_i the ascending PARENT row numbers of every row of those groups,
 * row i's list is pmm_topk_f32(q[i], parent rows ids_i, min(k, len(ids_i)))
 * with its indices mapped through ids_i: the same indices, score bits and tie
 * order (equal scores go to the lower parent row, also across groups).
 * out_len[i] = min(k, len(ids_i)); the slots past it hold index 0xFFFFFFFF and
 * score +0.0.  A row with one probe gets pmm_topk_f32_grouped's bits; probing
 * every group of a partition that dropped no row gives pmm_topk_f32_corpus'
 * bits on the parent.
 * The queries are uploaded once and never copied per probe: the grouped
 * kernel's row-table variant reads slot s's query row through slot_row[s],
 * ONE launch for every (group, <= 16 slots) unit whose segment has at most
 * PMM_GROUPED_SEG_MAX rows and roundup(d, 32) <= 1024; the other pairs gather
 * their rows and run one after another through pmm_topk_f32_corpus' route
 * (PMM_GROUPED=kernel | loop as in the grouped entry).  One launch of the merge
 * kernel then keeps every row's best k of its per-group lists, keyed by score
 * and parent row, and writes the caller's rows.
 * A label that is no group: PMM_ERR_ARG before any device call.  A handle that
 * is not partitioned: PMM_ERR_ARG; an f64 or bf16 handle, k > 128, or slots x
 * k past 2^31: PMM_ERR_UNSUPPORTED. */
int pmm_topk_f32_probed(const pmm_corpus *corpus, const float *q, int64_t m, const int64_t *probe_offsets,
                        const uint32_t *probe_labels, int64_t k, int metric, uint32_t *out_idx, float *out_score,
                        uint32_t *out_len);

/* pmm_topk_f32 against a device-resident corpus (host queries in, host
 * results out; 0 <= k <= n).  Results are pmm_topk_f32's bit for bit.
 *
 * A cosine call whose shape asks for the bf16 screen (the limits, thresholds
 * and per-call PMM_F32_SCREEN of pmm_topk_f32_device) on a handle of one
 * shard screens against the handle's screen image: the rows rounded to bf16
 * at stride roundup(d, 128) with each row's rounding residual and unsafe flag
 * (n * roundup(d, 128) * 2 + 8 n bytes; pmm_screen_prepare_device's kernel).
 * The first such call builds it, when it fits in half of the free HBM; it is
 * published whole, so concurrent callers see no image or all of it, and
 * pmm_corpus_destroy frees it.  A failed allocation is no error: the call runs
 * unscreened and a later call tries again.  A corpus with an unsafe row (zero,
 * non-finite or out-of-window values) keeps no image and never screens: the
 * flag is read once, at the build.  pmm_corpus_create_f32 builds no image.
 * Sharded handles run unscreened. */
int pmm_topk_f32_corpus(const pmm_corpus *corpus, const float *q, int64_t m, int64_t k,
                        int metric, uint32_t *out_idx, float *out_score);

/* pmm_topk_f64 against an f64 corpus handle (host queries in, host results
 * out; 0 <= k <= n; any k: the fused scan for k <= 1024 and a large score
 * matrix, else the materialised path, as pmm_topk_f64_device).  The results
 * equal pmm_topk_f64's bit for bit: the handle's norms are the ones every
 * call would compute, by the same kernel.  An f32 handle: PMM_ERR_ARG (and
 * pmm_topk_f32_corpus refuses an f64 handle the same way). */
int pmm_topk_f64_corpus(const pmm_corpus *corpus, const double *q, int64_t m, int64_t k,
                        int metric, uint32_t *out_idx, double *out_score);

/* pmm_topk_f32_ex(..., PMM_COMPUTE_BF16) against a bf16 corpus handle (host
 * f32 queries in, host results out, f32 scores; 0 <= k <= n).  On one device
 * the queries are uploaded and rounded by one pass that also writes the
 * metric's query norms (none for dot), and the search takes the route the host
 * entry takes with the handle's norms: no corpus upload, rounding or norms
 * per call.  The results equal pmm_topk_f32_ex(..., PMM_COMPUTE_BF16)'s bit
 * for bit (indices and scores), the widened route past d > 768 or k > 960
 * included (there the norms are recomputed from the widened rows, the same
 * values).  A sharded handle serves k <= 1024 (else PMM_ERR_UNSUPPORTED, as an
 * f32 handle) and equals the host entry under the same device list.  An f32
 * or f64 handle: PMM_ERR_ARG naming the entry that serves it (and
 * pmm_topk_f32_corpus / pmm_topk_f64_corpus refuse a bf16 handle the same
 * way). */
int pmm_topk_bf16_corpus(const pmm_corpus *corpus, const float *q, int64_t m, int64_t k,
                         int metric, uint32_t *out_idx, float *out_score);

/* ---------------------------------------------------------------------------
 * Rows of signed bytes (quantised embeddings; Polars Int8 columns).  The
 * reference widens them to f64 (src/matmul.rs:13-19, :143, :179) and takes its
 * f64 branch (:449-468); these entries return THAT answer -- the indices, the
 * f64 score bits and the tie order of pmm_topk_f64 on the values cast to f64 --
 * computed on the int8 MFMA (v_mfma_i32_16x16x64_i8).  An int8 dot product is
 * exact in i32 and a row's sum of squares in u32, so every f64 score is the
 * oracle's two or three correctly rounded operations on exact integers; a
 * zero score is +0.0.
 *   Limits.  d < 65536 (a sum of squares and a squared distance stay in u32,
 * a dot in i32), else PMM_ERR_UNSUPPORTED.  The int8 scan takes
 * roundup(d, 64) <= 2048 and k <= 1024; past either, both sides are widened to
 * f64 on the device (exactly) and searched by the f64 path: the same bits at
 * the f64 rate.  A query row whose candidate buffer overflows (many equal
 * corpus rows at its k-th place) is searched again on the widened rows, the
 * same bits again.  k = 0, m = 0 and k > n as pmm_topk_f64.  Under
 * pmm_set_devices the host entry runs on the list's first device (int8 rows
 * are not sharded).  Every entry synchronises the stream before it returns.
 * ------------------------------------------------------------------------- */
int pmm_topk_i8(const int8_t *q, int64_t m, const int8_t *c, int64_t n, int64_t d, int64_t k, int metric,
                uint32_t *out_idx, double *out_score);

/* pmm_topk_i8 against an int8 corpus handle (pmm_corpus_create_i8), bit-equal
 * to it: host queries in, host results out, 0 <= k <= n.  A handle of other
 * rows: PMM_ERR_ARG naming the entry that serves it (and pmm_topk_f32_corpus /
 * pmm_topk_f64_corpus / pmm_topk_bf16_corpus refuse an int8 handle the same
 * way, naming this entry). */
int pmm_topk_i8_corpus(const pmm_corpus *corpus, const int8_t *q, int64_t m, int64_t k, int metric,
                       uint32_t *out_idx, double *out_score);

/* Bytes of workspace pmm_topk_i8_device needs for this problem: the one route
 * decision (int8 scan or widened f64 search) the call then follows, with the
 * environment as it is now.  Touches no device.  0 for an empty or refused
 * problem. */
size_t pmm_topk_i8_workspace_bytes(int64_t m, int64_t n, int64_t d, int64_t k, int metric);

/* The same top-k over device rows on the caller's stream: ldq / ldc are row
 * strides in bytes, multiples of 16 and >= roundup(d, 64), columns past d
 * zero-filled, 16-byte-aligned bases; out_idx / out_score device buffers of
 * m * k entries, indices offset by index_base.  workspace: NULL (a per-thread
 * cached buffer) or workspace_bytes >= pmm_topk_i8_workspace_bytes at a
 * 256-byte-aligned address (an overflow re-run allocates for itself). */
int pmm_topk_i8_device(const int8_t *q, int64_t ldq, int64_t m, const int8_t *c, int64_t ldc, int64_t n, int64_t d,
                       int64_t k, int metric, uint32_t index_base, uint32_t *out_idx, double *out_score,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Bit rows (binary embeddings: the sign of each component) and the exact
 * Hamming top-k.  A bit row is w >= 1 bytes = D = 8 w bits; bit j is
 * (byte[j >> 3] >> (j & 7)) & 1, least significant bit first (numpy's
 * packbits(bitorder="little"), Arrow's bitmap order); no partial bytes.  The
 * score of query row i and corpus row j is popcount(q_i XOR c_j), an integer
 * in 0 .. D returned as f64 (exact); LOWER is better.  Row i's list holds the
 * k corpus rows of least distance, ascending by (distance, corpus index): a
 * tie at any place, the k-th included, goes to the lower index.
 *   For 0/1 vectors popcount(a AND b) is the dot product and the distance is
 * Pq + Pc - 2 dot (P: a row's popcount), so the scan runs on the int8 MFMA
 * (v_mfma_i32_16x16x64_i8) over bytes expanded from the bits in LDS, with the
 * int8 scan's euclidean key.
 *   Limits.  w <= 8192, else PMM_ERR_UNSUPPORTED.  k <= 1024 takes the MFMA
 * scan; a larger k expands both sides to 0/1 f64 rows on the device and takes
 * the f64 path's euclidean search, whose score s gives rint(s * s): the same
 * lists.  That route is for small corpora: the expansion takes
 * (m + n) * roundup(8 w, 16) * 8 bytes of workspace, 512 times the packed rows
 * (8 GB for 1M rows of 128 bytes; pmm_topk_bits_workspace_bytes states it), and
 * a call whose workspace does not fit fails in the allocation with
 * PMM_ERR_HIP.  A query row whose candidate buffer overflows is scanned again in
 * chunks that cannot overflow, the same lists again.  k = 0, m = 0 and k > n
 * as pmm_topk_f64.  Under pmm_set_devices the entries run on the list's first
 * device (bit rows are not sharded).  Every entry synchronises the stream
 * before it returns.
 * ------------------------------------------------------------------------- */

/* Sign packing on the device: bit j of output row r is 1 iff x[r * ldx + j] >
 * 0.0f -- +0, -0, negatives, -inf and NaN give 0, subnormals follow their
 * sign, +inf gives 1 -- for j < d; each row's roundup(ceil(d / 8), 8) bytes
 * are written whole, the bits from d up as zeros; bytes past them are left.
 * x: device f32 rows, any 4-byte-aligned address, ldx >= d floats; out: device
 * rows of ld_out bytes, ld_out >= roundup(ceil(d / 8), 8) and a multiple of 8,
 * 8-byte-aligned.  rows = 0 is PMM_OK.  Asynchronous on `stream`. */
int pmm_pack_sign_device(const float *x, int64_t ldx, int64_t rows, int64_t d, uint8_t *out, int64_t ld_out,
                         void *stream);

/* A bit corpus: n host rows of w packed bytes, kept at stride roundup(w, 16)
 * bytes (zero-padded: the search kernel's staging group) with one u32
 * popcount per row: n * roundup(w, 16) + 4 n bytes (pmm_corpus_bytes returns
 * it).  Never sharded.  pmm_corpus_subset_*, pmm_corpus_partition, the range,
 * self and candidate entries refuse it as they refuse an int8 handle, and the
 * other pmm_topk_*_corpus entries name pmm_topk_bits_corpus. */
int pmm_corpus_create_bits(const uint8_t *c, int64_t n, int64_t w, pmm_corpus **out);

/* The bit corpus of a resident f32 handle's rows: their signs (the rule of
 * pmm_pack_sign_device, w = ceil(d / 8)) packed on the device from the rows
 * the parent already holds -- no upload -- with the popcounts from the same
 * pass; the bytes pmm_corpus_create_bits makes of the same bits.  The parent:
 * an f32 handle of one shard, plain or derived by pmm_corpus_subset_* (the
 * index map is copied, + 4 n bytes, so the lists number the original corpus).
 * A partitioned, f64, bf16, int8 or bit parent: PMM_ERR_ARG; a sharded one:
 * PMM_ERR_UNSUPPORTED.  The result is independent of the parent. */
int pmm_corpus_sign_bits(const pmm_corpus *f32_parent, pmm_corpus **out);

/* The rows of a bit corpus handle copied to the host: out takes n x w bytes,
 * row-major without padding (pmm_corpus_info gives n and w).  With
 * pmm_corpus_sign_bits this packs a resident f32 corpus on the device and
 * returns the bytes.  A handle of other rows: PMM_ERR_ARG. */
int pmm_corpus_bits_rows(const pmm_corpus *corpus, uint8_t *out);

/* Hamming top-k of host rows: q (m x w), c (n x w) packed bytes, row-major;
 * out_idx / out_score m x k. */
int pmm_topk_bits(const uint8_t *q, int64_t m, const uint8_t *c, int64_t n, int64_t w, int64_t k, uint32_t *out_idx,
                  double *out_score);

/* pmm_topk_bits against a bit corpus handle, the same lists: host queries of
 * the handle's w bytes in, host results out, 0 <= k <= n.  A handle of other
 * rows: PMM_ERR_ARG naming the entry that serves it. */
int pmm_topk_bits_corpus(const pmm_corpus *corpus, const uint8_t *q, int64_t m, int64_t k, uint32_t *out_idx,
                         double *out_score);

/* Bytes of workspace pmm_topk_bits_device needs for this problem: the one
 * route decision (MFMA scan or expanded f64 search) the call then follows,
 * with the environment as it is now.  Touches no device.  0 for an empty or
 * refused problem. */
size_t pmm_topk_bits_workspace_bytes(int64_t m, int64_t n, int64_t w, int64_t k);

/* The same top-k over device rows on the caller's stream: ldq / ldc are row
 * strides in bytes, multiples of 16 and >= roundup(w, 16), bytes past w
 * zero-filled, 16-byte-aligned bases; out_idx / out_score device buffers of
 * m * k entries, indices offset by index_base.  workspace: NULL (a per-thread
 * cached buffer) or workspace_bytes >= pmm_topk_bits_workspace_bytes at a
 * 256-byte-aligned address. */
int pmm_topk_bits_device(const uint8_t *q, int64_t ldq, int64_t m, const uint8_t *c, int64_t ldc, int64_t n, int64_t w,
                         int64_t k, uint32_t index_base, uint32_t *out_idx, double *out_score, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Range search: every corpus row whose score passes a threshold, for each
 * query row (host queries in, host results out).  Corpus row j is a hit of
 * query row i iff its score s -- the exact f32 score, the bits pmm_topk_f32
 * returns -- satisfies s >= threshold (cosine, dot) or s <= threshold
 * (euclidean): IEEE comparisons, so -0.0 and +0.0 are the same threshold and
 * a NaN score is never a hit.  A NaN threshold is PMM_ERR_ARG; +-inf are legal.
 * The result is CSR: out_offsets (m + 1 entries) always takes the exact
 * bounds -- out_offsets[i + 1] - out_offsets[i] is the hit count of row i --
 * and *total = out_offsets[m].  When total <= cap (the entries out_idx and
 * out_score have room for), row i's hits fill out_idx / out_score
 * [out_offsets[i], out_offsets[i + 1]), best first in the total order of every
 * pmm_topk_* entry (score, then lower index): the first count_i entries of row
 * i of pmm_topk_f32_corpus with k = n, indices and score bits.  When total >
 * cap the call still returns PMM_OK and writes nothing to out_idx / out_score:
 * call again with room.  cap = 0 with null out_idx / out_score is the
 * count-only form.
 * One pass of the f32 top-k kernel's tiles, staging and K-ordered chain (the
 * 128 x 128 or 256 x 256 variant by the problem's size; PMM_GEMM_VARIANT = 0
 * or 3, per call, chooses) emits each element that passes a conservative
 * per-row bound and then the exact comparison as a record (ordered key |
 * column, query row) through one global cursor; the hit counts are read back
 * (the call's one wait before the lists), the keys are binned by row, each
 * row's segment sorted -- up to 128 keys in a wave, up to PMM_RANGE_SORT_MAX
 * (8192; read per call, can only be lowered) in a workgroup's LDS, longer
 * ones through pmm_topk_f32_corpus with k = the count -- and decoded.  The
 * keys of a row are unique, so the lists do not depend on the order the
 * records arrived in.  The screen image is never used.
 * Serves an f32 handle of one shard, plain or derived by pmm_corpus_subset_*
 * (a derived handle returns the PARENT's row numbers; its ascending map keeps
 * the tie order).  A sharded handle: PMM_ERR_UNSUPPORTED; a partitioned
 * handle: PMM_ERR_ARG (the text of pmm_topk_f32_corpus); an f64 or bf16
 * handle: PMM_ERR_ARG.  Null corpus, q, out_offsets or total, negative m or
 * cap, a bad metric: PMM_ERR_ARG before any device call.  m = 0: PMM_OK with
 * out_offsets[0] = 0.  Thread-safe like the other handle entries (the calling
 * thread's stream and arena); synchronises before it returns.  No reference
 * counterpart. */
int pmm_range_f32_corpus(const pmm_corpus *corpus, const float *q, int64_t m, float threshold, int metric,
                         int64_t cap, int64_t *out_offsets /* m + 1 */, uint32_t *out_idx, float *out_score,
                         int64_t *total);

/* Candidate search: exact top-k of every query row over its OWN list of
 * corpus rows (host queries and lists in, host results out; any k >= 1, since
 * k only cuts a sorted list).  Row i's candidates are cand_ids[cand_offsets[i]
 * .. cand_offsets[i + 1]): corpus row numbers, strictly ascending within a
 * row, each below n.  Its result is the first out_len[i] = min(k, count_i)
 * entries of the ranked list of exactly those rows, in the total order of
 * every pmm_topk_* entry (best first, NaN last, equal scores to the lower
 * index; -0.0 and +0.0 tie and a returned zero carries the reference's sign):
 * the index and score bits pmm_topk_f32 returns on the candidate rows alone,
 * its indices mapped through the list.  Row stride k in out_idx / out_score;
 * the slots past out_len[i] hold index 0xFFFFFFFF and score +0.0 (the grouped
 * entries' convention).  An empty list gives out_len[i] = 0; a list of every
 * row gives pmm_topk_f32_corpus' list.
 * One launch scores every (row, candidate) pair: a workgroup takes one query
 * row and up to 256 of its candidates, a lane one pair -- the f32 path's
 * K-ordered fmaf chain over exactly d elements and its epilogue on the
 * handle's norms -- with the candidate rows gathered 128 bytes per eight
 * lanes through LDS, two K chunks of loads in flight.  The keys (ordered
 * score | ~id) land in the lists' own CSR layout and are sorted by the range
 * search's kernels: up to 128 keys in a wave, up to PMM_RANGE_SORT_MAX (8192;
 * read per call, can only be lowered) in a workgroup's LDS; a longer list is
 * cut into pieces of that size, each sorted, and its best min(k, count) keys
 * merged by rank counting.  One more launch decodes the first out_len[i] keys
 * of every row into the planes and fills the rest.  The screen image is never
 * used.
 * Errors.  Null corpus, q, cand_offsets or an output, null cand_ids with a
 * non-empty list, negative m, k < 1, a bad metric, cand_offsets that do not
 * start at 0 or that descend, a list longer than n: PMM_ERR_ARG before any
 * device call.  A list that is not strictly ascending or holds an id >= n is
 * found on the device (such an id is clamped before it forms an address) and
 * reported after the call's wait as PMM_ERR_ARG naming the case; the lists are
 * then unspecified.  m = 0: PMM_OK.
 * Serves a plain f32 handle of one shard.  A derived (pmm_corpus_subset_*) or
 * partitioned handle: PMM_ERR_ARG (list the candidates in the parent's row
 * numbers and search the parent); an f64, bf16 or int8 handle: PMM_ERR_ARG; a
 * sharded handle: PMM_ERR_UNSUPPORTED.  Thread-safe like the other handle
 * entries (the calling thread's stream and arena, one arena acquisition);
 * synchronises once before it returns.  No reference counterpart. */
int pmm_topk_f32_candidates(const pmm_corpus *corpus, const float *q, int64_t m,
                            const int64_t *cand_offsets /* m + 1 */, const uint32_t *cand_ids,
                            int64_t k, int metric,
                            uint32_t *out_idx /* m * k */, float *out_score /* m * k */,
                            uint32_t *out_len /* m */);

/* Late interaction (ColBERT / ColPali style): multi-vector documents and the
 * MaxSim score.  No reference counterpart.
 *
 * pmm_corpus_create_f32_docs: an ordinary f32 handle of one shard over the
 * n_tokens token rows (the rows and norms of pmm_corpus_create_f32, so every
 * existing entry serves it as the plain handle of its tokens and
 * pmm_topk_f32_corpus on it is the token-level search) that also keeps the
 * documents' bounds, on the host and on the device: document c is token rows
 * [doc_offsets[c], doc_offsets[c + 1]).  The offsets start at 0, end at
 * n_tokens and ascend strictly (no empty document), else PMM_ERR_ARG naming
 * the position, before any device call.  Never sharded: with pmm_set_devices
 * in effect the handle is made on the current device, as the int8 creator's.
 * pmm_corpus_bytes counts the offsets; pmm_corpus_destroy frees them.  Handles
 * derived from it (pmm_corpus_subset_*, pmm_corpus_partition,
 * pmm_corpus_sign_bits) carry no documents. */
int pmm_corpus_create_f32_docs(const float *tokens, int64_t n_tokens, int64_t d,
                               const int64_t *doc_offsets /* n_docs + 1 */, int64_t n_docs, pmm_corpus **out);

/* The documents of a handle: *n_docs (0 for a handle without documents) and,
 * with doc_offsets_out and cap >= n_docs + 1, the n_docs + 1 bounds (a smaller
 * cap copies nothing: call once with cap = 0 to size the array). */
int pmm_corpus_docs(const pmm_corpus *corpus, int64_t *n_docs, int64_t *doc_offsets_out, int64_t cap);

/* The largest padded dimension (roundup(d, 32)) the MaxSim kernel serves: its
 * block of 32 query tokens (dp + 4 floats each) and four waves' document tiles
 * must fit the CU's 160 KiB of LDS. */
#define PMM_MAXSIM_MAX_DP 960

/* MaxSim top-k over per-row lists of documents.  Query row i holds the tokens
 * q_tokens[q_offsets[i] .. q_offsets[i + 1]) (d floats each, Lq_i >= 0 of
 * them) and lists the documents cand_docs[cand_offsets[i] .. cand_offsets[i +
 * 1]), strictly ascending, each below n_docs.  The score of (row, document):
 *   s[t][j]  the engine's f32 pair score of query token t and document token
 *            j (the K-ordered fmaf chain from +0.0f and, for cosine, the
 *            epilogue on the two tokens' norms: pmm_topk_f32's bits);
 *   mx[t]    fmaxf over j from -inf (a NaN pair score is ignored);
 *   score    (((+0.0f + mx[0]) + mx[1]) + ...) in f32, in token order.
 * The score is never -0.0.  Row i's result is its documents by (score
 * descending, document ascending, a NaN score last), the first out_len[i] =
 * min(k, listed documents) of them; a row without tokens has out_len[i] = 0.
 * Planes as pmm_topk_f32_candidates': row stride k, the slots past out_len[i]
 * hold index 0xFFFFFFFF and score +0.0.  metric: cosine or dot (a maximum over
 * distances is no similarity: euclidean is PMM_ERR_ARG).
 * One launch scores every pair -- a workgroup takes a query row and up to 64
 * of its documents, a wave one document at a time on v_mfma_f32_32x32x2_f32
 * with the max and the sum folded into the epilogue, so no Lq x Ld block
 * leaves the registers -- into keys in the lists' own layout, which the range
 * search's sorts and the candidate search's merge order (PMM_RANGE_SORT_MAX is
 * honoured); one more launch decodes.
 * Errors.  A null argument, k < 1, negative m, a bad metric or euclidean, a
 * handle without documents, a derived, partitioned or non-f32 handle, offsets
 * that do not start at 0 or that descend, a list longer than n_docs:
 * PMM_ERR_ARG before the handle's device is touched.  A sharded handle, or a
 * padded dimension above PMM_MAXSIM_MAX_DP: PMM_ERR_UNSUPPORTED.  A list that
 * does not ascend strictly or holds an id >= n_docs is found on the device
 * (the id is clamped before it forms an address) and reported after the wait
 * as PMM_ERR_ARG; the lists are then unspecified.  m = 0: PMM_OK.  Thread-safe
 * like the other handle entries; synchronises once before it returns. */
int pmm_topk_f32_maxsim(const pmm_corpus *corpus, const float *q_tokens, const int64_t *q_offsets /* m + 1 */,
                        int64_t m, const int64_t *cand_offsets /* m + 1 */, const uint32_t *cand_docs,
                        int64_t k, int metric,
                        uint32_t *out_idx /* m * k */, float *out_score /* m * k */,
                        uint32_t *out_len /* m */);

/* Self search: one handle searched against itself -- near-duplicate pairs and
 * the k-nearest-neighbour graph of its rows.  Neither entry takes queries: the
 * handle's n rows are the query rows (nothing is uploaded) and, for the range
 * entry, its cached norms are the query norms.  Both serve an f32 handle of
 * one shard, plain or derived by pmm_corpus_subset_* (a derived handle returns
 * the PARENT's row numbers; "row i" and "j > i" below are handle positions,
 * and the map ascends, so they are parent order too).  A sharded handle:
 * PMM_ERR_UNSUPPORTED; a partitioned handle: PMM_ERR_ARG (the text of
 * pmm_topk_f32_corpus); an f64 or bf16 handle: PMM_ERR_ARG; an int8 handle:
 * PMM_ERR_UNSUPPORTED (as pmm_range_f32_corpus).  Every argument check comes
 * before the handle is read.  Thread-safe like the other handle entries;
 * no reference counterpart.
 *
 * pmm_range_f32_self: row i's list is the list pmm_range_f32_corpus returns
 * for query row i when the queries are the handle's own rows, without the
 * entries at handle positions j <= i: each unordered pair {i, j} that passes
 * the threshold appears once, under its lower row, and the diagonal never
 * appears whatever its score.  Indices, score bits and the best-first order
 * are that call's; so are the cap / total protocol (out_offsets has n + 1
 * entries; total > cap writes no list; cap = 0 with null lists counts), the
 * NaN-threshold refusal and the folding of the two zeros.  The score of
 * (i, j) has the bits of the dropped (j, i) for all three metrics: the chain
 * multiplies the same pairs in the same K order, and the epilogues join the
 * two norms by one commutative IEEE operation (cosine their product,
 * euclidean the sum of the squared norms); the definition does not lean on
 * it.
 * The emit pass is the range pass on a triangular schedule: query block b
 * (BM rows) visits corpus tile t (BN columns) iff min(n, (t + 1) BN) - 1 >
 * b BM, the comparison column > row runs only in the tiles that reach a
 * wave's own rows, and everything else -- K order, staging, exact score -- is
 * the range pass's (pmm_range_self_plan reports the schedule).  Binning,
 * sorting and decoding are the range search's; a row with more hits than
 * PMM_RANGE_SORT_MAX is cut into pieces of that size, each sorted, and merged
 * by rank counting as the candidate search does (the handle's ordinary top-k
 * does not know j > i).  n = 0 or 1: PMM_OK with empty lists.  Null corpus,
 * out_offsets or total, negative cap, cap > 0 with a null list, a bad
 * metric: PMM_ERR_ARG. */
int pmm_range_f32_self(const pmm_corpus *corpus, float threshold, int metric, int64_t cap,
                       int64_t *out_offsets /* n + 1 */, uint32_t *out_idx, float *out_score, int64_t *total);

/* pmm_components_f32_self: duplicate groups -- the connected components of the
 * pairs pmm_range_f32_self lists.  Let E be the set of pairs (i, j), i < j,
 * that pmm_range_f32_self(threshold, metric) lists for this handle: the same
 * score bits, the same folding of the two zeros, a NaN score never an edge,
 * the diagonal never present.  out_labels[i] is the smallest handle position
 * in i's connected component of (rows, E), reported as a PARENT row number on
 * a derived handle (the map ascends, so it is the smallest parent row too); a
 * row with no edge labels itself.  The value does not depend on the order the
 * hits are found in.  *components: the number of distinct labels; *pairs:
 * |E|, pmm_range_f32_self's total.
 * The pass is pmm_range_f32_self's emit pass -- the triangular schedule, the
 * pre-filter, the exact score, the hit predicate -- except that a hit leaves no
 * record: it is counted, and its two rows are united in a lock-free union-find
 * over n words (the higher root linked under the lower by compare-and-swap),
 * where it is found.  One more launch reads every row's root.  Device memory
 * does NOT grow with the number of hits: the arena is the n parents, the n
 * labels and the pass's survivor queues, whether the column has no pair or
 * n (n - 1) / 2 of them, and there is no cap / total protocol and no second
 * run.  One wait: the labels and the pair count come back together.
 * Handles, refusals and their texts are pmm_range_f32_self's: an f32 handle of
 * one shard, plain or derived; sharded and int8 handles PMM_ERR_UNSUPPORTED,
 * partitioned, f64 and bf16 handles PMM_ERR_ARG; a NaN threshold, a bad
 * metric, a null corpus, components or pairs: PMM_ERR_ARG, all before the
 * handle is read or a device touched.  n = 0: PMM_OK, both counts 0, nothing
 * else written (out_labels may be NULL); otherwise a null out_labels is
 * PMM_ERR_ARG.  n = 1: the row's own number, 1 component, 0 pairs, no launch.
 * Thread-safe like the other handle entries; no reference counterpart. */
int pmm_components_f32_self(const pmm_corpus *corpus, float threshold, int metric,
                            uint32_t *out_labels /* n */, int64_t *components, int64_t *pairs);

/* pmm_topk_f32_self: row i's list is the ranked list of all n rows for query
 * row i (pmm_topk_f32_corpus' order: best first, NaN last, ties to the lower
 * index) with row i itself removed and then cut at k; 1 <= k <= n - 1 (else
 * PMM_ERR_ARG: clip k first; a handle of one row has no neighbours).  Row
 * stride k in out_idx / out_score (n * k entries each).
 * The handle's ordinary route for k + 1 runs with its rows as device-resident
 * queries inside the one host-call frame (the screened route where the shape
 * or PMM_F32_SCREEN selects it: bit-equal by construction), then one launch
 * (one wave per row) copies each (k + 1)-list without the entry whose index
 * is the row's own position -- or without the last entry when k + 1 others
 * rank above the row, e.g. exact duplicates with lower row numbers or a NaN
 * row.  The ranked list is a total order, so this is the definition for any
 * tie or NaN placement; asking pmm_topk_f32_corpus for k + 1 and dropping
 * rank 0 is not. */
int pmm_topk_f32_self(const pmm_corpus *corpus, int64_t k, int metric, uint32_t *out_idx /* n * k */,
                      float *out_score /* n * k */);

/* k-means (Lloyd's iteration) on the rows of an f32 handle.  No reference
 * counterpart.  The handle's n resident rows X are clustered around K
 * centroids, from the K initial centroids `init` (K * d floats):
 *
 *   C = init; updates = 0; converged = 0
 *   loop:
 *     L, S = assign(X, C)
 *     if updates > 0 and L == L_prev: converged = 1; break
 *     if updates == max_iter: break
 *     C = update(X, L, C); L_prev = L; updates += 1
 *
 * so the labels and scores returned are always the assignment against the
 * centroids returned, and max_iter = 0 is a pure assignment against init.
 *   assign.  L[i], S[i]: the exact f32 top-1 of row i among the K rows of C --
 * the bits pmm_topk_f32 (rows as queries, C as the corpus, k = 1) returns:
 * ties to the lower centroid, euclidean lower is better, the centroids' norms
 * from the norm kernel of every corpus.  A row whose best score is NaN gets
 * L[i] = PMM_NO_GROUP (what pmm_partition_plan reads as "dropped") and S[i] =
 * the quiet NaN 0x7FC00000.
 *   update.  Cluster c's members are the rows with label c in ascending row
 * order, cut into pieces of PMM_KMEANS_PIECE consecutive members (the last one
 * shorter).  Per column, each piece is summed in f64 sequentially from +0.0 in
 * member order; the piece sums are added sequentially in piece order from
 * +0.0; C[c][j] = (float)(sum / (double)count).  Euclidean: the term of row i
 * is (double)x[i][j], count the members.  Cosine (spherical k-means): the
 * term is (double)x[i][j] / (double)norm[i] with the handle's cached cosine
 * norm; a member with norm[i] <= 1e-6f (the reference's zero-norm rule) keeps
 * its place in its piece, adds no term and is not counted.  A cluster whose
 * count is 0 keeps its centroid's bits.  Rows labelled PMM_NO_GROUP belong to
 * no cluster.  The fixed two-level order makes the result independent of the
 * launch geometry.
 * Outputs: out_centroids (K * d), out_labels (n), out_score (n, may be NULL),
 * *out_updates (the updates performed, <= max_iter), *out_converged.
 * It serves an f32 handle of one shard -- plain, multi-vector (its tokens are
 * clustered) or derived by pmm_corpus_subset_* (the labels are numbered by the
 * handle's own rows).  A partitioned, f64, bf16, int8 or bit handle:
 * PMM_ERR_ARG; a sharded handle: PMM_ERR_UNSUPPORTED.  A null argument, K < 1,
 * K > n, K >= 2^32, a negative max_iter, dot (a mean does not maximise a dot
 * product) or a bad metric: PMM_ERR_ARG before any device call.  Each
 * iteration is the assignment (the fused f32 top-k), one launch that writes
 * labels, scores and a changed flag, a stable radix sort of the row numbers by
 * label on the device, and the gather-sum; the labels never visit the host
 * between iterations.  Thread-safe like the other handle entries; waits once
 * per iteration (the flag's read-back) and once at the end. */
#define PMM_KMEANS_PIECE 256
int pmm_kmeans_f32_corpus(const pmm_corpus *corpus, int64_t K, const float *init /* K * d */,
                          int metric, int64_t max_iter,
                          float *out_centroids /* K * d */, uint32_t *out_labels /* n */,
                          float *out_score /* n, may be NULL */,
                          int64_t *out_updates, int *out_converged);

/* The triangular schedule of pmm_range_f32_self's emit pass for n rows on a
 * device of `cus` compute units (host only, no device is touched).
 * variant_in: 0 (128 x 128 tiles) or 3 (256 x 256), or -1 to choose as the
 * entry does without PMM_GEMM_VARIANT.  *variant: the tile variant;
 * *block_tile_visits: the (query block, corpus tile) pairs the pass runs;
 * *block_tile_full: the QB * T pairs pmm_range_f32_corpus runs for the same
 * rows as queries.  n < 0, cus < 1, another variant_in or a null output:
 * PMM_ERR_ARG. */
int pmm_range_self_plan(int64_t n, int cus, int variant_in, int *variant, int64_t *block_tile_visits,
                        int64_t *block_tile_full);

/* The sort plan of ragged key lists -- what pmm_range_f32_self (cap =
 * INT64_MAX) and pmm_topk_f32_candidates (cap = k) lay out before they sort
 * (host only, no device is touched).  offsets: the m + 1 ascending bounds of
 * the segments, from 0.  A segment of up to smax keys is one piece; a longer
 * one is cut into ceil(count / smax) pieces of smax keys, the last one
 * shorter.  Every piece is sorted on its own; a cut segment's best
 * min(cap, count) keys are then merged to the merged-key array.
 * piece_offsets: the pieces' bounds (pieces + 1 entries); mid: the pieces of
 * more than 128 keys, ascending (the workgroup sort's; the others sort in one
 * wave); cut: one record per piece of a cut segment, segment by segment --
 * piece `self` of the segment's pieces [first, first + count), whose best
 * kout keys go to the merged keys [dst, dst + kout); counts[5]: pieces,
 * entries of mid, the longest piece in mid (0: none), entries of cut, merged
 * keys in all.  Room the caller gives: m + offsets[m] / smax pieces in each of
 * the three (one more bound in piece_offsets).  smax outside [128, 8192],
 * cap < 1, offsets that descend or do not start at 0, a null pointer:
 * PMM_ERR_ARG. */
typedef struct pmm_sort_piece {
  uint32_t self, first, count, kout;
  int64_t dst;
} pmm_sort_piece;
int pmm_sort_plan(const int64_t *offsets, int64_t m, int64_t smax, int64_t cap, int64_t *piece_offsets, int *mid,
                  pmm_sort_piece *cut, int64_t *counts);

/* Per-kernel timing on the launch stream (hipEvents around each launch).
 * enable=1 starts recording; pmm_timing_read returns the summed milliseconds
 * and launch count of kernels whose name contains `kernel` since the last
 * reset (it synchronises the recorded events). */
int pmm_timing_enable(int enable);
int pmm_timing_reset(void);
int pmm_timing_read(const char *kernel, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif

#endif /* PMM_H_ */
