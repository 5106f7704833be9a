// pmm_internal.h -- launch-side interface between the host orchestration
// (pmm_capi.hip) and the gfx950 kernels (pmm_kernels.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pmm {

// Benchmarking-only phase removal (PMM_ABLATE / PMM_MERGE_ABLATE: results are
// wrong by design).  Compiled in only by the lab build (`make lab` ->
// libpmm_lab.so, -DPMM_LAB); in the shipped libpmm.so the variables are never
// read and every ablation branch folds away at compile time.
#ifdef PMM_LAB
#define PMM_ABL(x) (x)
#else
#define PMM_ABL(x) 0
#endif

constexpr int kMetricCosine = 0;
constexpr int kMetricDot = 1;
constexpr int kMetricEuclidean = 2;

// Fused top-k path limits.  k above kFusedMaxK goes through the materialise +
// row-select path (kernels below), which also serves f64.
constexpr int kFusedMaxK = 1024;
// Row-select (materialised scores) keeps up to kRowSelMaxP entries per row in
// LDS; larger k uses the full-row global sort.
constexpr int kRowSelMaxP = 4096;

// Arguments of the f32 MFMA GEMM kernel (top-k and store modes).
struct GemmF32Args {
  const float *q;       // M x ldq
  const float *c;       // N x ldc
  const uint16_t *qb;   // bf16 compute path: M x ldq bf16 (bit patterns)
  const uint16_t *cb;   // bf16 compute path: N x ldc bf16
  const float *qn;      // cosine: L2 norms of Q rows; euclidean: squared norms
  const float *cn;      // same for C rows
  const float *cpre;    // pre-filter column factor: cosine 1/||c|| (0 if zero-norm),
                        // euclidean ||c||^2 * (1 - 2^-18)
  int64_t ldq, ldc;
  int M, N, D;          // D % 32 == 0
  int k, capg;          // top-k and candidate-buffer capacity (power of two)
  int ctrig;            // compaction trigger: a row's buffer is compacted to its best k
                        // once it holds more than ctrig entries (k < ctrig <= capg - 64)
  int metric;
  int QB, S, tps, ntiles, units;  // work decomposition (see plan_units)
  unsigned *counter;              // work-queue head, zeroed per call
  unsigned long long *cand;       // [M*S][capg] candidate composites
  unsigned *cnt;                  // [M*S] candidate counts
  unsigned long long *gthr;       // [M] shared per-row threshold, zeroed per call
  unsigned long long *wq;         // per-wave survivor queue [grid][NW][32 * BN]
  int qcap;                       // f32 kernel: survivor-queue entries per wave in LDS
                                  // (set by launch_gemm_f32; past them, wq)
  float *out;                     // store mode: out[M][ldo]
  int64_t ldo;
  int store_metric;               // store mode: 1 = metric-transformed score, 0 = raw dot
  int ablate;                     // benchmarking only (PMM_ABLATE): 1 = skip the epilogue
  int nst;                        // bf16 kernel: LDS ring slots (3 or 4)
  int round_sync;                 // bf16 kernel: align workgroups at unit rounds (speed only)
  int sync_timeout;               // bf16 kernel: round-barrier spin limit (100 MHz ticks)
  int pf;                         // bf16 kernel: corpus-fragment prefetch depth (1 or 2 substeps)
  int defer;                      // bf16 kernel: hold each K-step's last MFMA group past the barrier
  int qb_full;                    // wave-specialised bf16 kernel: query blocks processed whole
                                  // (phase A; a multiple of the grid), the rest as split units
  unsigned long long *stats;      // PMM_STATS only: [queued, flagged groups, tiles, compactions]
  // fire-and-forget bf16 kernel (pmm_bf16_ff_kernel.h): per-(unit, wave)
  // survivor regions of ffcap items (raw dot | row << 58 | column << 32) and
  // their counts (a count above ffcap: the region overflowed)
  unsigned long long *ffreg;
  unsigned *ffcnt;
  int ffcap;
  // screened f32 path (gemm_bf16_ws_kernel<KS, cosine, true>): per-row slack
  // of the bf16 scores against the exact f32 chain (score units), and per-row
  // flags set when a row's kept band outgrew its candidate segment
  const float *eps;
  unsigned *ovf;
  // screened f32 path, optional: per-row guessed bounds of the exact k-th
  // (launch_screen_guess).  A row starts from max(gthr, guess); gthr itself
  // only ever holds proven bounds, so "gthr[row] < guess[row]" after the pass
  // says the row's guess was never confirmed (screen_rescore_kernel decides).
  // Stored as the composite's high word (the score key; the low word is 0).
  const uint32_t *guess;
  // range mode (f32 kernel, mode 2): the threshold as a composite (okey32 of
  // its ranking value << 32; an element hits iff its composite is at or above
  // it), the record arena -- rcap records as key (okey32(rank value) << 32 |
  // ~column) and query row, filled through the cursor *rcur, which counts
  // every hit, stored or not -- and the rows' hit counts (zeroed per call)
  unsigned long long rthr;
  unsigned long long *rcur;
  unsigned *rhits;
  unsigned long long *rkey;
  uint32_t *rrow;
  unsigned long long rcap;
  // components mode (f32 kernel, mode 4): the union-find forest over the n
  // rows, parent[i] = i before the pass (launch_components_init)
  uint32_t *parent;
};

struct MergeArgs {
  // loader 0: candidate segments from the fused kernel
  const unsigned long long *cand;
  const unsigned *cnt;
  const unsigned long long *gthr;
  int capg;
  // loader 1: gathered (idx, score) lists; entry i of list s of row r is at
  // in_idx[r * row_stride + s * list_stride + i] (same offsets in in_score):
  // [M][S][k_in] is (S * k_in, k_in); the RCCL gather's [S][2][M][k_in]
  // (idx plane, score plane per rank) is (k_in, 2 * M * k_in)
  const uint32_t *in_idx;
  const float *in_score;
  int k_in;
  int64_t row_stride, list_stride;
  int M, S, k_out, P, metric;
  uint32_t index_base;
  uint32_t *out_idx;
  float *out_score;
  int ablate;  // benchmarking only (PMM_MERGE_ABLATE): 1 = no selection/sort, 2 = no candidate loads
  int no_rank;  // set by launch_merge: bitonic sort instead of rank counting (many rows)
  int flags;    // set by launch_merge: kMergeReverse, kMergePipelined, kMergeSplitRow
  int sorted;   // loader 1: every input list is best-first (the prefix fast path)
};
constexpr int kMergeReverse = 1;    // rows last to first (split rows, the heavy ones, start first)
constexpr int kMergePipelined = 2;  // next candidate batch's loads in flight while one is taken
constexpr int kMergeSplitRow = 4;   // a block of 4 waves per row, each merging a quarter of its lists

struct RowSelArgs {
  const void *scores;   // [rows][lds] f32 or f64, already metric-transformed
  int64_t lds;
  int rows, N, k, P, metric, is_f64;
  uint32_t index_base;  // added to every output index
  uint32_t *out_idx;    // [rows][k]
  void *out_score;      // [rows][k] f32 or f64
};

// ---- launchers (pmm_kernels.hip) ----
// (also zeroes zero_bytes at zero, a multiple of 16 at a 16-byte address)
hipError_t launch_norms_pair_f32(const float *q, int64_t m, int64_t ldq, float *qout, const float *c,
                                 int64_t n, int64_t ldc, float *cout, float *cinv, int64_t d, int squared,
                                 hipStream_t s, void *zero = nullptr, size_t zero_bytes = 0);
hipError_t launch_norms_f32(const float *a, int64_t rows, int64_t d, int64_t ld, int squared,
                            float *out, float *inv, hipStream_t s);
hipError_t launch_norms_f64(const double *a, int64_t rows, int64_t d, int64_t ld, int squared,
                            double *out, hipStream_t s);
// Tile-shape variant of the f32 GEMM (see pmm_kernels.hip): 0 = 128x128,
// 1 = 128x256, 2 = 256x128 (2 waves/SIMD), 3 = 256x256 (2 waves/SIMD),
// 4 = 128x64, 5 = 128x64 column-split (2 waves/SIMD, fused top-k only).
// mode 0 = fused top-k, 1 = store (2 = range: launch_gemm_f32_range).  grid =
// number of persistent workgroups.
hipError_t launch_gemm_f32(const GemmF32Args &a, int variant, int mode, int grid, hipStream_t s);
int gemm_f32_bm(int variant);   // query rows per workgroup
int gemm_f32_bn(int variant);   // corpus columns per tile
int gemm_f32_nw(int variant);   // waves per workgroup
int gemm_f32_segs(int variant); // candidate segments per (row, corpus split): 2 for the column split
size_t gemm_f32_lds_bytes(int variant, int mode, int capg);
// mode 2 = range (GemmF32Args::rthr ..): the same tiles, staging and chain,
// every element at or above the threshold emitted as a record.  Instantiated
// for the variants gemm_f32_range_variant names (0 and 3).
bool gemm_f32_range_variant(int variant);
hipError_t launch_gemm_f32_range(const GemmF32Args &a, int variant, int grid, hipStream_t s);
// mode 3 = self (pmm_range_f32_self): range mode with the corpus rows as the
// query rows (a.q = a.c, a.qn = a.cn, M = N), emitting only the pairs (row,
// column > row).  Unit (split, block) runs the split's tiles t with
// min(N, (t + 1) BN) - 1 > block * BM and is skipped when none is left; the
// filter column > row runs in the tiles that reach a wave's own rows.
hipError_t launch_gemm_f32_self(const GemmF32Args &a, int variant, int grid, hipStream_t s);
// The first tile (of ntiles tiles of bn columns over n rows) a query block
// starting at row0 visits in self mode, ntiles when it visits none: the rule is
// monotone in t, and (t + 1) bn - 1 > row0 first holds at t = (row0 + 1) / bn.
__host__ __device__ inline int self_first_tile(int n, int row0, int bn, int ntiles) {
  return n - 1 > row0 ? (row0 + 1) / bn : ntiles;
}
// mode 4 = components (pmm_components_f32_self): self mode's schedule, filter
// and hit predicate; a hit is counted on *rcur and unites its two rows in
// GemmF32Args::parent (lock-free union-find, the higher root under the lower)
// -- no record, no per-row count.
hipError_t launch_gemm_f32_components(const GemmF32Args &a, int variant, int grid, hipStream_t s);
// ---- duplicate groups: the forest's two passes (pmm_range.hip) ----
// parent[i] = i, i < n
hipError_t launch_components_init(uint32_t *parent, int64_t n, hipStream_t s);
// labels[i] = map ? map[root of i] : root of i, after the components pass
hipError_t launch_components_label(const uint32_t *parent, const uint32_t *map, int64_t n, uint32_t *labels,
                                   hipStream_t s);
// ---- range search: records -> per-row best-first lists (pmm_range.hip) ----
// Segments of up to kRangeWaveMax keys sort in one wave's registers, up to
// kRangeSortMax in one workgroup's LDS (64 KiB of keys).
constexpr int kRangeWaveMax = 128;
constexpr int kRangeSortMax = 8192;
// keys[offsets[row] + (the row's next free place)] = rkey[i], row = rrow[i],
// i < total; cur (m words, zeroed by the caller) holds the rows' places
hipError_t launch_range_bin(const unsigned long long *rkey, const uint32_t *rrow, int64_t total,
                            const int64_t *offsets, unsigned *cur, unsigned long long *keys, hipStream_t s);
// every row's segment of 2 .. kRangeWaveMax keys sorted best first, one wave per row
hipError_t launch_range_sort_wave(unsigned long long *keys, const int64_t *offsets, int m, hipStream_t s);
// the segments of rows[0 .. r) (each of at most pmax <= kRangeSortMax keys,
// pmax a power of two) sorted best first, one workgroup per row
hipError_t launch_range_sort_block(unsigned long long *keys, const int64_t *offsets, const int *rows, int r,
                                   int pmax, hipStream_t s);
struct RangeDecodeArgs {
  const unsigned long long *keys;  // binned, sorted
  int64_t total;
  const int64_t *offsets;          // m + 1 segment bounds (device)
  int m, metric, d;
  const uint32_t *map;             // a derived handle's index map, or null
  // cosine: what a +0.0 score's sign is recomputed from (see zero_sign_kernel)
  const float *q, *c, *qn, *cn;
  int64_t ldq, ldc;
  uint32_t *out_idx;
  float *out_score;
};
// keys -> (index, score) by the top-k epilogue's rules
hipError_t launch_range_decode(const RangeDecodeArgs &a, hipStream_t s);
// out[row][0 .. k) = in[row][0 .. k] without the entry whose index is `row`
// (or without the last one when there is none)
hipError_t launch_drop_self(const uint32_t *in_idx, const float *in_score, int64_t m, int64_t k, uint32_t *out_idx,
                            float *out_score, hipStream_t s);
// ---- candidate search: per-row candidate lists (pmm_candidates.hip) ----
// One work unit of the score pass = one workgroup: query row `row` against
// its candidates [start, start + kCandUnit) (places in the row's list).
constexpr int kCandUnit = 256;
struct CandUnit {
  uint32_t row, start;
};
struct CandScoreArgs {
  const float *q, *c;        // queries (row stride ldq) and the handle's rows (ldc), zero-padded to a multiple of 32
  const float *qn, *cn;      // cosine: norms, euclidean: squared norms; dot: unused
  const int64_t *offsets;    // m + 1 list bounds (device)
  const uint32_t *ids;       // the lists
  const CandUnit *unit;      // device table, one entry per workgroup
  int units;
  int64_t ldq, ldc;
  uint32_t n;                // corpus rows
  int d, metric;
  unsigned long long *keys;  // [offsets[m]]: okey32(rank value) << 32 | ~id, laid out as the lists
  unsigned *flag;            // |= 1: a list does not ascend strictly, |= 2: an id >= n (zeroed by the caller)
};
// keys[offsets[i] + j] = the composite of (query row i, corpus row ids[offsets[i] + j])
hipError_t launch_cand_score(const CandScoreArgs &a, hipStream_t s);
// A list longer than the in-LDS sort is cut into pieces that are sorted on
// their own (launch_range_sort_*, over the piece bounds).  Piece `self` of the
// row's pieces [first, first + T): the row's best kout keys go to dst[dst ..).
struct CandPiece {
  uint32_t self, first, T, kout;
  int64_t dst;
};
hipError_t launch_cand_merge(const unsigned long long *keys, const int64_t *piece_offsets, const CandPiece *pieces,
                             int npieces, unsigned long long *dst, hipStream_t s);
struct CandDecodeArgs {
  const unsigned long long *keys;  // sorted; row i's best keys start at keys[src[i]]
  const int64_t *src;
  const int64_t *offsets;          // m + 1 list bounds (device): row i has offsets[i + 1] - offsets[i] candidates
  int m, metric, d;
  int64_t k;
  // what a +0.0 cosine or dot score's sign is recomputed from (see range_decode_kernel)
  const float *q, *c, *qn, *cn;
  int64_t ldq, ldc;
  uint32_t *out_idx;               // [m][k], unused slots 0xFFFFFFFF
  float *out_score;                // [m][k], unused slots +0.0
  uint32_t *out_len;               // [m]: min(k, candidates)
};
hipError_t launch_cand_decode(const CandDecodeArgs &a, hipStream_t s);
// ---- late interaction: MaxSim over multi-vector documents (pmm_maxsim.hip) ----
// One work unit of the score pass = one workgroup: query row `row` (all its
// tokens, 32 at a time) against the documents at places [start, start +
// kMaxsimRun) of its list (a CandUnit).  The kernel keeps a block of 32 query
// tokens of dp + 4 floats and four waves' document tiles in LDS: the largest
// padded dimension whose carve fits the CU's 160 KiB is kMaxsimMaxDp
// (PMM_MAXSIM_MAX_DP in pmm.h).
constexpr int kMaxsimRun = 64;
constexpr int kMaxsimMaxDp = 960;
struct MaxsimScoreArgs {
  const float *q, *c;          // the query tokens (row stride ldq) and the handle's token rows (ldc), zero-padded to dp
  const float *qn, *cn;        // cosine: the tokens' norms; dot: unused
  const int64_t *q_offsets;    // m + 1 bounds of the rows' tokens in q (device)
  const int64_t *doc_offsets;  // n_docs + 1 bounds of the documents' tokens in c (device), strictly ascending
  const int64_t *offsets;      // m + 1 list bounds (device)
  const uint32_t *ids;         // the lists: document numbers
  const CandUnit *unit;        // device table, one entry per workgroup
  int units;
  int64_t ldq, ldc;
  uint32_t n_docs;
  int dp, metric;              // dp % 32 == 0, dp <= kMaxsimMaxDp; cosine or dot
  unsigned long long *keys;    // [offsets[m]]: okey32(score) << 32 | ~document, laid out as the lists
  unsigned *flag;              // |= 1: a list does not ascend strictly, |= 2: an id >= n_docs (zeroed by the caller)
};
size_t maxsim_lds_bytes(int dp);
hipError_t launch_maxsim_score(const MaxsimScoreArgs &a, hipStream_t s);
struct MaxsimDecodeArgs {
  const unsigned long long *keys;  // sorted; row i's best keys start at keys[src[i]]
  const int64_t *src;
  const int64_t *offsets;          // m + 1 list bounds (device)
  const int64_t *q_offsets;        // m + 1 token bounds (device): a row without tokens has length 0
  int m;
  int64_t k;
  uint32_t *out_idx;               // [m][k], unused slots 0xFFFFFFFF
  float *out_score;                // [m][k], unused slots +0.0
  uint32_t *out_len;               // [m]
};
hipError_t launch_maxsim_decode(const MaxsimDecodeArgs &a, hipStream_t s);
// ---- k-means on a resident f32 handle (pmm_kmeans.hip) ----
// The update sums a cluster's members (ascending rows) in pieces of
// kKmeansPiece consecutive members: each piece sequentially in f64 from +0.0,
// then the pieces in order from +0.0 (PMM_KMEANS_PIECE in pmm.h).  This
// constant is the one place the piece length is set.
constexpr int kKmeansPiece = 256;
// The ordering pass sorts runs of this many rows per wave.
constexpr int kKmeansSortRows = 1024;
// labels[i] = oi[i] and scores[i] = os[i] of the [n][1] top-1 lists; a NaN
// score gives the label 0xFFFFFFFF and the canonical NaN.  have_prev: *changed
// = 1 when a label differs from the one `labels` held (zeroed by the caller).
hipError_t launch_kmeans_labels(const uint32_t *oi, const float *os, int64_t n, uint32_t K, uint32_t *labels,
                                float *scores, bool have_prev, unsigned *changed, hipStream_t s);
struct KmeansOrder {
  const uint32_t *labels;      // [n]: a cluster below K or 0xFFFFFFFF
  int64_t n;
  uint32_t K;
  uint32_t *key[2], *val[2];   // [n] each: the sort's two key and row buffers
  uint32_t *hist, *base;       // [256 * kmeans_sort_units(n)] each
  uint32_t *bounds;            // [K + 1]: cluster c's members are sorted rows [bounds[c], bounds[c + 1])
  uint32_t *pbase;             // [K + 1]: cluster c's pieces are [pbase[c], pbase[c + 1])
};
int64_t kmeans_sort_units(int64_t n);
int kmeans_sort_passes(uint32_t K);                 // 8-bit digits of the keys 0 .. K
int64_t kmeans_max_pieces(int64_t n, int64_t K);    // an upper bound of pbase[K]
// the rows by (label, row), the rows of no cluster last; then bounds and pbase
hipError_t launch_kmeans_order(const KmeansOrder &a, hipStream_t s);
const uint32_t *kmeans_sorted_rows(const KmeansOrder &a);  // the buffer the last pass wrote
struct KmeansUpdateArgs {
  const float *x;              // the handle's rows (row stride ldx), zero-padded to dp
  int64_t ldx;
  const float *cn;             // cosine: the rows' norms (term x / norm, a norm <= 1e-6f adds none); euclidean: null
  const uint32_t *rows, *bounds, *pbase;  // launch_kmeans_order's
  uint32_t K;
  int d, dp;                   // dp % 32 == 0
  int64_t max_pieces;          // kmeans_max_pieces(n, K): the rows of psum and pcount
  double *psum;                // [max_pieces][dp] piece sums
  uint32_t *pcount;            // [max_pieces] members that added a term
  float *C;                    // [K][dp] centroids, updated in place
};
hipError_t launch_kmeans_update(const KmeansUpdateArgs &a, hipStream_t s);  // -> psum, pcount
hipError_t launch_kmeans_finish(const KmeansUpdateArgs &a, hipStream_t s);  // psum, pcount -> C
hipError_t launch_merge(const MergeArgs &a, int loader, hipStream_t s);
// Threshold seeding: gthr[row] = (k-th best composite of the row's ns
// materialised scores S[row][0..ns)) - 1, one wave per row; ns <= kSeedMaxNs.
constexpr int kSeedMaxNs = 1024;
// Row strides of pmm_topk_f32_device and pmm_topk_bf16_device.  Their GEMMs and
// threshold seeds read rows through buffer descriptors with 32-bit byte
// offsets, and a descriptor's size ends at kDescMaxBytes -- a load past it
// returns zeros, it does not fault.
//   GEMMs: one descriptor spans a corpus tile (BN rows) or a wave's query
// rows (32; 64 in the fire-and-forget kernel): at most kDescRowsMax rows
// (static_asserts below and at the kernels).  A stride of at most
// kMaxRowStrideBytes keeps such a span inside the size field and every offset
// below 2^31; the entries refuse a longer stride.
//   Seeds: one descriptor spans the sample's ns rows, more than a tile.  A
// seed only raises the starting thresholds, so a call whose sample does not
// fit one descriptor (seed_span_fits) runs unseeded: the same lists.
constexpr int64_t kDescMaxBytes = 0x7FFFFFFFll;
constexpr int kDescRowsMax = 256;
constexpr int64_t kMaxRowStrideBytes = (kDescMaxBytes / kDescRowsMax) & ~15ll;  // 8388592: whole 16-byte pieces
constexpr int kBf16SeedMaxNs = 4096;  // the bf16 seed's sample (default kSeedMaxNs; PMM_SEED_NS up to this)
inline bool seed_span_fits(int64_t ns, int64_t ld, int elem) { return ns * ld * elem <= kDescMaxBytes; }
// f32 seeded prologue: the form of its seed blocks for this sample (the
// environment read per call): 0 fmaf chains, 1 LDS-staged, 2 MFMA
int seeded_prologue_form(int64_t n, int dp, int ns);
// The fused top-k's prologue with threshold seeding in one launch: the seed
// (the sample's scores as fmaf chains, bit-identical to the fused kernel's,
// with its own norms; writes every row's gthr), the query norms (and the
// corpus norms when corpus_norms), and zeroing [z0, +z0_bytes) and [z1,
// +z1_bytes).  Padded dp <= kSeedDotsMaxD.
constexpr int kSeedDotsMaxD = 2048;
hipError_t launch_seeded_prologue(const float *q, int64_t ldq, int m, const float *c, int64_t ldc, int64_t n,
                                  int d, int dp, int ns, int k, int metric, float *qn, float *cn, bool corpus_norms,
                                  unsigned long long *gthr, void *z0, size_t z0_bytes, void *z1, size_t z1_bytes,
                                  hipStream_t s);
hipError_t launch_seed_select(const float *S, int64_t lds, int m, int ns, int k, int metric,
                              unsigned long long *gthr, hipStream_t s);
// ---- bf16 compute path (pmm_bf16.hip) ----
// Fused top-k on bf16 operands: 128 query rows x 128 corpus columns per
// workgroup tile, 4 waves (1 per SIMD), query rows register-resident.
constexpr int kBf16BM = 128, kBf16BN = 128, kBf16NW = 4;
constexpr int kBf16MaxD = 768;  // padded D (multiple of kBf16DAlign) limit: registers
constexpr int kBf16DAlign = 128;
constexpr int kBf16MaxCapg = 1024;  // LDS budget for the compaction scratch (k <= 960)
hipError_t launch_gemm_bf16(const GemmF32Args &a, int grid, hipStream_t s);
size_t gemm_bf16_lds_bytes(int capg, int nst);
// Wave-specialised bf16 kernel (pmm_bf16_ws_kernel.h): 128 query rows x 64
// corpus columns per tile, 4 MFMA waves + 4 epilogue waves.  Used when its
// LDS (compaction scratch included) fits: capg <= kBf16WsMaxCapg.
constexpr int kBf16WsBN = 64;
constexpr int kBf16WsMaxCapg = 512;
size_t gemm_bf16_ws_lds_bytes(int capg, int D);  // D = padded dimension
// screen: the conservative-screen form of the kernel (cosine only; a.eps, a.ovf)
hipError_t launch_gemm_bf16_ws(const GemmF32Args &a, int grid, hipStream_t s, bool screen = false);
// bf16 threshold seed (pmm_bf16_ws_kernel.h): S[row][0..ns) = the scores of
// corpus rows 0..ns-1 exactly as the wave-specialised kernel computes them
hipError_t launch_seed_bf16_ws(const GemmF32Args &a, float *S, int ns, hipStream_t s);
// 256-query-row bf16 kernel on v_mfma_f32_16x16x32_bf16 with survivors stored
// fire-and-forget against a static guessed threshold (pmm_bf16_ff_kernel.h):
// 64 rows x D per wave, 32-column corpus tiles.  N < 2^26.
constexpr int kBf16FfBM = 256, kBf16FfBN = 32;
static_assert(kBf16BN <= kDescRowsMax && kBf16WsBN <= kDescRowsMax && kBf16FfBN <= kDescRowsMax &&
                  kBf16FfBM / 4 <= kDescRowsMax,
              "a bf16 kernel's descriptor spans one corpus tile or one wave's query rows");
size_t gemm_bf16_ff_lds_bytes(int D);  // D = padded dimension; 0 if unsupported
hipError_t launch_gemm_bf16_ff(const GemmF32Args &a, int grid, hipStream_t s);
// Exact re-score and bucketing of the ff kernel's survivor regions into the
// per-(row, split) candidate lists of merge_kernel: one workgroup per (query
// block, wave); rows whose lists overflowed, whose region overflowed or that
// kept fewer than k candidates at or above their threshold go to fb_rows
// (*fb_count of them) for a re-run.
hipError_t launch_ff_bucket(const GemmF32Args &a, unsigned *fb_count, int *fb_rows, hipStream_t s);
// f32 rows -> bf16 (round to nearest even) with row stride ldd, columns
// d..ldd-1 zero-filled.
hipError_t launch_f32_to_bf16(const float *src, int64_t rows, int64_t d, int64_t lds, uint16_t *dst,
                              int64_t ldd, hipStream_t s);
// The same rounding and, in the same pass, the rows' norms of both metrics:
// norm = sqrt(sum), inv_norm = the cosine pre-filter factor, sq = sum,
// sq_factor = the euclidean one, all from one sum of squares of the ROUNDED
// values in norms_rows' order -- bit-equal to launch_f32_to_bf16 followed by
// launch_norms_bf16 with squared = 0 and 1.  A null array is skipped.  lds >= d
// (any alignment; 16-byte loads when src and lds allow), ldd >= d a multiple
// of 8, dst 16-byte aligned.
hipError_t launch_round_norms_bf16(const float *src, int64_t rows, int64_t d, int64_t lds, uint16_t *dst,
                                   int64_t ldd, float *norm, float *inv_norm, float *sq, float *sq_factor,
                                   hipStream_t s);
// bf16 rows -> f32 rows (exact), columns d..ldd-1 zero-filled
hipError_t launch_bf16_to_f32(const uint16_t *src, int64_t rows, int64_t d, int64_t lds, float *dst, int64_t ldd,
                              hipStream_t s);
hipError_t launch_norms_bf16(const uint16_t *a, int64_t rows, int64_t d, int64_t ld, int squared,
                             float *out, float *inv, hipStream_t s);
size_t merge_lds_bytes_per_wave(int P);
// ---- screened f32 top-k (cosine): bf16 screen + exact f32 re-score ----
// One pass over f32 rows (pmm_bf16.hip): the bf16 image (RNE, row stride ldd,
// columns d..ldd-1 zero), per row an upper bound of ||x - bf16(x)|| / ||x|| in
// rel[] and an "unsafe" flag in bad[] (non-finite or out-of-window element, or
// a norm at or below the reference's 1e-6 rule), AND the rows' exact cosine
// norms and pre-filter factors (launch_norms_f32's bits, squared = 0).  With
// `scal`: scal[0] takes the maximum rel over the safe rows (float bits),
// scal[1] is set when any row is unsafe (the corpus form); both zeroed by the
// caller.  A null array is skipped.  lds >= d (any alignment; 16-byte loads
// when src and lds allow), ldd >= d a multiple of 8, dst 16-byte aligned.
hipError_t launch_screen_prepare(const float *src, int64_t rows, int64_t d, int64_t lds, uint16_t *dst, int64_t ldd,
                                 float *norm, float *inv_norm, float *rel, unsigned *bad, unsigned *scal,
                                 hipStream_t s);
// eps[row] from rel[row] and the corpus scalar; with `seeded` the rows' bf16
// seed thresholds in gthr are lowered by eps into bounds of the exact k-th
hipError_t launch_screen_prep(const float *rel, const unsigned *scal, int m, int dp, float *eps,
                              unsigned long long *gthr, int seeded, hipStream_t s);
struct ScreenFinishArgs {
  const float *q, *c;
  int64_t ldq, ldc;
  const float *qn, *cn, *eps;
  int M, N, dp, S, capg, k;
  unsigned long long *cand;
  const unsigned *cnt;
  const unsigned long long *gthr;
  // optional: [0] += candidates re-scored (rows gathered), [1] = max per row,
  // [2] += entries at or above the published bound - eps (one pass's gathers)
  unsigned *stat;
  // optional (with ovf): the rows' guessed starting bounds.  A row whose
  // proven bound (gthr) stayed below its guess is finished only if the k best
  // approximate entries' exact scores all reach the guess; otherwise ovf[row]
  // = kScreenGuessMissed (unless already set) and the row is re-run.
  const uint32_t *guess;
  unsigned *ovf;
};
constexpr unsigned kScreenGuessMissed = 2u;  // ovf[row]: 1 = the band outgrew the segment
// guess[row] = a bound of row's exact k-th extrapolated from its ns sample
// scores S[row][0 .. ns) (mean + z standard deviations, lowered by eps[row]);
// 0 = no guess; the score key (high word) of the composite.  ns <= 4096.
hipError_t launch_screen_guess(const float *S, int m, int ns, float z, const float *eps, uint32_t *guess,
                               hipStream_t s);
// every kept candidate's approximate key replaced by its exact composite (the
// f32 path's fmaf chain and epilogue); entries below the bound dropped -- the
// published one lowered by eps, raised to (the exact k-th of the k best
// approximate entries) - eps once those are scored
hipError_t launch_screen_rescore(const ScreenFinishArgs &a, hipStream_t s);
// rows[0 .. *count) = the rows with ovf[row] | bad[row] set; count[1] += the overflowed
// ones, count[5] += those whose guessed bound was not confirmed (kScreenGuessMissed)
hipError_t launch_screen_collect(const unsigned *ovf, const unsigned *bad, int m, unsigned *count, int *rows,
                                 hipStream_t s);
// cosine and dot lists: +0.0 scores whose reference value is -0.0 get their
// sign back (the selection keys fold the two zeros); euclidean: nothing.  The
// norms are read for cosine only.  qrow (f32, may be NULL): list row i belongs
// to row qrow[i] of q and qn (probed search: several lists per query row).
hipError_t launch_zero_sign_f32(const float *q, int64_t ldq, const float *c, int64_t ldc, const float *qn,
                                const float *cn, int m, int64_t n, int d, int k, int metric, uint32_t index_base,
                                const uint32_t *out_idx, float *out_score, hipStream_t s,
                                const uint32_t *qrow = nullptr);
hipError_t launch_zero_sign_f64(const double *q, int64_t ldq, const double *c, int64_t ldc, const double *qn,
                                const double *cn, int m, int64_t n, int d, int k, int metric, uint32_t index_base,
                                const uint32_t *out_idx, double *out_score, hipStream_t s);
// after a k-way merge of f32 lists (which folds the zeros again): a merged
// +0.0 takes the zero its entry has in the input lists (strides as MergeArgs')
hipError_t launch_zero_sign_lists(const uint32_t *in_idx, const float *in_score, int lists, int k_in,
                                  int64_t row_stride, int64_t list_stride, int m, int k, const uint32_t *out_idx,
                                  float *out_score, hipStream_t s);
// ---- re-runs of listed rows (the screen's, the ff kernel's) ----
// dst row i (units 16-byte units, dense) = src row rows[i] (row stride
// ld_units 16-byte units); both 16-byte aligned
hipError_t launch_gather_rows(const void *src, int64_t ld_units, const int *rows, int r, int units, void *dst,
                              hipStream_t s);
// out_idx / out_score row rows[i] = the dense lists' row i (k entries each)
hipError_t launch_scatter_lists(const uint32_t *oi, const float *os, const int *rows, int r, int k,
                                uint32_t *out_idx, float *out_score, hipStream_t s);
// ---- derived corpus handles: subset search (pmm_subset.hip) ----
// Bitmap compaction.  words: the bitmap as 64-bit words from the byte that
// holds bit 0 of the selection (8-byte aligned, cdiv(n + shift, 64) + 1 words
// readable), shift = the first bit's position in that byte (0..7): row r is
// selected iff bit shift + r is set, r < n.  One 256-thread block takes
// kMaskBlockRows rows, a lane one word of 64.
constexpr int kMaskBlockRows = 256 * 64;
// launch one: counts[b] = selected rows of block b
hipError_t launch_mask_count(const unsigned long long *words, int shift, int64_t n, uint32_t *counts,
                             hipStream_t s);
// the one-block scan between the two: bases[b] = counts[0] + .. + counts[b - 1], bases[nblk] = the total
hipError_t launch_mask_scan(const uint32_t *counts, int64_t nblk, uint32_t *bases, hipStream_t s);
// launch two: out[bases[b] ..] = block b's selected rows, ascending (so all of out is)
hipError_t launch_mask_write(const unsigned long long *words, int shift, int64_t n, const uint32_t *bases,
                             uint32_t *out, hipStream_t s);
// dst row i (units 16-byte units, dense) = src row ids[i] (row stride the
// same units), i < s: one wave per destination row, four rows in flight per
// wave.  In the same launch the na (<= 4) per-row arrays of aux_bytes-wide
// (4 or 8) elements: aux_dst[a * s + i] = aux_src[a * n_src + ids[i]].  With
// `any` and flag_arr >= 0: *any = 1 when a gathered element of array flag_arr
// is non-zero (4-byte elements; zeroed by the caller).
hipError_t launch_subset_gather(const void *src, const uint32_t *ids, int64_t s, int units, void *dst,
                                const void *aux_src, void *aux_dst, int na, int aux_bytes, int64_t n_src,
                                int flag_arr, unsigned *any, hipStream_t st);
// idx[t] = map[idx[t]] for t < count; entries at or above s (the empty slot 0xFFFFFFFF) stay
hipError_t launch_remap_index(uint32_t *idx, int64_t count, const uint32_t *map, int64_t s, hipStream_t st);
// ---- grouped search (pmm_grouped.hip) ----
// The grouped f32 kernel's limits: list length, padded dimension (its 16 query
// rows and a row's candidate keys live in LDS), query rows per work unit.
constexpr int kGroupedMaxK = 128;
constexpr int kGroupedMaxDp = 1024;
constexpr int kGroupedRows = 16;
// One work unit = one workgroup: partition rows [c0, c0 + ng) of one group
// against rows [q0, q0 + mq) of the label-grouped queries, 1 <= mq <= kGroupedRows.
struct GroupedUnit {
  uint32_t c0, ng, q0, mq;
};
struct GroupedArgs {
  const float *q;            // the queries grouped by label (row stride ldq, zero-padded to dp)
  const float *c;            // the partitioned handle's rows (row stride ldc)
  const float *qn, *cn;      // cosine: norms, euclidean: squared norms (per grouped query / partition row); dot: unused
  int64_t ldq, ldc;
  int dp, k;                 // dp % 32 == 0, dp <= kGroupedMaxDp; 1 <= k <= kGroupedMaxK
  const GroupedUnit *units;  // device table, one entry per workgroup
  uint32_t *out_idx;         // [grouped rows][k]: partition-row numbers, best first, padded
  float *out_score;
  // The row table (probed search, the kernel's ROWTAB variant; NULL: the grouped
  // entry's layout above).  A unit's rows [q0, q0 + mq) are then slots of the
  // label-sorted (query row, label) slots: slot s reads row qrow[s] of q -- the
  // uploaded queries as they are -- and norm qn[qrow[s]], and writes list s.
  const uint32_t *qrow;
};
size_t grouped_lds_bytes(int dp);
// (a.qrow set: one launch of the row-table variant, Timed as probed_topk_f32)
hipError_t launch_grouped_topk_f32(const GroupedArgs &a, int units, int metric, hipStream_t s);
// di / ds rows of k entries = the dense rows x kg lists si / ss, padded (index 0xFFFFFFFF, score 0)
hipError_t launch_grouped_pad(const uint32_t *si, const void *ss, int rows, int kg, int k, uint32_t *di, void *ds,
                              bool f64, hipStream_t s);
// out row qrow[i] = grouped row i's list with its indices (< n) mapped through
// `map` and the slots past glen[i] padded; out_len[qrow[i]] = glen[i]
hipError_t launch_grouped_scatter(const uint32_t *gi, const void *gs, const uint32_t *qrow, const uint32_t *glen,
                                  int64_t rows, int k, const uint32_t *map, uint32_t n, uint32_t *out_idx,
                                  void *out_score, uint32_t *out_len, bool f64, hipStream_t s);
// ---- probed search (pmm_probed.hip) ----
// The merge of a query row's per-slot lists (probe_merge_f32_kernel): row i's
// lists are the slots row_slots[row_off[i] .. row_off[i + 1]) of in_idx /
// in_score (k entries each, partition rows, best first, padded with index
// 0xFFFFFFFF); out row i = the best k of them under okey32(rank value) << 32 |
// ~map[partition row], in the parent's numbering, padded, with its length.
struct ProbeMergeArgs {
  const uint32_t *in_idx;     // [slots][k]
  const float *in_score;      // [slots][k]
  const uint32_t *row_off;    // [m + 1]
  const uint32_t *row_slots;  // [slots]
  const uint32_t *map;        // [n]: partition row -> parent row
  uint32_t n;
  int m, k;                   // 1 <= k <= kGroupedMaxK
  uint32_t *out_idx;          // [m][k]
  float *out_score;           // [m][k]
  uint32_t *out_len;          // [m]
};
hipError_t launch_probe_merge_f32(const ProbeMergeArgs &a, int metric, hipStream_t s);
// the grouped kernel's row-table variant (a.qrow set); launch_grouped_topk_f32 checks the arguments and calls it
hipError_t launch_grouped_rowtab(const GroupedArgs &a, int units, int metric, hipStream_t s);
hipError_t launch_gemm_f64_store(const double *q, int64_t ldq, const double *c, int64_t ldc,
                                 const double *qn, const double *cn, int M, int N, int D,
                                 int metric, int store_metric, double *out, int64_t ldo,
                                 hipStream_t s);
hipError_t launch_rowselect(const RowSelArgs &a, hipStream_t s);
// ---- fused f64 top-k (pmm_f64.hip) ----
struct Ent;
struct F64TopkArgs {
  const double *q;           // this launch's rows (row stride ldq)
  const double *c;           // the whole corpus (row stride ldc)
  const double *qn, *cn;     // cosine: norms, euclidean: squared norms (qn: this launch's rows)
  int64_t ldq, ldc;
  int M, D;                  // rows; padded K (multiple of 16)
  int col0, ncol;            // corpus columns [col0, col0 + ncol) of this chunk
  int metric;
  const unsigned long long *tkey;  // [M] row threshold: the k-th entry (key, index); (0, ~0) = accept all
  const uint32_t *tidx;
  unsigned *cnt;             // [M] buffer counts
  Ent *cand;                 // [M][cap] candidate buffers
  int cap;
  int accept_all;            // first chunk (ncol <= cap): every element at slot = its chunk column
};
struct F64SelArgs {
  Ent *cand;
  unsigned *cnt;
  int cap, M, k, P;          // P: LDS entries per wave, a power of two >= cap
  int mode;                  // 0: keep the best k + raise the thresholds; 1: write the final lists
  unsigned long long *tkey;
  uint32_t *tidx;
  int metric;
  uint32_t index_base;
  uint32_t *out_idx;
  double *out_score;
  unsigned *overflow;        // set when a row's count exceeded cap (entries were dropped)
};
// k-way merge of G (<= 64) sorted f64 top-k lists per row: entry i of list g
// of row r at gi / gs[g * list_stride + r * k + i]
struct F64MergeArgs {
  const uint32_t *gi;
  const double *gs;
  int64_t list_stride;
  int M, G, k, metric;
  uint32_t *out_idx;    // [M][k]
  double *out_score;
};
hipError_t launch_f64_merge(const F64MergeArgs &a, hipStream_t s);
hipError_t launch_gemm_f64_topk(const F64TopkArgs &a, hipStream_t s);
hipError_t launch_f64_select(const F64SelArgs &a, hipStream_t s);
hipError_t launch_f64_reset(unsigned long long *tkey, uint32_t *tidx, unsigned *cnt, int m, unsigned cnt0,
                            hipStream_t s);
// ---- int8 top-k (pmm_i8.hip) ----
// Rows of signed bytes at a stride that is a multiple of kI8DAlign bytes,
// zero-padded.  The int8 MFMA scan takes a padded d up to kI8MaxD (the range
// its tests pin; its K loop has no register limit) and k up to kFusedMaxK (the
// candidate buffers); past either the rows are widened to f64 on the device
// and searched by the f64 path.  d < kI8DimLimit keeps a row's sum of squares
// and a squared distance in u32 and a dot in i32.
constexpr int kI8DAlign = 64;
constexpr int kI8MaxD = 2048;
constexpr int kI8DimLimit = 1 << 16;
// The cosine key's distance from the f64 score (DESIGN.md §4d "Int8 rows"): five f32
// roundings of a value of magnitude at most 1, 5.001 * 2^-24 < 2^-21.
constexpr float kI8CosEps = 0x1p-21f;
struct I8TopkArgs {
  const int8_t *q;           // this launch's rows (row stride ldq bytes)
  const int8_t *c;           // the whole corpus (row stride ldc bytes)
  const uint32_t *qs, *cs;   // integer sums of squares (qs: this launch's rows)
  const float *qf, *cf;      // f32(1 / sqrt(sum)), 0 for a zero row
  int64_t ldq, ldc;
  int M, D;                  // rows; padded K (a multiple of kI8DAlign)
  int col0, ncol;            // corpus columns [col0, col0 + ncol) of this chunk
  int metric;
  const uint32_t *tkey;      // [M] row threshold: an element is appended iff (key, lower index)
  const uint32_t *tidx;      // beats (tkey, tidx); (0, ~0) = accept all
  unsigned *cnt;             // [M] buffer counts
  Ent *cand;                 // [M][cap]: key << 32, corpus row, the exact dot in `pad`
  int cap;
};
struct I8SelArgs {
  Ent *cand;
  unsigned *cnt;
  int cap, M, k, P;          // P: LDS entries per wave, a power of two >= cap
  uint32_t *tkey, *tidx;
  unsigned *ovf;             // [M] set when a row's count exceeded cap (entries were dropped)
  int metric;
  // the finish
  const uint32_t *qs, *cs;
  uint32_t index_base;
  uint32_t *out_idx;         // [M][k]
  double *out_score;
};
hipError_t launch_i8_norms(const int8_t *a, int64_t rows, int64_t ld, int dp, uint32_t *sq, float *fac,
                           hipStream_t s);
hipError_t launch_gemm_i8_topk(const I8TopkArgs &a, hipStream_t s);
hipError_t launch_i8_select(const I8SelArgs &a, hipStream_t s);
hipError_t launch_i8_finish(const I8SelArgs &a, hipStream_t s);
hipError_t launch_i8_reset(uint32_t *tkey, uint32_t *tidx, unsigned *cnt, unsigned *ovf, int m, hipStream_t s);
// rows[old *count ..) = base + r for every r < m with ovf[r] set; *count grows by their number
hipError_t launch_i8_collect(const unsigned *ovf, int m, int base, unsigned *count, int *rows, hipStream_t s);
// dst row i (ldd doubles, columns d .. ldd - 1 zero) = src row (rows ? rows[i] : i), widened exactly
hipError_t launch_i8_widen(const int8_t *src, int64_t ld, const int *rows, int64_t r, int d, double *dst,
                           int64_t ldd, hipStream_t s);
hipError_t launch_i8_scatter(const uint32_t *oi, const double *os, const int *rows, int64_t r, int k,
                             uint32_t *out_idx, double *out_score, hipStream_t s);
// ---- bit rows (pmm_bits.hip) ----
// Packed rows of w bytes (bit j = (byte[j >> 3] >> (j & 7)) & 1) at a stride
// that is a multiple of kBitsAlign bytes, zero-padded: the search kernel's
// staging group.  The MFMA scan takes w up to kBitsMaxW (no wider row is
// served) and k up to kFusedMaxK; past that k both sides are expanded to 0/1
// f64 rows and searched by the f64 path.  The scan reuses I8TopkArgs /
// I8SelArgs with the euclidean key, D in packed bytes and qs / cs the rows'
// popcounts, and launch_i8_select / _reset / _collect as they are.
constexpr int kBitsAlign = 16;
constexpr int kBitsMaxW = 8192;
// rows of roundup(ceil(d / 8), 8) bytes written whole (ld_out a multiple of 8, out 8-byte aligned); pop optional
hipError_t launch_pack_sign(const float *x, int64_t ldx, int64_t rows, int d, uint8_t *out, int64_t ld_out,
                            uint32_t *pop, hipStream_t s);
// pop[r] = the popcount of the first dp bytes (a multiple of 16) of row r
hipError_t launch_bits_popcount(const uint8_t *a, int64_t rows, int64_t ld, int dp, uint32_t *pop, hipStream_t s);
hipError_t launch_gemm_bits_topk(const I8TopkArgs &a, hipStream_t s);
// the lists of buffer rows 0 .. a.M - 1 to output rows rows[r] (nullptr: r), scores the integer distances
hipError_t launch_bits_finish(const I8SelArgs &a, const int *rows, hipStream_t s);
hipError_t launch_bits_gather(const uint8_t *src, int64_t ld, const int *rows, int64_t r, uint8_t *dst, int64_t ldd,
                              const uint32_t *ps, uint32_t *pd, hipStream_t s);
hipError_t launch_bits_widen(const uint8_t *src, int64_t ld, int64_t r, int w, double *dst, int64_t ldd,
                             hipStream_t s);
hipError_t launch_bits_square(double *score, int64_t total, hipStream_t s);
// full-row sort fallback for very large k
hipError_t launch_rowsort_global(const void *scores, int64_t lds, int rows, int N, int is_f64,
                                 int metric, void *keys_ws, int P2, int k, uint32_t index_base,
                                 uint32_t *out_idx,
                                 void *out_score, hipStream_t s);

}  // namespace pmm
