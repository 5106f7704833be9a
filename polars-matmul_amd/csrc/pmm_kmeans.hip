// pmm_kmeans.hip -- kernels of k-means clustering on a resident f32 handle
// (pmm_kmeans_f32_corpus; DESIGN.md §4d "k-means").  No reference counterpart.
// The assignment is the fused f32 top-1 (pmm_kernels.hip) with the centroids
// as the corpus; here are the passes around it:
//   labels   [n][1] lists -> labels, scores and the changed flag;
//   ordering a stable LSD radix sort of the row numbers by label (8-bit digits,
//            one wave per run of kKmeansSortRows rows), so every cluster's
//            members stand in ascending row order; bounds by binary search;
//            the clusters' pieces of kKmeansPiece members by one scan;
//   update   one wave per (piece, 256 columns): the members' rows read whole,
//            eight in flight, summed in f64 registers in member order;
//   finish   the pieces of a cluster added in piece order, divided, rounded.
// Plain vector loads and stores; LDS counters in the sort; no scratch, no
// global atomics: the sums do not depend on the launch geometry.
#include "pmm_internal.h"

namespace pmm {

namespace {

constexpr int kWave = 64;
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;  // PMM_NO_GROUP
constexpr int kSortRounds = kKmeansSortRows / kWave;
constexpr int kUpdateRows = 8;    // member rows in flight per wave
constexpr int kUpdateCols = 256;  // columns per wave: one float4 per lane

// exclusive prefix sum of a block of 1024 threads' values; *total = their sum
__device__ inline uint32_t block_exclusive(uint32_t v, uint32_t *wsum, uint32_t *total) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t x = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += x;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t x = wsum[j];
    before += j < wv ? x : 0u;
    all += x;
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

}  // namespace

__global__ __launch_bounds__(256) void kmeans_labels_kernel(const uint32_t *__restrict__ oi,
                                                            const float *__restrict__ os, int64_t n, uint32_t K,
                                                            uint32_t *__restrict__ labels, float *__restrict__ scores,
                                                            int have_prev, unsigned *__restrict__ changed) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    float s = os[i];
    uint32_t l = oi[i];
    if (s != s) {
      l = kNoLabel;
      s = __uint_as_float(0x7FC00000u);
    } else if (l >= K) {
      l = kNoLabel;  // (an empty slot: never with k = 1 <= K)
    }
    if (have_prev && labels[i] != l) *changed = 1u;  // (every writer stores the same word)
    labels[i] = l;
    scores[i] = s;
  }
}

// hist[digit * units + u] = the rows of run u whose key has that digit
__global__ __launch_bounds__(256) void kmeans_sort_hist_kernel(const uint32_t *__restrict__ keys, uint32_t K,
                                                               int shift, int64_t n, int64_t units,
                                                               uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[4][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * 4 + wv;
  for (int j = lane; j < 256; j += kWave) h[wv][j] = 0u;
  __syncthreads();
  for (int r = 0; r < kSortRounds; r++) {
    const int64_t i = u * kKmeansSortRows + r * kWave + lane;
    if (u < units && i < n) atomicAdd(&h[wv][(min(keys[i], K) >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (u < units)
    for (int j = lane; j < 256; j += kWave) hist[(int64_t)j * units + u] = h[wv][j];
}

// out[i] = in[0] + .. + in[i - 1], one block, eight entries per thread and step
__global__ __launch_bounds__(1024) void kmeans_scan_kernel(const uint32_t *__restrict__ in, int64_t count,
                                                           uint32_t *__restrict__ out) {
  __shared__ uint32_t wsum[16];
  uint32_t carry = 0;
  for (int64_t i0 = 0; i0 < count; i0 += 8192) {
    const int64_t i = i0 + (int64_t)threadIdx.x * 8;
    uint32_t v[8], sum = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      v[e] = i + e < count ? in[i + e] : 0u;
      sum += v[e];
    }
    uint32_t total;
    uint32_t run = carry + block_exclusive(sum, wsum, &total);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      if (i + e < count) out[i + e] = run;
      run += v[e];
    }
    carry += total;
  }
}

// One stable pass: the rows of run u go, in their order, to the places that
// start at base[digit * units + u].  A lane's place inside its round is the
// number of lower lanes with its digit (the ballots), the run's next free
// place of every digit sits in LDS.  vals == nullptr: the row numbers.
__global__ __launch_bounds__(256) void kmeans_sort_scatter_kernel(const uint32_t *__restrict__ keys,
                                                                  const uint32_t *__restrict__ vals, uint32_t K,
                                                                  int shift, int64_t n, int64_t units,
                                                                  const uint32_t *__restrict__ base,
                                                                  uint32_t *__restrict__ keys_out,
                                                                  uint32_t *__restrict__ vals_out) {
  __shared__ uint32_t off[4][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * 4 + wv;
  if (u < units)
    for (int j = lane; j < 256; j += kWave) off[wv][j] = base[(int64_t)j * units + u];
  __syncthreads();
  for (int r = 0; r < kSortRounds; r++) {  // (every wave of the block runs every round: the barriers)
    const int64_t i = u * kKmeansSortRows + r * kWave + lane;
    const bool valid = u < units && i < n;
    const uint32_t key = valid ? min(keys[i], K) : 0u;
    const uint32_t val = valid ? (vals ? vals[i] : (uint32_t)i) : 0u;
    const uint32_t dg = (key >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (dg >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    const uint32_t pos = off[wv][dg] + rank;
    __syncthreads();
    if (valid && rank == 0) off[wv][dg] += (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid && pos < (uint64_t)n) {
      keys_out[pos] = key;
      vals_out[pos] = val;
    }
  }
}

// bounds[c] = the first place of the sorted keys that holds c or more, c <= K
__global__ __launch_bounds__(256) void kmeans_bounds_kernel(const uint32_t *__restrict__ skeys, int64_t n,
                                                            uint32_t K, uint32_t *__restrict__ bounds) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > (int64_t)K) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (skeys[mid] < (uint32_t)c) lo = mid + 1;
    else hi = mid;
  }
  bounds[c] = (uint32_t)lo;
}

// pbase[c] = the pieces of the clusters below c; pbase[K] = all pieces
__global__ __launch_bounds__(1024) void kmeans_pieces_kernel(const uint32_t *__restrict__ bounds, uint32_t K,
                                                             uint32_t *__restrict__ pbase) {
  __shared__ uint32_t wsum[16];
  uint32_t carry = 0;
  for (int64_t c0 = 0; c0 < (int64_t)K; c0 += 1024) {
    const int64_t c = c0 + threadIdx.x;
    const uint32_t v = c < (int64_t)K ? (bounds[c + 1] - bounds[c] + (kKmeansPiece - 1)) / kKmeansPiece : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive(v, wsum, &total);
    if (c < (int64_t)K) pbase[c] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) pbase[K] = carry;
}

// One wave per (piece g, columns [256 ch, 256 ch + 256)): psum[g][those] = the
// f64 sum of the piece's members' terms, from +0.0 in member order; the wave of
// ch = 0 also writes pcount[g], the members that added a term.
template <bool kCos>
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float *__restrict__ x, int64_t ldx,
                                                            const float *__restrict__ cn,
                                                            const uint32_t *__restrict__ rows,
                                                            const uint32_t *__restrict__ bounds,
                                                            const uint32_t *__restrict__ pbase, uint32_t K, int dp,
                                                            int nchunks, int64_t nwaves, double *__restrict__ psum,
                                                            uint32_t *__restrict__ pcount) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nwaves) return;  // (the whole wave)
  const uint32_t g = (uint32_t)(w / nchunks);
  const int ch = (int)(w % nchunks);
  if (g >= pbase[K]) return;
  // the piece's cluster: the last c with pbase[c] <= g (an empty cluster has no piece)
  uint32_t lo = 0, hi = K;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pbase[mid] <= g) lo = mid;
    else hi = mid;
  }
  const uint32_t m0 = bounds[lo] + (g - pbase[lo]) * (uint32_t)kKmeansPiece;
  const uint32_t m1 = min(m0 + (uint32_t)kKmeansPiece, bounds[lo + 1]);
  const int col = ch * kUpdateCols + lane * 4;
  const bool active = col < dp;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  uint32_t counted = 0;
  for (uint32_t m = m0; m < m1; m += kUpdateRows) {
    float4 v[kUpdateRows];
    float nr[kUpdateRows];
#pragma unroll
    for (int j = 0; j < kUpdateRows; j++) {
      // (past the piece's end: its last member again, loaded and not added)
      const uint32_t rid = (uint32_t)__builtin_amdgcn_readfirstlane((int)rows[min(m + j, m1 - 1)]);
      v[j] = active ? *(const float4 *)(x + (int64_t)rid * ldx + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      nr[j] = kCos ? cn[rid] : 1.0f;
    }
#pragma unroll
    for (int j = 0; j < kUpdateRows; j++) {
      if (m + j >= m1) break;
      if (kCos) {
        if (nr[j] <= 1e-6f) continue;  // the reference's zero-norm rule
        const double dn = (double)nr[j];
        a0 += (double)v[j].x / dn;
        a1 += (double)v[j].y / dn;
        a2 += (double)v[j].z / dn;
        a3 += (double)v[j].w / dn;
      } else {
        a0 += (double)v[j].x;
        a1 += (double)v[j].y;
        a2 += (double)v[j].z;
        a3 += (double)v[j].w;
      }
      counted++;
    }
  }
  if (active) {
    double2 *p = (double2 *)(psum + (int64_t)g * dp + col);
    p[0] = make_double2(a0, a1);
    p[1] = make_double2(a2, a3);
  }
  if (ch == 0 && lane == 0) pcount[g] = counted;
}

// C[c][j] = (float)(the cluster's piece sums added in piece order from +0.0 /
// its counted members); a cluster that counted none keeps its row; the padded
// columns are +0.0
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double *__restrict__ psum,
                                                            const uint32_t *__restrict__ pcount,
                                                            const uint32_t *__restrict__ pbase, int d, int dp,
                                                            int nchunks, float *__restrict__ C) {
  const int64_t c = blockIdx.x / nchunks;
  const int j = (int)(blockIdx.x % nchunks) * 256 + threadIdx.x;
  if (j >= dp) return;
  if (j >= d) {
    C[c * dp + j] = 0.0f;
    return;
  }
  const uint32_t p0 = pbase[c], p1 = pbase[c + 1];
  uint32_t count = 0;
  double sum = 0.0;
  for (uint32_t p = p0; p < p1; p++) {
    count += pcount[p];
    sum += psum[(int64_t)p * dp + j];
  }
  if (count > 0) C[c * dp + j] = (float)(sum / (double)count);
}

int64_t kmeans_sort_units(int64_t n) { return (n + kKmeansSortRows - 1) / kKmeansSortRows; }

int kmeans_sort_passes(uint32_t K) {
  int p = 1;  // (the keys are 0 .. K: the rows of no cluster sort last)
  while (p < 4 && (K >> (8 * p)) != 0) p++;
  return p;
}

int64_t kmeans_max_pieces(int64_t n, int64_t K) {
  const int64_t a = n / kKmeansPiece + K;  // (at most one short piece per cluster)
  return a < n ? a : n;
}

hipError_t launch_kmeans_labels(const uint32_t *oi, const float *os, int64_t n, uint32_t K, uint32_t *labels,
                                float *scores, bool have_prev, unsigned *changed, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + 255) / 256;
  kmeans_labels_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, s>>>(
      oi, os, n, K, labels, scores, have_prev ? 1 : 0, changed);
  return hipGetLastError();
}

hipError_t launch_kmeans_order(const KmeansOrder &a, hipStream_t s) {
  if (a.n <= 0 || a.n > INT32_MAX) return hipErrorInvalidValue;
  const int64_t units = kmeans_sort_units(a.n);
  const unsigned grid = (unsigned)((units + 3) / 4);
  const int passes = kmeans_sort_passes(a.K);
  const uint32_t *keys = a.labels, *vals = nullptr;
  for (int p = 0; p < passes; p++) {
    kmeans_sort_hist_kernel<<<grid, 256, 0, s>>>(keys, a.K, 8 * p, a.n, units, a.hist);
    kmeans_scan_kernel<<<1, 1024, 0, s>>>(a.hist, 256 * units, a.base);
    kmeans_sort_scatter_kernel<<<grid, 256, 0, s>>>(keys, vals, a.K, 8 * p, a.n, units, a.base, a.key[p & 1],
                                                    a.val[p & 1]);
    keys = a.key[p & 1];
    vals = a.val[p & 1];
  }
  kmeans_bounds_kernel<<<(unsigned)(((int64_t)a.K + 1 + 255) / 256), 256, 0, s>>>(keys, a.n, a.K, a.bounds);
  kmeans_pieces_kernel<<<1, 1024, 0, s>>>(a.bounds, a.K, a.pbase);
  return hipGetLastError();
}

const uint32_t *kmeans_sorted_rows(const KmeansOrder &a) { return a.val[(kmeans_sort_passes(a.K) - 1) & 1]; }

hipError_t launch_kmeans_update(const KmeansUpdateArgs &a, hipStream_t s) {
  const int nchunks = (a.dp + kUpdateCols - 1) / kUpdateCols;
  const int64_t nwaves = a.max_pieces * nchunks, blocks = (nwaves + 3) / 4;
  if (a.dp % 32 != 0 || a.ldx % 4 != 0 || blocks > INT32_MAX) return hipErrorInvalidValue;
  if (a.cn)
    kmeans_update_kernel<true><<<(unsigned)blocks, 256, 0, s>>>(a.x, a.ldx, a.cn, a.rows, a.bounds, a.pbase, a.K, a.dp,
                                                                 nchunks, nwaves, a.psum, a.pcount);
  else
    kmeans_update_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(a.x, a.ldx, nullptr, a.rows, a.bounds, a.pbase, a.K,
                                                                  a.dp, nchunks, nwaves, a.psum, a.pcount);
  return hipGetLastError();
}

hipError_t launch_kmeans_finish(const KmeansUpdateArgs &a, hipStream_t s) {
  const int nchunks = (a.dp + 255) / 256;
  const int64_t blocks = (int64_t)a.K * nchunks;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  kmeans_finish_kernel<<<(unsigned)blocks, 256, 0, s>>>(a.psum, a.pcount, a.pbase, a.d, a.dp, nchunks, a.C);
  return hipGetLastError();
}

}  // namespace pmm
