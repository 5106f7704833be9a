// pmm_range.hip -- range search (pmm_range_f32_corpus, pmm_range_f32_self;
// DESIGN.md §4d), with the self top-k's drop-self pass at the end: the
// passes that turn the records the f32 GEMM's range mode emitted (composite
// key + query row, in no order) into per-row, best-first lists.  Bin: every
// key to its row's segment of the CSR layout.  Sort: a segment's keys are
// unique (the column rides in the low word), so sorting them descending gives
// the engine's total order whatever order the records arrived in -- up to 128
// keys in one wave's registers, up to kRangeSortMax in one workgroup's LDS.
// Decode: key -> (index, score) by the top-k epilogue's rules.  No reference
// counterpart (the reference has no range search).
#include "pmm_device.h"

namespace pmm {

__global__ __launch_bounds__(256) void range_bin_kernel(const u64 *__restrict__ rkey,
                                                        const uint32_t *__restrict__ rrow, int64_t total,
                                                        const int64_t *__restrict__ offsets,
                                                        unsigned *__restrict__ cur, u64 *__restrict__ keys) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const uint32_t row = rrow[t];
    const int64_t o = offsets[row], len = offsets[row + 1] - o;
    const int64_t p = (int64_t)atomicAdd(cur + row, 1u);
    if (p < len) keys[o + p] = rkey[t];  // (always: the row's count is its number of records)
  }
}

__global__ __launch_bounds__(256) void range_sort_wave_kernel(u64 *__restrict__ keys,
                                                              const int64_t *__restrict__ offsets, int m) {
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (row >= m) return;  // (the whole wave)
  const int64_t o = offsets[row], n = offsets[row + 1] - o;
  if (n < 2 || n > kRangeWaveMax) return;
  // (a record's key is never 0: empty slots sort last)
  u64 y0 = lane < n ? keys[o + lane] : 0ull;
  u64 y1 = lane + 64 < n ? keys[o + lane + 64] : 0ull;
  wave_sort128_desc(y0, y1, lane);
  if (lane < n) keys[o + lane] = y0;
  if (lane + 64 < n) keys[o + lane + 64] = y1;
}

// Bitonic sort, best first, of one row's segment in LDS: P = the power of two
// at or above its length (<= pmax), the tail padded with 0.
__global__ __launch_bounds__(256) void range_sort_block_kernel(u64 *__restrict__ keys,
                                                               const int64_t *__restrict__ offsets,
                                                               const int *__restrict__ rows, int pmax) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64 *sk = (u64 *)smem;
  const int tid = threadIdx.x;
  const int row = rows[blockIdx.x];
  const int64_t o = offsets[row], n = offsets[row + 1] - o;
  if (n < 2 || n > pmax) return;  // (the whole workgroup)
  int P = 64;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += 256) sk[i] = i < n ? keys[o + i] : 0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (P >> 1); i += 256) {
        const int x0 = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
        const int x1 = x0 + stride;
        const u64 a = sk[x0], b = sk[x1];
        const bool desc = (x0 & size) == 0;
        if (desc ? (a < b) : (a > b)) {
          sk[x0] = b;
          sk[x1] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += 256) keys[o + i] = sk[i];
}

// One thread per list entry.  The score is the key's (a zero euclidean
// distance leaves as +0.0); the keys fold -0 onto +0, so a +0.0 cosine or dot
// product is recomputed by the reference's arithmetic and takes that zero's sign, as
// zero_sign_kernel does for the top-k lists (its row found by bisection of
// the offsets: zero scores are rare).  The index goes through the index map.
__global__ __launch_bounds__(256) void range_decode_kernel(RangeDecodeArgs a) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.total; t += step) {
    const u64 key = a.keys[t];
    const uint32_t col = ~(uint32_t)key;
    const float v = dekey32((uint32_t)(key >> 32));
    float sc = a.metric == kMetricEuclidean ? 0.0f - v : v;
    if (a.metric != kMetricEuclidean && __float_as_uint(sc) == 0u) {
      int lo = 0, hi = a.m;  // offsets[lo] <= t < offsets[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.offsets[mid] <= t) lo = mid;
        else hi = mid;
      }
      const float *qr = a.q + (int64_t)lo * a.ldq, *cr = a.c + (int64_t)col * a.ldc;
      float acc = 0.0f;
      for (int i = 0; i < a.d; i++) acc = fmaf(qr[i], cr[i], acc);
      // (a dot product is its chain: no norms are read)
      const float ex = a.metric == kMetricDot ? acc : exact_score<kMetricCosine>(acc, a.qn[lo], a.cn[col]);
      if (ex == 0.0f) sc = ex;
    }
    a.out_idx[t] = a.map ? a.map[col] : col;
    a.out_score[t] = sc;
  }
}

// Self top-k (pmm_topk_f32_self): row i's ranked (k + 1)-list of the handle's
// rows, searched with the rows themselves as queries, minus row i -- the entry
// whose index is the row's own handle position (the lists are not yet mapped
// to a derived handle's parent numbers), or the last entry when the row is not
// in its list (k + 1 others rank above it).  The ranked list is a total
// order, so what is left is the first k of the row's ranking without itself.
// One wave per row, 64 entries at a time.
__global__ __launch_bounds__(256) void drop_self_kernel(const uint32_t *__restrict__ in_idx,
                                                        const float *__restrict__ in_score, int m, int k,
                                                        uint32_t *__restrict__ out_idx,
                                                        float *__restrict__ out_score) {
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (row >= m) return;  // (the whole wave)
  const uint32_t *ii = in_idx + (int64_t)row * (k + 1);
  const float *is = in_score + (int64_t)row * (k + 1);
  int p = k;  // the place to drop
  for (int j0 = 0; j0 <= k; j0 += 64) {
    const int j = j0 + lane;
    const u64 found = __ballot(j <= k && ii[j] == (uint32_t)row);
    if (found) {
      p = j0 + __builtin_ctzll(found);
      break;
    }
  }
  for (int j = lane; j < k; j += 64) {
    const int src = j + (j >= p ? 1 : 0);
    out_idx[(int64_t)row * k + j] = ii[src];
    out_score[(int64_t)row * k + j] = is[src];
  }
}

// Duplicate groups (pmm_components_f32_self): the union-find forest before
// and after the components pass of the f32 GEMM (MODE 4).  The label pass
// reads with plain loads: the kernel boundary orders them after every link.
__global__ __launch_bounds__(256) void components_init_kernel(uint32_t *__restrict__ parent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void components_label_kernel(const uint32_t *__restrict__ parent,
                                                               const uint32_t *__restrict__ map, int64_t n,
                                                               uint32_t *__restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t x = (uint32_t)i;
  for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
  labels[i] = map ? map[x] : x;
}

static unsigned range_grid(int64_t count) {
  const int64_t blocks = (count + 255) / 256;
  return (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));
}

hipError_t launch_range_bin(const unsigned long long *rkey, const uint32_t *rrow, int64_t total,
                            const int64_t *offsets, unsigned *cur, unsigned long long *keys, hipStream_t s) {
  if (total <= 0) return hipSuccess;
  range_bin_kernel<<<range_grid(total), 256, 0, s>>>(rkey, rrow, total, offsets, cur, keys);
  return hipGetLastError();
}

hipError_t launch_range_sort_wave(unsigned long long *keys, const int64_t *offsets, int m, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  range_sort_wave_kernel<<<(unsigned)((m + 3) / 4), 256, 0, s>>>(keys, offsets, m);
  return hipGetLastError();
}

hipError_t launch_range_sort_block(unsigned long long *keys, const int64_t *offsets, const int *rows, int r,
                                   int pmax, hipStream_t s) {
  if (r <= 0) return hipSuccess;
  if (pmax < 64 || pmax > kRangeSortMax || (pmax & (pmax - 1))) return hipErrorInvalidValue;
  range_sort_block_kernel<<<(unsigned)r, 256, (size_t)pmax * 8, s>>>(keys, offsets, rows, pmax);
  return hipGetLastError();
}

hipError_t launch_range_decode(const RangeDecodeArgs &a, hipStream_t s) {
  if (a.total <= 0) return hipSuccess;
  range_decode_kernel<<<range_grid(a.total), 256, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_drop_self(const uint32_t *in_idx, const float *in_score, int64_t m, int64_t k, uint32_t *out_idx,
                            float *out_score, hipStream_t s) {
  if (m <= 0 || k <= 0) return hipSuccess;
  if (m > INT32_MAX || k >= INT32_MAX) return hipErrorInvalidValue;
  drop_self_kernel<<<(unsigned)((m + 3) / 4), 256, 0, s>>>(in_idx, in_score, (int)m, (int)k, out_idx, out_score);
  return hipGetLastError();
}

hipError_t launch_components_init(uint32_t *parent, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  components_init_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(parent, n);
  return hipGetLastError();
}

hipError_t launch_components_label(const uint32_t *parent, const uint32_t *map, int64_t n, uint32_t *labels,
                                   hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  components_label_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(parent, map, n, labels);
  return hipGetLastError();
}

}  // namespace pmm
