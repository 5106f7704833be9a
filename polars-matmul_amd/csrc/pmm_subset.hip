// pmm_subset.hip -- kernels of the derived corpus handles (subset search,
// pmm_corpus_subset_ids / pmm_corpus_subset_mask): compaction
// of a selection bitmap into ascending row numbers, the gather of the selected
// rows and their per-row arrays, and the remap of a top-k call's indices to
// the parent's numbering.  No reference counterpart (the reference filters on
// the host).  Plain vector loads and stores, no scratch, no atomics.
#include "pmm_internal.h"

namespace pmm {

namespace {

constexpr int kWave = 64;

// rows [64 w, 64 w + 64) of the selection as one word, bit j = row 64 w + j;
// rows at or past n read as unselected
__device__ inline unsigned long long mask_word(const unsigned long long *__restrict__ words, int shift, int64_t w,
                                               int64_t n) {
  const int64_t row0 = w * 64;
  if (row0 >= n) return 0ull;
  unsigned long long v = words[w] >> shift;
  if (shift) v |= words[w + 1] << (64 - shift);
  const int64_t left = n - row0;
  if (left < 64) v &= (1ull << left) - 1ull;
  return v;
}

// inclusive prefix sum over the wave's lanes (every lane takes part)
__device__ inline uint32_t wave_inclusive(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t x = __shfl_up(v, o, kWave);
    if (lane >= o) v += x;
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void mask_count_kernel(const unsigned long long *__restrict__ words, int shift,
                                                         int64_t n, uint32_t *__restrict__ counts) {
  __shared__ uint32_t wsum[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t c = (uint32_t)__popcll(mask_word(words, shift, (int64_t)blockIdx.x * 256 + t, n));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
  if (lane == 0) wsum[wv] = c;
  __syncthreads();
  if (t == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(1024) void mask_scan_kernel(const uint32_t *__restrict__ counts, int64_t nblk,
                                                         uint32_t *__restrict__ bases) {
  __shared__ uint32_t wsum[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t carry = 0;
  for (int64_t i0 = 0; i0 < nblk; i0 += 1024) {
    const int64_t i = i0 + t;
    const uint32_t v = i < nblk ? counts[i] : 0u;
    const uint32_t inc = wave_inclusive(v, lane);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t x = wsum[j];
      before += j < wv ? x : 0u;
      total += x;
    }
    if (i < nblk) bases[i] = carry + before + inc - v;
    carry += total;
    __syncthreads();
  }
  if (t == 0) bases[nblk] = carry;
}

__global__ __launch_bounds__(256) void mask_write_kernel(const unsigned long long *__restrict__ words, int shift,
                                                         int64_t n, const uint32_t *__restrict__ bases,
                                                         uint32_t *__restrict__ out) {
  __shared__ uint32_t wsum[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t w = (int64_t)blockIdx.x * 256 + t;
  unsigned long long v = mask_word(words, shift, w, n);
  const uint32_t c = (uint32_t)__popcll(v);
  const uint32_t inc = wave_inclusive(c, lane);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t off = bases[blockIdx.x] + inc - c;
#pragma unroll
  for (int j = 0; j < 3; j++) off += j < wv ? wsum[j] : 0u;
  // the lane's set bits, lowest first, as row numbers at its offset: within
  // the lane, across the lanes and across the blocks the rows ascend
  const uint32_t row0 = (uint32_t)(w * 64);
  while (v) {
    out[off++] = row0 + (uint32_t)(__ffsll((long long)v) - 1);
    v &= v - 1ull;
  }
}

constexpr int kGatherRows = 4;  // destination rows in flight per wave

template <typename T>
__global__ __launch_bounds__(256) void subset_gather_kernel(const uint4 *__restrict__ src,
                                                            const uint32_t *__restrict__ ids, int64_t s, int units,
                                                            uint4 *__restrict__ dst, const T *__restrict__ aux_src,
                                                            T *__restrict__ aux_dst, int na, int64_t n_src,
                                                            int flag_arr, unsigned *__restrict__ any) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kGatherRows;
  if (r0 >= s) return;  // (the whole wave)
  // the wave's source rows, wave-uniform (past the last row: the last row
  // again, loaded and not stored)
  int64_t base[kGatherRows];
#pragma unroll
  for (int j = 0; j < kGatherRows; j++) {
    const int64_t r = r0 + j < s ? r0 + j : s - 1;
    base[j] = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)ids[r]) * units;
  }
  for (int u = lane; u < units; u += kWave) {
    uint4 v[kGatherRows];
#pragma unroll
    for (int j = 0; j < kGatherRows; j++) v[j] = src[base[j] + u];
#pragma unroll
    for (int j = 0; j < kGatherRows; j++)
      if (r0 + j < s) dst[(r0 + j) * units + u] = v[j];
  }
  // the per-row arrays: lane 4 a + j takes array a of the wave's row j
  if (lane < na * kGatherRows) {
    const int a = lane >> 2;
    const int64_t r = r0 + (lane & 3);
    if (r < s) {
      const T x = aux_src[a * n_src + ids[r]];
      aux_dst[a * s + r] = x;
      if (any && a == flag_arr && x != (T)0) *any = 1u;  // (every writer stores the same word)
    }
  }
}

__global__ __launch_bounds__(256) void remap_index_kernel(uint32_t *__restrict__ idx, int64_t count,
                                                          const uint32_t *__restrict__ map, uint32_t s) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += step) {
    const uint32_t v = idx[t];
    if (v < s) idx[t] = map[v];
  }
}

hipError_t launch_mask_count(const unsigned long long *words, int shift, int64_t n, uint32_t *counts,
                             hipStream_t s) {
  if (n <= 0) return hipSuccess;
  mask_count_kernel<<<(unsigned)((n + kMaskBlockRows - 1) / kMaskBlockRows), 256, 0, s>>>(words, shift, n, counts);
  return hipGetLastError();
}

hipError_t launch_mask_scan(const uint32_t *counts, int64_t nblk, uint32_t *bases, hipStream_t s) {
  mask_scan_kernel<<<1, 1024, 0, s>>>(counts, nblk, bases);
  return hipGetLastError();
}

hipError_t launch_mask_write(const unsigned long long *words, int shift, int64_t n, const uint32_t *bases,
                             uint32_t *out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  mask_write_kernel<<<(unsigned)((n + kMaskBlockRows - 1) / kMaskBlockRows), 256, 0, s>>>(words, shift, n, bases,
                                                                                         out);
  return hipGetLastError();
}

hipError_t launch_subset_gather(const void *src, const uint32_t *ids, int64_t s, int units, void *dst,
                                const void *aux_src, void *aux_dst, int na, int aux_bytes, int64_t n_src,
                                int flag_arr, unsigned *any, hipStream_t st) {
  if (s <= 0) return hipSuccess;
  if (units <= 0 || na < 0 || na > 4 || (aux_bytes != 4 && aux_bytes != 8)) return hipErrorInvalidValue;
  const int64_t waves = (s + kGatherRows - 1) / kGatherRows;
  const unsigned grid = (unsigned)((waves + 3) / 4);
  if (aux_bytes == 8)
    subset_gather_kernel<unsigned long long><<<grid, 256, 0, st>>>(
        (const uint4 *)src, ids, s, units, (uint4 *)dst, (const unsigned long long *)aux_src,
        (unsigned long long *)aux_dst, na, n_src, flag_arr, any);
  else
    subset_gather_kernel<uint32_t><<<grid, 256, 0, st>>>((const uint4 *)src, ids, s, units, (uint4 *)dst,
                                                         (const uint32_t *)aux_src, (uint32_t *)aux_dst, na, n_src,
                                                         flag_arr, any);
  return hipGetLastError();
}

hipError_t launch_remap_index(uint32_t *idx, int64_t count, const uint32_t *map, int64_t s, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const int64_t blocks = (count + 255) / 256;
  remap_index_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, st>>>(idx, count, map,
                                                                                          (uint32_t)s);
  return hipGetLastError();
}

}  // namespace pmm
