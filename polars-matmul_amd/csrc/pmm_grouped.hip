// pmm_grouped.hip -- kernels of grouped search (pmm_corpus_partition,
// pmm_topk_f32_grouped / pmm_topk_f64_grouped): the exact f32
// top-k of many small (group segment, query rows) pairs in ONE launch, the
// padding of a short per-pair list to the call's k, and the final pass that
// maps partition rows to the parent's numbering and scatters lists and lengths
// back to the caller's query order.  No reference counterpart (the reference
// has no per-row filter).  No waits between workgroups, no scratch, plain
// vector stores.
#include "pmm_grouped_kernel.h"

namespace pmm {

// A loop pair whose segment is shorter than k: its dense rows x kg lists into
// the rows' k-wide lists, the slots past kg as the contract pads them.
template <typename Score>
__global__ __launch_bounds__(256) void grouped_pad_kernel(const uint32_t *__restrict__ si,
                                                          const Score *__restrict__ ss, int rows, int kg, int k,
                                                          uint32_t *__restrict__ di, Score *__restrict__ ds) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)rows * k) return;
  const int i = (int)(t / k), j = (int)(t - (int64_t)i * k);
  di[t] = j < kg ? si[(int64_t)i * kg + j] : 0xFFFFFFFFu;
  ds[t] = j < kg ? ss[(int64_t)i * kg + j] : (Score)0;
}

// The call's last launch: grouped row i's list (partition-row numbers) leaves
// as row qrow[i] of the caller's order in the parent's numbering (map), slots
// past its length padded, with its length.
template <typename Score>
__global__ __launch_bounds__(256) void grouped_scatter_kernel(const uint32_t *__restrict__ gi,
                                                              const Score *__restrict__ gs,
                                                              const uint32_t *__restrict__ qrow,
                                                              const uint32_t *__restrict__ glen, int64_t rows, int k,
                                                              const uint32_t *__restrict__ map, uint32_t n,
                                                              uint32_t *__restrict__ out_idx,
                                                              Score *__restrict__ out_score,
                                                              uint32_t *__restrict__ out_len) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * k) return;
  const int64_t i = t / k;
  const int j = (int)(t - i * k);
  const int64_t dst = (int64_t)qrow[i] * k + j;
  const uint32_t len = glen[i];
  const uint32_t v = gi[t];
  const bool in = (uint32_t)j < len && v < n;
  out_idx[dst] = in ? map[v] : 0xFFFFFFFFu;
  out_score[dst] = in ? gs[t] : (Score)0;
  if (j == 0) out_len[qrow[i]] = len;
}

size_t grouped_lds_bytes(int dp) { return grp::lds_bytes(dp); }


hipError_t launch_grouped_topk_f32(const GroupedArgs &a, int units, int metric, hipStream_t s) {
  if (units <= 0) return hipSuccess;
  if (a.k < 1 || a.k > kGroupedMaxK || a.dp < grp::KC || a.dp > kGroupedMaxDp || a.dp % grp::KC != 0 ||
      a.ldq % 4 != 0 || a.ldc % 4 != 0 || a.ldq < a.dp || a.ldc < a.dp || (((uintptr_t)a.q | (uintptr_t)a.c) & 15))
    return hipErrorInvalidValue;
  if (a.qrow) return launch_grouped_rowtab(a, units, metric, s);  // (probed search: pmm_probed.hip)
  switch (metric) {
    case kMetricCosine: return launch_grouped_tt<kMetricCosine, false>(a, units, s);
    case kMetricDot: return launch_grouped_tt<kMetricDot, false>(a, units, s);
    case kMetricEuclidean: return launch_grouped_tt<kMetricEuclidean, false>(a, units, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_grouped_pad(const uint32_t *si, const void *ss, int rows, int kg, int k, uint32_t *di, void *ds,
                              bool f64, hipStream_t s) {
  if (rows <= 0 || k <= 0) return hipSuccess;
  const unsigned grid = (unsigned)(((int64_t)rows * k + 255) / 256);
  if (f64) grouped_pad_kernel<double><<<grid, 256, 0, s>>>(si, (const double *)ss, rows, kg, k, di, (double *)ds);
  else grouped_pad_kernel<float><<<grid, 256, 0, s>>>(si, (const float *)ss, rows, kg, k, di, (float *)ds);
  return hipGetLastError();
}

hipError_t launch_grouped_scatter(const uint32_t *gi, const void *gs, const uint32_t *qrow, const uint32_t *glen,
                                  int64_t rows, int k, const uint32_t *map, uint32_t n, uint32_t *out_idx,
                                  void *out_score, uint32_t *out_len, bool f64, hipStream_t s) {
  if (rows <= 0 || k <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((rows * k + 255) / 256);
  if (f64)
    grouped_scatter_kernel<double><<<grid, 256, 0, s>>>(gi, (const double *)gs, qrow, glen, rows, k, map, n, out_idx,
                                                        (double *)out_score, out_len);
  else
    grouped_scatter_kernel<float><<<grid, 256, 0, s>>>(gi, (const float *)gs, qrow, glen, rows, k, map, n, out_idx,
                                                       (float *)out_score, out_len);
  return hipGetLastError();
}

}  // namespace pmm
