// pmm_probed.hip -- kernels of probed search (pmm_topk_f32_probed; DESIGN.md
// §4d "Probed search"): the row-table variant of the grouped top-k kernel
// (pmm_grouped_kernel.h), which writes one exact per-group list for every
// (query row, probed group) slot without a copy of the query row per probe,
// and the merge that keeps the best k of a row's lists under the order of a
// search of the union's parent rows.  No reference counterpart.  No atomics, no
// waits between workgroups, no scratch, plain vector loads and stores.
#include "pmm_grouped_kernel.h"

namespace pmm {

// ===========================================================================
// probe_merge_f32_kernel: one wave per query row, four rows per workgroup.
//
// Keys: okey32(score, or -distance) << 32 | ~map[partition row].  The index
// part is the PARENT row: partition order follows the groups, so between two
// groups a lower partition row may be the higher parent row, and equal scores
// go to the lower parent row.  A parent row lies in one group and a row's
// labels are distinct, so a row's keys are distinct.  A NaN score keys as 0 in
// its upper half (after every number, the lower parent row first), which is
// where the per-group lists and every other entry put it.
//
// Selection (the grouped kernel's scheme): the row's lists are read as one
// array of lists x k entries, 256 per round, four per lane; padding entries
// (index 0xFFFFFFFF) and keys not above the running k-th are dropped.  The
// row's <= k <= 128 candidates live in registers, two per lane, between the
// rounds.  While survivors and candidates together are at most k they are all
// kept; otherwise the best k of both are (wave_kth_u64) and their least is the
// new bound.  Either way wave_keep_ge packs them through a 1 KiB LDS staging
// row of the wave (a lane cannot address another lane's register), from which
// they return to the two registers.  wave_sort128_desc orders the final keys.
//
// Zeros: okey32 folds -0 onto +0 and dekey32 returns +0.0, but the per-slot
// lists carry the reference's sign (launch_zero_sign_f32 ran on them).  A
// cosine or dot entry that leaves as a zero looks its parent row up in the
// row's lists and takes that entry's score (zero_sign_lists_kernel's idea;
// zeros are rare).  A euclidean zero is +0.0 everywhere.
// ===========================================================================
namespace prb {
constexpr int WAVES = 4;
constexpr int CAP = kGroupedMaxK;
}  // namespace prb

template <bool EUCLID>
__global__ __launch_bounds__(64 * prb::WAVES) void probe_merge_f32_kernel(ProbeMergeArgs a) {
  using namespace prb;
  __shared__ u64 stage[WAVES][CAP];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = (int)blockIdx.x * WAVES + w;
  if (row >= a.m) return;  // (wave-uniform: the selection below runs with the whole wave)
  const int k = a.k;
  const uint32_t s0 = a.row_off[row];
  const uint32_t total = (a.row_off[row + 1] - s0) * (uint32_t)k;  // lists * k entries (the call's: <= 2^31)
  const uint32_t *slots = a.row_slots + s0;
  u64 *st = stage[w];
  // entry e of the row: list e / k, position e % k -> its place in in_idx / in_score (-1: past the end)
  auto place = [&](uint32_t e) __attribute__((always_inline)) -> int64_t {
    if (e >= total) return -1;
    const uint32_t l = e / (uint32_t)k;
    return (int64_t)slots[l] * k + (e - l * (uint32_t)k);
  };
  u64 c0 = 0ull, c1 = 0ull;  // the candidates: key i in lane i & 63, c0 for i < 64
  int cnt = 0;
  u64 thr = 0ull;
  for (uint32_t e0 = 0; e0 < total; e0 += 256) {
    u64 z[6];
    int ns = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t p = place(e0 + lane + 64 * j);
      u64 x = 0ull;
      if (p >= 0) {
        const uint32_t id = a.in_idx[p];
        if (id < a.n) {
          const float sc = a.in_score[p];
          x = ((u64)okey32(EUCLID ? -sc : sc) << 32) | (u64)(~a.map[id]);
        }
      }
      z[j] = x > thr ? x : 0ull;
      ns += __popcll(__ballot(z[j] != 0ull));
    }
    if (ns == 0) continue;
    z[4] = c0;
    z[5] = c1;
    u64 t = 0ull;
    if (cnt + ns > k) t = thr = wave_kth_u64<6>(z, k);
    // (a row's keys are distinct, so at most k pass; the guard keeps a broken table inside the staging row)
    cnt = wave_keep_ge<6>(z, t, [&](int pos, u64 x) __attribute__((always_inline)) { if (pos < CAP) st[pos] = x; },
                          lane);
    cnt = min(cnt, k);
    wave_sync();
    c0 = lane < cnt ? st[lane] : 0ull;
    c1 = lane + 64 < cnt ? st[lane + 64] : 0ull;
    wave_sync();  // every lane has read before the next round rewrites the staging row
  }
  wave_sort128_desc(c0, c1, lane);  // (empty slots, 0, sort last)
  uint32_t *oi = a.out_idx + (int64_t)row * k;
  float *os = a.out_score + (int64_t)row * k;
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int pos = lane + 64 * e;
    const u64 y = e ? c1 : c0;
    if (pos >= k) continue;
    uint32_t id = 0xFFFFFFFFu;
    float sc = 0.0f;
    if (y != 0ull) {
      id = ~(uint32_t)y;
      const float val = dekey32((uint32_t)(y >> 32));
      sc = EUCLID ? 0.0f - val : val;  // +0.0 for a zero distance
      if (!EUCLID && val == 0.0f) {
        // the zero's sign, from the entry's own list
        for (uint32_t f = 0; f < total; f++) {
          const int64_t p = place(f);
          const uint32_t pi = a.in_idx[p];
          if (pi < a.n && a.map[pi] == id) {
            sc = a.in_score[p];
            break;
          }
        }
      }
    }
    oi[pos] = id;
    os[pos] = sc;
  }
  if (lane == 0) a.out_len[row] = (uint32_t)cnt;
}

// (checked by launch_grouped_topk_f32, its only caller)
hipError_t launch_grouped_rowtab(const GroupedArgs &a, int units, int metric, hipStream_t s) {
  switch (metric) {
    case kMetricCosine: return launch_grouped_tt<kMetricCosine, true>(a, units, s);
    case kMetricDot: return launch_grouped_tt<kMetricDot, true>(a, units, s);
    case kMetricEuclidean: return launch_grouped_tt<kMetricEuclidean, true>(a, units, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_probe_merge_f32(const ProbeMergeArgs &a, int metric, hipStream_t s) {
  if (a.m <= 0) return hipSuccess;
  if (a.k < 1 || a.k > kGroupedMaxK) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)((a.m + prb::WAVES - 1) / prb::WAVES);
  if (metric == kMetricEuclidean) probe_merge_f32_kernel<true><<<grid, 64 * prb::WAVES, 0, s>>>(a);
  else probe_merge_f32_kernel<false><<<grid, 64 * prb::WAVES, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace pmm
