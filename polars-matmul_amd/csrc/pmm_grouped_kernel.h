// pmm_grouped_kernel.h -- the grouped f32 top-k kernel as a template, so that
// its two variants compile in two objects: the grouped entry's layout in
// pmm_grouped.hip, the row-table variant of probed search in pmm_probed.hip.
// Not installed.
#pragma once
#include "pmm_device.h"

namespace pmm {

// ===========================================================================
// grouped_topk_f32_kernel: one work unit per workgroup, read from a table the
// host wrote: partition rows [c0, c0 + ng) of one group against up to 16 of
// that group's query rows (rows [q0, q0 + mq) of the label-grouped queries).
//
// Scores: v_mfma_f32_16x16x4_f32 with K in natural order -- the arrangement of
// seed_mfma_block (pmm_kernels.hip): each MFMA is bitwise a k-ordered fmaf
// chain over its 4 k and step s feeds k = 4 s + (lane >> 4), so a score is the
// chain over k = 0 .. dp-1, the fused kernel's value bit for bit; exact_score
// on the handle's corpus norms and the norm kernel's query norms finishes it.
// The 16 query rows stay in LDS; the segment streams through LDS in blocks of
// 256 columns, each in K chunks of 32 floats, double-buffered, one barrier
// per chunk, four chunks of global loads in flight per thread.  16 waves: wave
// w multiplies columns [16 w, 16 w + 16) of the block and, after the block's
// K loop, selects for query row w.
//
// Selection: composite keys okey32(score) << 32 | ~partition_row.  The
// block's 16 x 256 keys are staged in LDS (over the idle chunk buffers); wave
// w drops those not above its row's running k-th, and when the survivors and
// the row's candidate buffer (LDS, <= k <= 128 keys) exceed k keeps the best k
// of both (wave_kth_u64) and raises the running k-th.  The final <= 128 keys
// are ordered by wave_sort128_desc.  Columns past the segment's end and rows
// past mq stage empty keys (0); a list shorter than k is padded with index
// 0xFFFFFFFF and score 0.
// ===========================================================================
namespace grp {
constexpr int RM = kGroupedRows;  // query rows per unit (the MFMA's M)
constexpr int NT = 1024;          // threads: 16 waves
constexpr int NSM = 256;          // segment columns per block
constexpr int KC = 32;            // K floats per chunk
constexpr int CS = KC + 4;        // LDS row stride of a chunk (floats): conflict-free B reads
constexpr int CAP = kGroupedMaxK; // candidate keys per row
constexpr int PFC = 4;            // chunks of global loads in flight
constexpr int NPC = NSM * 8 / NT; // 16-byte pieces per thread per chunk
static_assert(NT / 64 == RM, "one wave per query row");
static_assert(NT / 64 * 16 == NSM, "one 16-column accumulator chain per wave");
static_assert((size_t)RM * NSM * 8 <= (size_t)2 * NSM * CS * 4, "the staged keys alias the chunk buffers");
__host__ __device__ constexpr size_t lds_bytes(int dp) {
  return (size_t)RM * (dp + 4) * 4 + (size_t)2 * NSM * CS * 4 + RM * 4 + NSM * 4 + (size_t)RM * CAP * 8;
}
static_assert(lds_bytes(kGroupedMaxDp) <= 160 * 1024, "LDS budget");
}  // namespace grp

// ROWTAB (probed search, pmm_topk_f32_probed): a unit's rows are slots of the
// call's label-sorted (query row, label) slots; slot s reads query row
// a.qrow[s] of the ungathered queries and its norm, and writes list s.  A query
// row that probes P groups is read by P units and copied by none.
template <int METRIC, bool ROWTAB = false>
__global__ __launch_bounds__(grp::NT) void grouped_topk_f32_kernel(GroupedArgs a) {
  using namespace grp;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool XFORM = METRIC != kMetricDot;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const GroupedUnit u = a.units[blockIdx.x];
  const int dp = a.dp, k = a.k;
  const int mq = (int)u.mq, ng = (int)u.ng;
  const int QS = dp + 4;              // query row stride in LDS: conflict-free A reads
  float *qs = (float *)smem;          // [RM][QS]
  float *cbuf = qs + RM * QS;         // [2][NSM][CS]
  float *qn_s = cbuf + 2 * NSM * CS;  // [RM]
  float *cn_s = qn_s + RM;            // [NSM]
  u64 *cand = (u64 *)(cn_s + NSM);    // [RM][CAP]
  u64 *keys = (u64 *)cbuf;            // [RM][NSM], between a block's K loop and the next block's first chunk
  const int G = dp / KC;
  // the unit's query rows (rows past mq as zeros) and their norms
  for (int i = tid; i < RM * (dp / 4); i += NT) {
    const int r = i / (dp / 4), j4 = i - r * (dp / 4);
    f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < mq) {
      int64_t row = (int64_t)(u.q0 + r);
      if constexpr (ROWTAB) row = (int64_t)a.qrow[u.q0 + r];
      x = *(const f32x4 *)(a.q + row * a.ldq + 4 * j4);
    }
    *(f32x4 *)(qs + r * QS + 4 * j4) = x;
  }
  if (tid < RM) {
    float v = 0.0f;
    if (XFORM && tid < mq) {
      if constexpr (ROWTAB) v = a.qn[a.qrow[u.q0 + tid]];
      else v = a.qn[u.q0 + tid];
    }
    qn_s[tid] = v;
  }
  const int g4 = lane >> 4, l16 = lane & 15;
  const int col = 16 * w + l16;  // this lane's column of a block
  // row w's candidate count and running k-th (wave-uniform; 0 = accept all)
  int cnt = 0;
  u64 thr = 0ull;
  for (int cb0 = 0; cb0 < ng; cb0 += NSM) {
    const int nv = min(NSM, ng - cb0);  // the block's columns inside the segment
    const float *cblk = a.c + (int64_t)(u.c0 + cb0) * a.ldc;
    // piece p = tid + NT u -> column p >> 3, 16-byte part p & 7 (8 consecutive
    // threads read one 128-byte run); a column past the segment's end reads
    // the segment's last row again (loaded, multiplied and never kept)
    f32x4 v[PFC][NPC];
    auto load_chunk = [&](int t, f32x4 (&r)[NPC]) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < NPC; p++) {
        const int pc = tid + NT * p, c = min(pc >> 3, nv - 1), part = pc & 7;
        r[p] = *(const f32x4 *)(cblk + (int64_t)c * a.ldc + t * KC + 4 * part);
      }
    };
    auto store_chunk = [&](int buf, const f32x4 (&r)[NPC]) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < NPC; p++) {
        const int pc = tid + NT * p, c = pc >> 3, part = pc & 7;
        *(f32x4 *)(cbuf + buf * NSM * CS + c * CS + 4 * part) = r[p];
      }
    };
#pragma unroll
    for (int j = 0; j < PFC; j++) load_chunk(min(j, G - 1), v[j]);  // (clamped: every load unconditional)
    if (XFORM && tid < NSM) cn_s[tid] = tid < nv ? a.cn[(int64_t)u.c0 + cb0 + tid] : 0.0f;
    store_chunk(0, v[0]);
    __syncthreads();
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t0 = 0; t0 < G; t0 += PFC) {
#pragma unroll
      for (int j = 0; j < PFC; j++) {
        const int t = t0 + j;
        if (t < G) {
          const float *cb = cbuf + (t & 1) * NSM * CS + col * CS + g4;
          const float *qa = qs + l16 * QS + t * KC + g4;
#pragma unroll
          for (int s4 = 0; s4 < KC / 4; s4++)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[4 * s4], cb[4 * s4], acc, 0, 0, 0);
        }
        // chunk t + 1 into the other buffer (its last readers, chunk t - 1,
        // passed the previous barrier); chunk t + PFC into chunk t's registers
        store_chunk((t + 1) & 1, v[(j + 1) % PFC]);
        load_chunk(min(t + PFC, G - 1), v[j]);
        __syncthreads();
      }
    }
    // (every wave is past the last chunk's MFMAs and every chunk store has
    // landed: the chunk buffers now take the block's keys)
    // D of the 16x16x4: the lane holds rows 4 (lane >> 4) + i of its column
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = 4 * g4 + i;
      const bool ok = r < mq && col < nv;
      const float sc = exact_score<METRIC>(acc[i], XFORM ? qn_s[r] : 0.0f, XFORM ? cn_s[col] : 0.0f);
      const uint32_t prow = u.c0 + (uint32_t)(cb0 + col);
      keys[r * NSM + col] =
          ok ? (((u64)okey32(METRIC == kMetricEuclidean ? -sc : sc) << 32) | (u64)(~prow)) : 0ull;
    }
    __syncthreads();
    if (w < mq) {
      u64 z[6];
      int ns = 0;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const u64 x = keys[w * NSM + lane + 64 * e];
        z[e] = x > thr ? x : 0ull;
        ns += __popcll(__ballot(z[e] != 0ull));
      }
      u64 *cw = cand + w * CAP;
      if (cnt + ns <= k) {
        // room for all of them: appended behind the row's candidates
        const int base = cnt;
        const u64 z4[4] = {z[0], z[1], z[2], z[3]};
        cnt += wave_keep_ge<4>(z4, 0ull, [&](int pos, u64 x) __attribute__((always_inline)) { cw[base + pos] = x; },
                               lane);
      } else {
        // the best k of the survivors and the candidates; the k-th is the
        // row's new bound (later keys must beat it)
#pragma unroll
        for (int e = 0; e < 2; e++) z[4 + e] = (lane + 64 * e < cnt) ? cw[lane + 64 * e] : 0ull;
        wave_sync();  // every lane has read before any rewrites
        const u64 t = wave_kth_u64<6>(z, k);
        cnt = wave_keep_ge<6>(z, t, [&](int pos, u64 x) __attribute__((always_inline)) { cw[pos] = x; }, lane);
        thr = t;
      }
      wave_sync();
    }
    __syncthreads();  // the keys are consumed before the next block's first chunk lands on them
  }
  if (w >= mq) return;
  // row w's list: its <= k candidates, best first, padded to k
  const u64 *cw = cand + w * CAP;
  u64 y0 = lane < cnt ? cw[lane] : 0ull;
  u64 y1 = lane + 64 < cnt ? cw[lane + 64] : 0ull;
  wave_sort128_desc(y0, y1, lane);  // (empty slots, 0, sort last)
  uint32_t *oi = a.out_idx + (int64_t)(u.q0 + w) * k;
  float *os = a.out_score + (int64_t)(u.q0 + w) * k;
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int pos = lane + 64 * e;
    const u64 y = e ? y1 : y0;
    if (pos < k) {
      uint32_t id = 0xFFFFFFFFu;
      float sc = 0.0f;
      if (y != 0ull) {
        id = ~(uint32_t)y;
        const float val = dekey32((uint32_t)(y >> 32));
        sc = METRIC == kMetricEuclidean ? 0.0f - val : val;  // +0.0 for a zero distance
      }
      oi[pos] = id;
      os[pos] = sc;
    }
  }
}

template <int METRIC, bool ROWTAB>
static inline hipError_t launch_grouped_tt(const GroupedArgs &a, int units, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void *)grouped_topk_f32_kernel<METRIC, ROWTAB>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr = true;
  }
  grouped_topk_f32_kernel<METRIC, ROWTAB><<<(unsigned)units, grp::NT, grp::lds_bytes(a.dp), s>>>(a);
  return hipGetLastError();
}
}  // namespace pmm
