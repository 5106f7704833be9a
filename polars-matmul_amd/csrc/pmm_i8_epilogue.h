// pmm_i8_epilogue.h -- the epilogue of a 128 x 128 int8-MFMA top-k tile, shared
// by the kernels that accumulate one in i32: gemm_i8_topk_kernel (pmm_i8.hip,
// signed bytes) and gemm_bits_topk_kernel (pmm_bits.hip, 0/1 bytes expanded
// from packed bits).  Defined once; both kernels inline it.
#pragma once
#include "pmm_device.h"

namespace pmm {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kI8Tile = 128;
constexpr int kI8Step = 64;

__device__ __forceinline__ uint32_t i8_key(int metric, int dot, uint32_t qs, uint32_t cs, float qf, float cf) {
  if (metric == kMetricDot) return (uint32_t)dot ^ 0x80000000u;
  if (metric == kMetricEuclidean) return ~(qs + cs - 2u * (uint32_t)dot);
  return okey32(__fmul_rn((float)dot, __fmul_rn(qf, cf)));
}

// acc: this wave's 4 x 4 MFMA tiles (C/D layout: column = lane & 15, row =
// 4 (lane >> 4) + reg) of the 64 x 64 outputs at rows row0 .., chunk columns
// lc0 ...  One 16-row block (ti) at a time as in gemm_f64_topk_kernel: the
// keys and pass flags first, one buffer reservation per (row, wave) -- the
// 16 lanes of a row group share it -- then the appends.
template <int METRIC>
__device__ __forceinline__ void i8_tile_epilogue(const I8TopkArgs &a, const i32x4 (&acc)[4][4], int row0, int lc0,
                                                 int lane) {
  const int i = lane & 15, kq = lane >> 4;
  const u64 grp = 0xFFFFull << (16 * kq);
  const u64 below = (1ull << lane) - 1ull;
  uint32_t csv[4];
  float cfv[4];
#pragma unroll
  for (int tj = 0; tj < 4; tj++) {
    const int lc = lc0 + 16 * tj + i;
    const bool cv = lc < a.ncol;
    csv[tj] = (METRIC == kMetricEuclidean && cv) ? a.cs[a.col0 + lc] : 0u;
    cfv[tj] = (METRIC == kMetricCosine && cv) ? a.cf[a.col0 + lc] : 0.0f;
  }
#pragma unroll
  for (int ti = 0; ti < 4; ti++) {
    uint32_t key[4][4];
    bool ps[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = row0 + 16 * ti + 4 * kq + r;
      const bool rv = row < a.M;
      const uint32_t tk = rv ? a.tkey[row] : 0xFFFFFFFFu;
      const uint32_t tx = rv ? a.tidx[row] : 0u;
      const uint32_t qsv = (METRIC == kMetricEuclidean && rv) ? a.qs[row] : 0u;
      const float qfv = (METRIC == kMetricCosine && rv) ? a.qf[row] : 0.0f;
#pragma unroll
      for (int tj = 0; tj < 4; tj++) {
        const int lc = lc0 + 16 * tj + i;
        const uint32_t gcol = (uint32_t)(a.col0 + lc);
        key[r][tj] = i8_key(METRIC, acc[ti][tj][r], qsv, csv[tj], qfv, cfv[tj]);
        ps[r][tj] = rv && lc < a.ncol && (key[r][tj] > tk || (key[r][tj] == tk && gcol < tx));
      }
    }
    unsigned base[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      unsigned n = 0u;
#pragma unroll
      for (int tj = 0; tj < 4; tj++) n += (unsigned)__popcll(__ballot(ps[r][tj]) & grp);
      unsigned b0 = 0u;
      if (i == 0 && n != 0u) b0 = atomicAdd(a.cnt + row0 + 16 * ti + 4 * kq + r, n);  // (n != 0: the row is valid)
      base[r] = b0;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = row0 + 16 * ti + 4 * kq + r;
      unsigned pos = (unsigned)__shfl((int)base[r], lane & 48, 64);
#pragma unroll
      for (int tj = 0; tj < 4; tj++) {
        const u64 m = __ballot(ps[r][tj]) & grp;
        const unsigned at = pos + (unsigned)__popcll(m & below);
        if (ps[r][tj] && at < (unsigned)a.cap) {
          Ent e;
          e.key = (u64)key[r][tj] << 32;
          e.idx = (uint32_t)(a.col0 + lc0 + 16 * tj + i);
          e.pad = (uint32_t)acc[ti][tj][r];  // the exact dot, for the finish
          a.cand[(int64_t)row * a.cap + at] = e;
        }
        pos += (unsigned)__popcll(m);
      }
    }
  }
}

}  // namespace pmm
