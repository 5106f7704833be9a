// pmm_i8.hip -- top-k over signed 8-bit rows on the int8 MFMA
// (v_mfma_i32_16x16x64_i8), bit-equal to the f64 branch on the same values
// widened to f64 (src/matmul.rs:449-468: what an Int8 column takes in the
// reference, and took here before this file).
//
// An int8 dot product is exact in i32 in any order (|x y| <= 2^14, d < 2^16),
// and so are the rows' sums of squares in u32; the f64 scores the reference
// computes from them are then two or three correctly rounded f64 operations on
// exact integers, which i8_finish_kernel repeats (exact_score_f64).  What the
// scan needs is only an ORDER close enough to the f64 one to keep every
// possible member of the top k:
//   dot        key = the i32 dot, exact;
//   euclidean  key = ~(Sq + Sc - 2 dot), the exact squared distance in u32 --
//              distinct integers below 2^32 have distinct f64 square roots, so
//              (key, lower index) IS the f64 order;
//   cosine     key = okey32(a), a = f32(dot) * (fq * fc), fq = f32(1/sqrt(Sq));
//              |a - score| < kI8CosEps (DESIGN.md §4d "Int8 rows"), so a row
//              keeps every entry with a >= a_k - 2 eps (a_k: its k-th best
//              approximate score) and the finish ranks the kept band by the
//              f64 scores.
// The scan is the f64 path's (pmm_f64.hip): the corpus in growing column
// chunks, one GEMM launch per chunk whose epilogue appends each element at or
// above its row's threshold to the row's candidate buffer (with its dot), a
// per-row compaction between chunks.  A row whose buffer overflowed is flagged
// and re-run on the widened rows by the caller.
#include "pmm_i8_epilogue.h"

namespace pmm {

// ---------------------------------------------------------------------------
// Row sums of squares and the cosine factors: one wave per row over the padded
// row (the padding is zero), 16 bytes per lane and step.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void i8_norms_kernel(const int8_t *__restrict__ a, int64_t rows, int64_t ld,
                                                       int dp, uint32_t *__restrict__ sq, float *__restrict__ fac) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const i32x4 *p = (const i32x4 *)(a + row * ld);
  uint32_t s = 0u;
  for (int u = lane; u < dp / 16; u += 64) {
    const i32x4 v = p[u];
#pragma unroll
    for (int w = 0; w < 4; w++) {
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int x = (int)(int8_t)((uint32_t)v[w] >> (8 * b));
        s += (uint32_t)(x * x);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, 64);
  if (lane == 0) {
    sq[row] = s;
    fac[row] = s ? (float)__ddiv_rn(1.0, __dsqrt_rn((double)s)) : 0.0f;
  }
}

hipError_t launch_i8_norms(const int8_t *a, int64_t rows, int64_t ld, int dp, uint32_t *sq, float *fac,
                           hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  i8_norms_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(a, rows, ld, dp, sq, fac);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The GEMM tile: 128 query rows x 128 corpus columns per workgroup, four waves
// in 2 x 2, each 4 x 4 v_mfma_i32_16x16x64_i8 tiles (64 x 64 outputs, 64
// accumulator registers).  K runs in steps of 64 bytes through a double-
// buffered LDS image [row][64 bytes] of both operands (32 KiB); lane (i =
// lane & 15, g = lane >> 4) takes bytes 16 g .. 16 g + 15 of row i of a
// fragment for A and for B alike -- the sum is over all 64 bytes whichever k
// the hardware assigns to a byte position, and integer sums have no order.
// C/D layout: column = lane & 15, row = 4 (lane >> 4) + reg.
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void gemm_i8_topk_kernel(I8TopkArgs a) {
  __shared__ __attribute__((aligned(16))) int8_t lds[2 * 2 * kI8Tile * kI8Step];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int nR = (a.M + kI8Tile - 1) / kI8Tile, nC = (a.ncol + kI8Tile - 1) / kI8Tile;
  // consecutive workgroups go to the 8 XCDs in turn: each XCD walks a
  // contiguous stretch of the tile order, row block fastest (f64_tile_of)
  const int64_t T = (int64_t)nR * nC, per = (T + 7) / 8;
  const int64_t L = (int64_t)(blockIdx.x % 8) * per + blockIdx.x / 8;
  if (L >= T) return;
  const int r0 = (int)(L % nR) * kI8Tile, lc0w = (int)(L / nR) * kI8Tile;
  const int mrows = a.M - r0, ncols = a.ncol - lc0w;
  // staging: thread t takes bytes 16 (t & 3) .. +15 of rows t / 4 and t / 4 + 64
  const int lr = tid >> 2, seg = (tid & 3) * 16;
  const int8_t *ga[2], *gb[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    ga[j] = a.q + (int64_t)(r0 + min(lr + 64 * j, mrows - 1)) * a.ldq + seg;
    gb[j] = a.c + (int64_t)(a.col0 + lc0w + min(lr + 64 * j, ncols - 1)) * a.ldc + seg;
  }
  int8_t *As = lds, *Bs = lds + 2 * kI8Tile * kI8Step;
  i32x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ti++)
#pragma unroll
    for (int tj = 0; tj < 4; tj++) acc[ti][tj] = (i32x4){0, 0, 0, 0};
  i32x4 ra[2], rb[2];
  auto load = [&](int ko) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      ra[j] = *(const i32x4 *)(ga[j] + ko);
      rb[j] = *(const i32x4 *)(gb[j] + ko);
    }
  };
  auto put = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      *(i32x4 *)(As + buf * kI8Tile * kI8Step + (lr + 64 * j) * kI8Step + seg) = ra[j];
      *(i32x4 *)(Bs + buf * kI8Tile * kI8Step + (lr + 64 * j) * kI8Step + seg) = rb[j];
    }
  };
  const int wr = (wid >> 1) * 64, wc = (wid & 1) * 64;
  load(0);
  put(0);
  __syncthreads();
  const int nch = a.D / kI8Step;
  for (int ch = 0; ch < nch; ch++) {
    const int buf = ch & 1;
    if (ch + 1 < nch) load((ch + 1) * kI8Step);
    const int8_t *pa = As + buf * kI8Tile * kI8Step + (wr + i) * kI8Step + 16 * kq;
    const int8_t *pb = Bs + buf * kI8Tile * kI8Step + (wc + i) * kI8Step + 16 * kq;
    i32x4 av[4], bv[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      av[t] = *(const i32x4 *)(pa + 16 * t * kI8Step);
      bv[t] = *(const i32x4 *)(pb + 16 * t * kI8Step);
    }
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
#pragma unroll
      for (int tj = 0; tj < 4; tj++)
        acc[ti][tj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
    if (ch + 1 < nch) put(buf ^ 1);
    __syncthreads();
  }

  i8_tile_epilogue<METRIC>(a, acc, r0 + wr, lc0w + wc, lane);  // (pmm_i8_epilogue.h)
}

hipError_t launch_gemm_i8_topk(const I8TopkArgs &a, hipStream_t s) {
  if (a.M <= 0 || a.ncol <= 0) return hipSuccess;
  const int64_t T = (int64_t)((a.M + kI8Tile - 1) / kI8Tile) * ((a.ncol + kI8Tile - 1) / kI8Tile);
  const dim3 grid((unsigned)((T + 7) / 8 * 8)), blk(256);
  if (a.metric == kMetricCosine) gemm_i8_topk_kernel<kMetricCosine><<<grid, blk, 0, s>>>(a);
  else if (a.metric == kMetricEuclidean) gemm_i8_topk_kernel<kMetricEuclidean><<<grid, blk, 0, s>>>(a);
  else gemm_i8_topk_kernel<kMetricDot><<<grid, blk, 0, s>>>(a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Between chunks, one wave per row: the row's buffer sorted in LDS under (key,
// lower index), its best k kept and the threshold raised to the k-th -- dot and
// euclidean: the k-th entry itself (key and index; the keys are exact);
// cosine: every entry whose key is at or above okey32(a_k - 2 eps) stays (the
// band), and later elements are appended from that key up, any index.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void i8_select_kernel(I8SelArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int row = blockIdx.x * (blockDim.x >> 6) + wid;
  if (row >= a.M) return;
  Ent *scr = (Ent *)smem + (size_t)wid * a.P;
  int n = (int)a.cnt[row];
  if (n > a.cap) {
    if (lane == 0) a.ovf[row] = 1u;
    n = a.cap;
  }
  if (n < a.k) return;  // still accepting everything
  Ent *buf = a.cand + (int64_t)row * a.cap;
  const int P2 = min(a.P, next_pow2_dev(n));
  for (int j = lane; j < P2; j += 64) {
    Ent e;
    if (j < n) {
      e = buf[j];
    } else {
      e.key = 0ull;
      e.idx = 0xFFFFFFFFu;
      e.pad = 0u;
    }
    scr[j] = e;
  }
  wave_sync();
  wave_sort_desc_ent(scr, P2, lane);
  uint32_t tk = (uint32_t)(scr[a.k - 1].key >> 32), tx = scr[a.k - 1].idx;
  int keep = a.k;
  if (a.metric == kMetricCosine) {
    tk = okey32(__fsub_rn(dekey32(tk), 2.0f * kI8CosEps));
    tx = 0xFFFFFFFFu;
    keep = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      keep += __popcll(__ballot(j < n && (uint32_t)(scr[j].key >> 32) >= tk));
    }
  }
  for (int j = lane; j < keep; j += 64) buf[j] = scr[j];
  if (lane == 0) {
    a.cnt[row] = (unsigned)keep;
    a.tkey[row] = tk;
    a.tidx[row] = tx;
  }
}

// ---------------------------------------------------------------------------
// The finish, one wave per row: every kept candidate's f64 score from its
// exact dot and the rows' integer sums of squares by the oracle's operations
// (exact_score_f64: cosine dot / (sqrt(Sq) sqrt(Sc)) past the 1e-10 rule,
// euclidean sqrt(max(Sq + Sc - 2 dot, 0)), dot itself -- every input an exact
// integer in f64), then the k best under (f64 score, lower index), best first.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double i8_score(int metric, int dot, uint32_t qs, uint32_t cs) {
  if (metric == kMetricCosine)
    return exact_score_f64<kMetricCosine>((double)dot, __dsqrt_rn((double)qs), __dsqrt_rn((double)cs));
  if (metric == kMetricEuclidean) return exact_score_f64<kMetricEuclidean>((double)dot, (double)qs, (double)cs);
  return (double)dot;
}

__global__ __launch_bounds__(256) void i8_finish_kernel(I8SelArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int row = blockIdx.x * (blockDim.x >> 6) + wid;
  if (row >= a.M) return;
  Ent *scr = (Ent *)smem + (size_t)wid * a.P;
  int n = (int)a.cnt[row];
  if (n > a.cap) {
    if (lane == 0) a.ovf[row] = 1u;
    n = a.cap;
  }
  const Ent *buf = a.cand + (int64_t)row * a.cap;
  const uint32_t qs = a.metric == kMetricDot ? 0u : a.qs[row];
  const int P2 = min(a.P, next_pow2_dev(n));
  for (int j = lane; j < P2; j += 64) {
    Ent e;
    e.key = 0ull;
    e.idx = 0xFFFFFFFFu;
    e.pad = 0u;
    if (j < n) {
      const Ent c = buf[j];
      const uint32_t cs = a.metric == kMetricDot ? 0u : a.cs[c.idx];
      const double sc = i8_score(a.metric, (int)c.pad, qs, cs);
      e.key = okey64(a.metric == kMetricEuclidean ? -sc : sc);
      e.idx = c.idx;
    }
    scr[j] = e;
  }
  wave_sync();
  wave_sort_desc_ent(scr, P2, lane);
  const int kk = min(a.k, n);
  for (int j = lane; j < a.k; j += 64) {
    const bool ok = j < kk;
    const double v = ok ? dekey64(scr[j].key) : __longlong_as_double(0x7FF8000000000000ll);
    a.out_idx[(int64_t)row * a.k + j] = ok ? scr[j].idx + a.index_base : 0xFFFFFFFFu;
    a.out_score[(int64_t)row * a.k + j] = (ok && a.metric == kMetricEuclidean) ? 0.0 - v : v;
  }
}

// LDS: P entries per wave, up to 4 waves per workgroup
static hipError_t launch_i8_rows(const I8SelArgs &a, bool finish, hipStream_t s) {
  if (a.M <= 0) return hipSuccess;
  const size_t per_wave = (size_t)a.P * sizeof(Ent);
  int wpb = (int)(131072 / per_wave);
  wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
  const size_t lds = (size_t)wpb * per_wave;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void *)i8_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void *)i8_finish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr = true;
  }
  const unsigned grid = (unsigned)((a.M + wpb - 1) / wpb);
  if (finish) i8_finish_kernel<<<grid, wpb * 64, lds, s>>>(a);
  else i8_select_kernel<<<grid, wpb * 64, lds, s>>>(a);
  return hipGetLastError();
}
hipError_t launch_i8_select(const I8SelArgs &a, hipStream_t s) { return launch_i8_rows(a, false, s); }
hipError_t launch_i8_finish(const I8SelArgs &a, hipStream_t s) { return launch_i8_rows(a, true, s); }

// thresholds to accept-all, counts and overflow flags to zero
__global__ __launch_bounds__(256) void i8_reset_kernel(uint32_t *tkey, uint32_t *tidx, unsigned *cnt, unsigned *ovf,
                                                       int m) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < m) {
    tkey[r] = 0u;
    tidx[r] = 0xFFFFFFFFu;
    cnt[r] = 0u;
    ovf[r] = 0u;
  }
}
hipError_t launch_i8_reset(uint32_t *tkey, uint32_t *tidx, unsigned *cnt, unsigned *ovf, int m, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  i8_reset_kernel<<<(m + 255) / 256, 256, 0, s>>>(tkey, tidx, cnt, ovf, m);
  return hipGetLastError();
}

// rows[*count ..] += the rows base + r with ovf[r] set (any order)
__global__ __launch_bounds__(256) void i8_collect_kernel(const unsigned *ovf, int m, int base, unsigned *count,
                                                         int *rows) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < m && ovf[r]) rows[atomicAdd(count, 1u)] = base + r;
}
hipError_t launch_i8_collect(const unsigned *ovf, int m, int base, unsigned *count, int *rows, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  i8_collect_kernel<<<(m + 255) / 256, 256, 0, s>>>(ovf, m, base, count, rows);
  return hipGetLastError();
}

// dst row i (ldd doubles, columns d .. ldd - 1 zero) = src row (rows ? rows[i] : i) widened; exact
__global__ __launch_bounds__(256) void i8_widen_kernel(const int8_t *__restrict__ src, int64_t lds_,
                                                       const int *__restrict__ rows, int64_t r, int d,
                                                       double *__restrict__ dst, int64_t ldd) {
  const int64_t total = r * ldd;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / ldd;
    const int j = (int)(t - i * ldd);
    const int64_t sr = rows ? rows[i] : i;
    dst[t] = j < d ? (double)src[sr * lds_ + j] : 0.0;
  }
}
hipError_t launch_i8_widen(const int8_t *src, int64_t ld, const int *rows, int64_t r, int d, double *dst,
                           int64_t ldd, hipStream_t s) {
  if (r <= 0) return hipSuccess;
  const int64_t blocks = (r * ldd + 255) / 256;
  i8_widen_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(src, ld, rows, r, d, dst, ldd);
  return hipGetLastError();
}

// out_idx / out_score row rows[i] = the dense lists' row i (k entries each)
__global__ __launch_bounds__(256) void i8_scatter_kernel(const uint32_t *__restrict__ oi,
                                                         const double *__restrict__ os,
                                                         const int *__restrict__ rows, int64_t r, int k,
                                                         uint32_t *__restrict__ out_idx,
                                                         double *__restrict__ out_score) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= r * k) return;
  const int64_t i = t / k, j = t - i * k;
  out_idx[(int64_t)rows[i] * k + j] = oi[t];
  out_score[(int64_t)rows[i] * k + j] = os[t];
}
hipError_t launch_i8_scatter(const uint32_t *oi, const double *os, const int *rows, int64_t r, int k,
                             uint32_t *out_idx, double *out_score, hipStream_t s) {
  if (r <= 0 || k <= 0) return hipSuccess;
  i8_scatter_kernel<<<(unsigned)((r * k + 255) / 256), 256, 0, s>>>(oi, os, rows, r, k, out_idx, out_score);
  return hipGetLastError();
}

}  // namespace pmm
