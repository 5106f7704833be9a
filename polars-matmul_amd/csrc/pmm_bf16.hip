// pmm_bf16.hip -- bf16 compute path of the fused top-k (PMM_COMPUTE_BF16;
// BASELINE configs[3]: 100k x 1M x 768 bf16 cosine k=100, CDNA4 bf16 MFMA with
// f32 accumulation).
//
// Scores are those of the bf16-rounded embeddings: Q and C are rounded to
// bf16 (round to nearest even), S = Q.C^T runs on v_mfma_f32_32x32x16_bf16
// (f32 accumulation), the norms are the f32 norms of the bf16 rows in the
// reference's order, and the metric epilogue and per-row top-k are the f32
// path's (exact_score / prefilter_bound / candidate buffers / merge), so the
// result is the exact top-k of the bf16 vectors up to f32 accumulation order.
//
// Why a different kernel shape than the f32 path: a bf16 MFMA does 8x the
// work of the f32 one per operand byte, so the f32 kernel's 256 x 256 tile with
// both operands re-streamed through LDS would need ~20 TB/s from L2 + MALL.
// Here each wave keeps its 32 query rows x D in registers for a whole work
// unit (D <= 768: 4 registers per 16 columns of D), so only corpus tiles
// stream: 128 query rows x 128 corpus columns per workgroup, 4 waves (one per
// SIMD), corpus K-steps of 128 bf16 (32 KiB per step) through a 3-slot LDS-DMA
// ring with counted vmcnt waits (the next-but-one step is always in flight).
#include "pmm_bf16_kernel.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pmm {

size_t gemm_bf16_lds_bytes(int capg, int nst) {
  return (size_t)OFF_RING + (size_t)nst * STAGE + (size_t)NW * capg * 8;
}

// ---------------------------------------------------------------------------
// f32 -> bf16 with zero padding: one thread per 8 output elements.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float *__restrict__ src,
                                                          int64_t rows, int64_t d, int64_t lds,
                                                          uint16_t *__restrict__ dst, int64_t ldd) {
  const int64_t per_row = ldd >> 3;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * per_row) return;
  const int64_t r = t / per_row;
  const int64_t c0 = (t - r * per_row) * 8;
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int64_t c = c0 + j;
    // plain cast: v_cvt_pk_bf16_f32, round to nearest even, NaN stays NaN
    v[j] = (c < d) ? (__bf16)src[r * lds + c] : (__bf16)0.0f;
  }
  *(bf16x8 *)(dst + r * ldd + c0) = v;
}

hipError_t launch_f32_to_bf16(const float *src, int64_t rows, int64_t d, int64_t lds, uint16_t *dst,
                              int64_t ldd, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int64_t threads = rows * (ldd >> 3);
  f32_to_bf16_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(src, rows, d, lds, dst, ldd);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// f32 -> bf16 with zero padding AND the rows' norms of both metrics, one pass:
// what f32_to_bf16_kernel + norms_kernel<float, __bf16> (squared = 0 and 1)
// give in three launches and 10 bytes of HBM traffic per element, in one and 6.
//
// A workgroup takes a band of kRnRows rows, kRnCols columns at a time.  Every
// thread rounds groups of 8 columns (two 16-byte loads where the source
// allows, one 16-byte store) and parks the rounded group in LDS; then 8 lanes
// per row walk the chunk out of LDS in norms_rows' order -- lane j owns the
// partial sum of columns j, j + 8, ... -- carrying the partial over the
// chunks, so any d works.  The combine, the tail columns d8..d-1 and the
// factors are norms_rows' statements (no FMA: -ffp-contract=off).
// ---------------------------------------------------------------------------
constexpr int kRnRows = 32;    // rows per workgroup: 256 threads / 8 lanes per row
constexpr int kRnCols = 256;   // columns per chunk
constexpr int kRnLd = kRnCols + 8;  // LDS row stride (bf16): 8 rows of a wave land 4 banks apart

__global__ __launch_bounds__(256) void round_norms_bf16_kernel(const float *__restrict__ src, int64_t rows,
                                                               int64_t d, int64_t lds, uint16_t *__restrict__ dst,
                                                               int64_t ldd, float *__restrict__ norm,
                                                               float *__restrict__ inv_norm, float *__restrict__ sq,
                                                               float *__restrict__ sq_factor, int vec) {
  __shared__ __attribute__((aligned(16))) __bf16 park[kRnRows * kRnLd];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kRnRows;
  const int nrows = (int)((rows - row0) < kRnRows ? (rows - row0) : kRnRows);
  const int64_t d8 = d & ~(int64_t)7;
  const int my = tid >> 3, j = tid & 7;  // norm phase: lane j of band row my
  float acc = 0.0f;
  float tail[7];
#pragma unroll
  for (int t = 0; t < 7; t++) tail[t] = 0.0f;
  for (int64_t cb = 0; cb < ldd; cb += kRnCols) {
    const int cw = (int)((ldd - cb) < kRnCols ? (ldd - cb) : kRnCols);  // a multiple of 8
    const int gpr = cw >> 3;                                             // 8-column groups per row
    for (int g = tid; g < nrows * gpr; g += 256) {
      const int r = g / gpr;
      const int cl = (g - r * gpr) * 8;
      const int64_t c0 = cb + cl;
      const float *p = src + (row0 + r) * lds + c0;
      float x[8];
      if (vec && c0 + 8 <= d) {
        const float4 lo = *(const float4 *)p, hi = *(const float4 *)(p + 4);
        x[0] = lo.x, x[1] = lo.y, x[2] = lo.z, x[3] = lo.w;
        x[4] = hi.x, x[5] = hi.y, x[6] = hi.z, x[7] = hi.w;
      } else {
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = (c0 + u < d) ? p[u] : 0.0f;
      }
      bf16x8 v;
      // plain cast, as f32_to_bf16_kernel: round to nearest even, NaN stays NaN
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = (__bf16)x[u];
      *(bf16x8 *)(dst + (row0 + r) * ldd + c0) = v;
      *(bf16x8 *)(park + r * kRnLd + cl) = v;
    }
    __syncthreads();
    if (my < nrows && cb < d) {
      const __bf16 *pr = park + my * kRnLd;
      const int lim = (int)((d8 - cb) < cw ? (d8 - cb) : cw);  // columns of this chunk below d8
      int i = j;
      for (; i + 56 < lim; i += 64) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = (float)pr[i + 8 * u];
#pragma unroll
        for (int u = 0; u < 8; u++) acc = acc + x[u] * x[u];
      }
      for (; i < lim; i += 8) {
        const float x = (float)pr[i];
        acc = acc + x * x;
      }
      // the tail columns d8..d-1 lie in one chunk: lane 0 keeps them for the end
      if (j == 0 && d8 < d && d8 >= cb && d8 < cb + cw) {
#pragma unroll
        for (int t = 0; t < 7; t++)
          if (d8 + t < d) tail[t] = (float)pr[(int)(d8 - cb) + t];
      }
    }
    __syncthreads();
  }
  const int base = (tid & 63) & ~7;
  float pp[8];
#pragma unroll
  for (int t = 0; t < 8; t++) pp[t] = __shfl(acc, base + t, 64);
  if (my < nrows && j == 0) {
    float sum = 0.0f;
    sum = sum + (pp[0] + pp[4]);
    sum = sum + (pp[1] + pp[5]);
    sum = sum + (pp[2] + pp[6]);
    sum = sum + (pp[3] + pp[7]);
#pragma unroll
    for (int t = 0; t < 7; t++)
      if (d8 + t < d) sum = sum + tail[t] * tail[t];
    const int64_t row = row0 + my;
    const float v = sqrt_rn<float>(sum);
    if (norm) norm[row] = v;
    if (inv_norm) inv_norm[row] = (v > 1e-6f) ? 1.0f / v : 0.0f;
    if (sq) sq[row] = sum;
    if (sq_factor) sq_factor[row] = sum * (float)(1.0 - 0x1p-18);
  }
}

hipError_t launch_round_norms_bf16(const float *src, int64_t rows, int64_t d, int64_t lds, uint16_t *dst,
                                   int64_t ldd, float *norm, float *inv_norm, float *sq, float *sq_factor,
                                   hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (ldd < d || ldd % 8 != 0 || lds < d || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
  const int vec = (((uintptr_t)src & 15) == 0 && lds % 4 == 0) ? 1 : 0;
  const int64_t grid = (rows + kRnRows - 1) / kRnRows;
  round_norms_bf16_kernel<<<(unsigned)grid, 256, 0, s>>>(src, rows, d, lds, dst, ldd, norm, inv_norm, sq, sq_factor,
                                                         vec);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Rows prepared for the f32 cosine screen in one read of the
// f32 rows: the bf16 image, the EXACT cosine norm and pre-filter factor of the
// unrounded row (norms_kernel<float, float>'s bits), the rounding residual
// bound and the unsafe flag -- what norms_kernel and a rounding pass over the
// rows gave in two launches and 10 bytes of HBM traffic per element, in one
// and 6.  Handles and the device entry both prepare their operands with it.
//
// round_norms_bf16_kernel's shape: a band of kRnRows rows, kRnCols columns at
// a time.  Every thread rounds groups of 8 columns (16-byte loads where the
// source allows, one 16-byte store) and parks the UNROUNDED group in LDS; then
// 8 lanes per row walk the chunk in norms_rows' order -- lane j owns columns
// j, j + 8, ... -- carrying the sum of squares over the chunks (norms_rows'
// statements, no FMA) and, beside it, the sum of squared residuals and the
// element-window test (any order: the 2^-9 inflation covers their rounding).
// ---------------------------------------------------------------------------
constexpr int kSpLd = kRnCols + 8;  // LDS row stride (f32): the 8 rows of a wave land 8 banks apart

// round to nearest even, NaN stays NaN
__device__ __forceinline__ uint32_t screen_bf16_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  return (x != x) ? ((u >> 16) | 0x40u) : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
// one element's share of the residual sum and of the window test
__device__ __forceinline__ void screen_element(float x, float &r2, bool &ok) {
  const float r = x - __uint_as_float(screen_bf16_bits(x) << 16);  // (exact for a safe element)
  r2 = fmaf(r, r, r2);
  const float ax = fabsf(x);
  ok = ok && (ax == 0.0f || (ax >= kScreenMinAbs && ax <= kScreenMaxAbs));
}

__global__ __launch_bounds__(256) void screen_prepare_kernel(const float *__restrict__ src, int64_t rows, int64_t d,
                                                             int64_t lds, uint16_t *__restrict__ dst, int64_t ldd,
                                                             float *__restrict__ norm, float *__restrict__ inv_norm,
                                                             float *__restrict__ rel, unsigned *__restrict__ bad,
                                                             unsigned *scal, int vec) {
  __shared__ __attribute__((aligned(16))) float park[kRnRows * kSpLd];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kRnRows;
  const int nrows = (int)((rows - row0) < kRnRows ? (rows - row0) : kRnRows);
  const int64_t d8 = d & ~(int64_t)7;
  const int my = tid >> 3, j = tid & 7;  // norm phase: lane j of band row my
  float acc = 0.0f, r2 = 0.0f;
  bool ok = true;
  float tail[7];
#pragma unroll
  for (int t = 0; t < 7; t++) tail[t] = 0.0f;
  for (int64_t cb = 0; cb < ldd; cb += kRnCols) {
    const int cw = (int)((ldd - cb) < kRnCols ? (ldd - cb) : kRnCols);  // a multiple of 8
    const int gpr = cw >> 3;                                             // 8-column groups per row
    for (int g = tid; g < nrows * gpr; g += 256) {
      const int r = g / gpr;
      const int cl = (g - r * gpr) * 8;
      const int64_t c0 = cb + cl;
      const float *p = src + (row0 + r) * lds + c0;
      f32x4 lo = {0.0f, 0.0f, 0.0f, 0.0f}, hi = {0.0f, 0.0f, 0.0f, 0.0f};
      if (vec && c0 + 8 <= d) {
        lo = *(const f32x4 *)p;
        hi = *(const f32x4 *)(p + 4);
      } else {
#pragma unroll
        for (int u = 0; u < 4; u++) {
          lo[u] = (c0 + u < d) ? p[u] : 0.0f;
          hi[u] = (c0 + 4 + u < d) ? p[4 + u] : 0.0f;
        }
      }
      uint32_t b[8];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        b[u] = screen_bf16_bits(lo[u]);
        b[4 + u] = screen_bf16_bits(hi[u]);
      }
      *(uint4 *)(dst + (row0 + r) * ldd + c0) =
          make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
      *(f32x4 *)(park + r * kSpLd + cl) = lo;
      *(f32x4 *)(park + r * kSpLd + cl + 4) = hi;
    }
    __syncthreads();
    if (my < nrows && cb < d) {
      const float *pr = park + my * kSpLd;
      const int lim = (int)((d8 - cb) < cw ? (d8 - cb) : cw);  // columns of this chunk below d8
      int i = j;
      for (; i + 56 < lim; i += 64) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = pr[i + 8 * u];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          acc = acc + x[u] * x[u];
          screen_element(x[u], r2, ok);
        }
      }
      for (; i < lim; i += 8) {
        const float x = pr[i];
        acc = acc + x * x;
        screen_element(x, r2, ok);
      }
      // the tail columns d8..d-1 lie in one chunk: lane 0 keeps them for the end
      if (j == 0 && d8 < d && d8 >= cb && d8 < cb + cw) {
#pragma unroll
        for (int t = 0; t < 7; t++)
          if (d8 + t < d) {
            tail[t] = pr[(int)(d8 - cb) + t];
            screen_element(tail[t], r2, ok);
          }
      }
    }
    __syncthreads();
  }
  const int base = (tid & 63) & ~7;
  float pp[8];
#pragma unroll
  for (int t = 0; t < 8; t++) pp[t] = __shfl(acc, base + t, 64);
  int okw = ok ? 1 : 0;
#pragma unroll
  for (int off = 4; off; off >>= 1) {
    r2 += __shfl_xor(r2, off, 64);
    okw &= __shfl_xor(okw, off, 64);
  }
  if (my < nrows && j == 0) {
    float sum = 0.0f;
    sum = sum + (pp[0] + pp[4]);
    sum = sum + (pp[1] + pp[5]);
    sum = sum + (pp[2] + pp[6]);
    sum = sum + (pp[3] + pp[7]);
#pragma unroll
    for (int t = 0; t < 7; t++)
      if (d8 + t < d) sum = sum + tail[t] * tail[t];
    const int64_t row = row0 + my;
    const float v = sqrt_rn<float>(sum);
    if (norm) norm[row] = v;
    if (inv_norm) inv_norm[row] = (v > 1e-6f) ? 1.0f / v : 0.0f;
    const bool unsafe = !okw || !(v > 1e-6f) || !(sum > 0.0f);
    // (the sums' and the square root's rounding: far inside the 2^-9 inflation;
    // a safe row's true ratio is below 2^-8, bf16's half ulp)
    const float rl = unsafe ? 0x1p-8f : fminf(__builtin_sqrtf(r2 / sum) * (1.0f + 0x1p-9f), 0x1p-8f);
    if (rel) rel[row] = rl;
    if (bad) bad[row] = unsafe ? 1u : 0u;
    if (scal) {
      if (unsafe) {
        atomicOr(scal + 1, 1u);
      } else if (__float_as_uint(rl) > __hip_atomic_load(scal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        atomicMax(scal, __float_as_uint(rl));  // (non-negative floats order as their bits)
      }
    }
  }
}

hipError_t launch_screen_prepare(const float *src, int64_t rows, int64_t d, int64_t lds, uint16_t *dst, int64_t ldd,
                                 float *norm, float *inv_norm, float *rel, unsigned *bad, unsigned *scal,
                                 hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (ldd < d || ldd % 8 != 0 || lds < d || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
  const int vec = (((uintptr_t)src & 15) == 0 && lds % 4 == 0) ? 1 : 0;
  const int64_t grid = (rows + kRnRows - 1) / kRnRows;
  screen_prepare_kernel<<<(unsigned)grid, 256, 0, s>>>(src, rows, d, lds, dst, ldd, norm, inv_norm, rel, bad, scal,
                                                       vec);
  return hipGetLastError();
}

// bf16 -> f32 (exact widening) with zero padding to ldd: one thread per element
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const uint16_t *__restrict__ src, int64_t rows,
                                                          int64_t d, int64_t lds, float *__restrict__ dst,
                                                          int64_t ldd) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * ldd) return;
  const int64_t r = t / ldd, c = t - r * ldd;
  dst[t] = (c < d) ? __uint_as_float((uint32_t)src[r * lds + c] << 16) : 0.0f;
}

hipError_t launch_bf16_to_f32(const uint16_t *src, int64_t rows, int64_t d, int64_t lds, float *dst, int64_t ldd,
                              hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int64_t threads = rows * ldd;
  bf16_to_f32_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(src, rows, d, lds, dst, ldd);
  return hipGetLastError();
}

hipError_t launch_norms_bf16(const uint16_t *a, int64_t rows, int64_t d, int64_t ld, int squared,
                             float *out, float *inv, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int64_t threads = rows * 8;
  norms_kernel<float, __bf16><<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(
      (const __bf16 *)a, rows, d, ld, squared, out, inv);
  return hipGetLastError();
}

// per-KS instantiations (pmm_bf16_ks.hip)
hipError_t launch_bf16_ks1(const GemmF32Args &a, int grid, size_t lds, hipStream_t s);
hipError_t launch_bf16_ks2(const GemmF32Args &a, int grid, size_t lds, hipStream_t s);
hipError_t launch_bf16_ks3(const GemmF32Args &a, int grid, size_t lds, hipStream_t s);
hipError_t launch_bf16_ks4(const GemmF32Args &a, int grid, size_t lds, hipStream_t s);
hipError_t launch_bf16_ks5(const GemmF32Args &a, int grid, size_t lds, hipStream_t s);
hipError_t launch_bf16_ks6(const GemmF32Args &a, int grid, size_t lds, hipStream_t s);

hipError_t launch_gemm_bf16(const GemmF32Args &a, int grid, hipStream_t s) {
  const size_t lds = gemm_bf16_lds_bytes(a.capg, a.nst);
  if (lds > 160 * 1024 || a.D % kBf16DAlign != 0) return hipErrorInvalidValue;
  switch (a.D / 128) {
    case 1: return launch_bf16_ks1(a, grid, lds, s);
    case 2: return launch_bf16_ks2(a, grid, lds, s);
    case 3: return launch_bf16_ks3(a, grid, lds, s);
    case 4: return launch_bf16_ks4(a, grid, lds, s);
    case 5: return launch_bf16_ks5(a, grid, lds, s);
    case 6: return launch_bf16_ks6(a, grid, lds, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pmm
