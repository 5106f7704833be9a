// pmm_bits.hip -- bit rows (DESIGN.md §4d "Bit rows"): sign packing of f32
// rows and the exact Hamming top-k over packed rows on the int8 MFMA.
//
// A bit row is w bytes = D = 8 w bits, bit j = (byte[j >> 3] >> (j & 7)) & 1.
// For 0/1 vectors popcount(a & b) is the dot product and the Hamming distance
// popcount(a ^ b) = Pa + Pb - 2 dot is the squared Euclidean distance, so the
// scan is the int8 scan (pmm_i8.hip) with the euclidean key ~(Pq + Pc - 2 dot)
// and S = popcount: the same tile, MFMA, epilogue (pmm_i8_epilogue.h),
// candidate buffers, thresholds and between-chunk select (i8_select_kernel's
// exact rule).  Only the staging differs -- packed bytes are read from HBM and
// 0/1 bytes written to the LDS image -- and the finish, which writes the
// integer distance itself.
#include "pmm_i8_epilogue.h"

namespace pmm {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// Sign packing: one wave per row.  A ballot of x > 0 over 64 consecutive
// elements (one coalesced 256-byte read) is 8 output bytes; NaN, -inf, both
// zeros and negatives compare false, lanes past d contribute 0.  Lane t keeps
// the ballot of the row's t-th group of 64 (per run of 64 groups) and the
// run is stored as consecutive 8-byte words, so a row's roundup(w, 8) bytes
// are written whole, the bytes past w as zeros.  pop (optional): the row's
// popcount.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_sign_kernel(const float *__restrict__ x, int64_t ldx, int64_t rows, int d,
                                                        uint8_t *__restrict__ out, int64_t ld_out,
                                                        uint32_t *__restrict__ pop) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *p = x + row * ldx;
  u64 *o = (u64 *)(out + row * ld_out);
  const int groups = (d + 63) >> 6;
  uint32_t cnt = 0u;
  for (int g0 = 0; g0 < groups; g0 += 64) {
    const int gn = min(64, groups - g0);
    u64 mine = 0ull;
    int g = 0;
    for (; g + 4 <= gn; g += 4) {  // four reads in flight
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = (g0 + g + u) * 64 + lane;
        v[u] = j < d ? p[j] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const u64 b = __ballot(v[u] > 0.0f);
        cnt += (uint32_t)__popcll(b);
        if (lane == g + u) mine = b;
      }
    }
    for (; g < gn; g++) {
      const int j = (g0 + g) * 64 + lane;
      const float v = j < d ? p[j] : 0.0f;
      const u64 b = __ballot(v > 0.0f);
      cnt += (uint32_t)__popcll(b);
      if (lane == g) mine = b;
    }
    if (lane < gn) o[g0 + lane] = mine;
  }
  if (pop && lane == 0) pop[row] = cnt;
}

hipError_t launch_pack_sign(const float *x, int64_t ldx, int64_t rows, int d, uint8_t *out, int64_t ld_out,
                            uint32_t *pop, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  pack_sign_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(x, ldx, rows, d, out, ld_out, pop);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Row popcounts of packed rows: the first dp bytes (a multiple of 16, the
// zero-padded row) of every stride of ld bytes; 16 lanes per row, 16 bytes per
// lane and step.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bits_popcount_kernel(const uint8_t *__restrict__ a, int64_t rows, int64_t ld,
                                                            int dp, uint32_t *__restrict__ pop) {
  const int sub = threadIdx.x & 15;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  uint32_t s = 0u;
  if (row < rows) {
    const u32x4 *p = (const u32x4 *)(a + row * ld);
    for (int u = sub; u < (dp >> 4); u += 16) {
      const u32x4 v = p[u];
      s += (uint32_t)(__popc(v[0]) + __popc(v[1]) + __popc(v[2]) + __popc(v[3]));
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, 64);
  if (row < rows && sub == 0) pop[row] = s;
}

hipError_t launch_bits_popcount(const uint8_t *a, int64_t rows, int64_t ld, int dp, uint32_t *pop, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  bits_popcount_kernel<<<(unsigned)((rows + 15) / 16), 256, 0, s>>>(a, rows, ld, dp, pop);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The search tile: gemm_i8_topk_kernel's (128 x 128 outputs, four waves in
// 2 x 2, each 4 x 4 v_mfma_i32_16x16x64_i8 tiles) over 0/1 bytes.  One K step
// of 64 expanded bytes is 8 packed bytes of a row, so a staging group is
// kBitsGroup K steps: thread t reads the 8 packed bytes of K step t & 1 of row
// t >> 1 of both operands -- the two threads of a row read 16 consecutive
// bytes -- and writes them as 64 bytes into that step's LDS image [row][64].
// Four bits become four bytes with one multiply and one mask: a nibble n times
// 0x00204081 puts bit b of n at bit 8 b (the four shifted copies, 7 apart and
// 4 wide, do not overlap, so nothing carries).  Byte p of a step's image row
// is bit p of that step for A and B alike, which is all the sum needs.  The
// four 16-byte pieces of a row are written in an order rotated by the row
// pair and the step, so that the eight lanes of one ds_write_b128 group cover
// 128 consecutive bytes modulo the bank width.  Double-buffered: 2 buffers x
// 2 operands x kBitsGroup steps x 8 KiB = 64 KiB.
// a.D: the padded row length in packed bytes, a multiple of 16; a.qs / a.cs:
// the rows' popcounts; the key is the euclidean one.
// ---------------------------------------------------------------------------
constexpr int kBitsGroup = 2;
constexpr int kBitsStepImage = kI8Tile * kI8Step;              // one operand, one K step
constexpr int kBitsBuf = 2 * kBitsGroup * kBitsStepImage;      // both operands, one buffer

__device__ __forceinline__ i32x4 bits_expand16(uint32_t h) {
  i32x4 r;
#pragma unroll
  for (int b = 0; b < 4; b++) r[b] = (int)((((h >> (4 * b)) & 15u) * 0x00204081u) & 0x01010101u);
  return r;
}

__global__ __launch_bounds__(256) void gemm_bits_topk_kernel(I8TopkArgs a) {
  __shared__ __attribute__((aligned(16))) int8_t lds[2 * kBitsBuf];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int nR = (a.M + kI8Tile - 1) / kI8Tile, nC = (a.ncol + kI8Tile - 1) / kI8Tile;
  // (the tile order of gemm_i8_topk_kernel)
  const int64_t T = (int64_t)nR * nC, per = (T + 7) / 8;
  const int64_t L = (int64_t)(blockIdx.x % 8) * per + blockIdx.x / 8;
  if (L >= T) return;
  const int r0 = (int)(L % nR) * kI8Tile, lc0w = (int)(L / nR) * kI8Tile;
  const int mrows = a.M - r0, ncols = a.ncol - lc0w;
  const int lr = tid >> 1, st = tid & 1;
  const int rot = 2 * ((lr >> 1) & 1) + st;
  const int8_t *ga = a.q + (int64_t)(r0 + min(lr, mrows - 1)) * a.ldq + 8 * st;
  const int8_t *gb = a.c + (int64_t)(a.col0 + lc0w + min(lr, ncols - 1)) * a.ldc + 8 * st;
  int8_t *As = lds, *Bs = lds + kBitsGroup * kBitsStepImage;  // (inside a buffer)
  i32x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ti++)
#pragma unroll
    for (int tj = 0; tj < 4; tj++) acc[ti][tj] = (i32x4){0, 0, 0, 0};
  u32x2 ra, rb;
  auto load = [&](int grp) __attribute__((always_inline)) {
    ra = *(const u32x2 *)(ga + 16 * grp);
    rb = *(const u32x2 *)(gb + 16 * grp);
  };
  auto put = [&](int buf) __attribute__((always_inline)) {
    const int at = buf * kBitsBuf + st * kBitsStepImage + lr * kI8Step;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = (j + rot) & 3;  // the 16-byte piece: bits 16 c .. 16 c + 15 of the step
      const uint32_t ha = ((c & 2) ? ra[1] : ra[0]) >> (16 * (c & 1));
      const uint32_t hb = ((c & 2) ? rb[1] : rb[0]) >> (16 * (c & 1));
      *(i32x4 *)(As + at + 16 * c) = bits_expand16(ha);
      *(i32x4 *)(Bs + at + 16 * c) = bits_expand16(hb);
    }
  };
  const int wr = (wid >> 1) * 64, wc = (wid & 1) * 64;
  load(0);
  put(0);
  __syncthreads();
  const int ngr = a.D / (8 * kBitsGroup);
  for (int g = 0; g < ngr; g++) {
    const int buf = g & 1;
    if (g + 1 < ngr) load(g + 1);
#pragma unroll
    for (int s = 0; s < kBitsGroup; s++) {
      const int8_t *pa = As + buf * kBitsBuf + s * kBitsStepImage + (wr + i) * kI8Step + 16 * kq;
      const int8_t *pb = Bs + buf * kBitsBuf + s * kBitsStepImage + (wc + i) * kI8Step + 16 * kq;
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
    }
    if (g + 1 < ngr) put(buf ^ 1);
    __syncthreads();
  }
  i8_tile_epilogue<kMetricEuclidean>(a, acc, r0 + wr, lc0w + wc, lane);
}

hipError_t launch_gemm_bits_topk(const I8TopkArgs &a, hipStream_t s) {
  if (a.M <= 0 || a.ncol <= 0) return hipSuccess;
  const int64_t T = (int64_t)((a.M + kI8Tile - 1) / kI8Tile) * ((a.ncol + kI8Tile - 1) / kI8Tile);
  gemm_bits_topk_kernel<<<(unsigned)((T + 7) / 8 * 8), 256, 0, s>>>(a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The finish, one wave per row: the row's buffer sorted under (key, lower
// index) -- the key is ~distance, exact -- and the k best written with the
// distance (double)(Pq + Pc - 2 dot) = (double)~key, best (least) first.
// rows: the output row of buffer row r is rows[r] (an overflow re-run's
// gathered rows), else r.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bits_finish_kernel(I8SelArgs a, const int *__restrict__ rows) {
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
  const int P2 = min(a.P, next_pow2_dev(n));
  for (int j = lane; j < P2; j += 64) {
    Ent e;
    e.key = 0ull;
    e.idx = 0xFFFFFFFFu;
    e.pad = 0u;
    if (j < n) e = buf[j];
    scr[j] = e;
  }
  wave_sync();
  wave_sort_desc_ent(scr, P2, lane);
  const int kk = min(a.k, n);
  const int64_t orow = rows ? rows[row] : row;
  for (int j = lane; j < a.k; j += 64) {
    const bool ok = j < kk;
    a.out_idx[orow * a.k + j] = ok ? scr[j].idx + a.index_base : 0xFFFFFFFFu;
    a.out_score[orow * a.k + j] =
        ok ? (double)(~(uint32_t)(scr[j].key >> 32)) : __longlong_as_double(0x7FF8000000000000ll);
  }
}

// LDS: P entries per wave, up to 4 waves per workgroup (launch_i8_rows' rule)
hipError_t launch_bits_finish(const I8SelArgs &a, const int *rows, hipStream_t s) {
  if (a.M <= 0) return hipSuccess;
  const size_t per_wave = (size_t)a.P * sizeof(Ent);
  int wpb = (int)(131072 / per_wave);
  wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void *)bits_finish_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr = true;
  }
  bits_finish_kernel<<<(unsigned)((a.M + wpb - 1) / wpb), wpb * 64, (size_t)wpb * per_wave, s>>>(a, rows);
  return hipGetLastError();
}

// dst row i (ldd bytes, a multiple of 16) = the first ldd bytes of src row rows[i] (stride ld >= ldd);
// pd[i] = ps[rows[i]]
__global__ __launch_bounds__(256) void bits_gather_kernel(const uint8_t *__restrict__ src, int64_t ld,
                                                          const int *__restrict__ rows, int64_t r,
                                                          uint8_t *__restrict__ dst, int64_t ldd,
                                                          const uint32_t *__restrict__ ps, uint32_t *__restrict__ pd) {
  const int64_t per = ldd >> 4, total = r * per;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / per, u = t - i * per;
    ((u32x4 *)(dst + i * ldd))[u] = ((const u32x4 *)(src + (int64_t)rows[i] * ld))[u];
    if (u == 0) pd[i] = ps[rows[i]];
  }
}
hipError_t launch_bits_gather(const uint8_t *src, int64_t ld, const int *rows, int64_t r, uint8_t *dst, int64_t ldd,
                              const uint32_t *ps, uint32_t *pd, hipStream_t s) {
  if (r <= 0) return hipSuccess;
  const int64_t blocks = (r * (ldd >> 4) + 255) / 256;
  bits_gather_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(src, ld, rows, r, dst, ldd, ps, pd);
  return hipGetLastError();
}

// dst row i (ldd doubles) = the bits of src row i as 0.0 / 1.0, columns 8 w .. ldd - 1 zero
__global__ __launch_bounds__(256) void bits_widen_kernel(const uint8_t *__restrict__ src, int64_t ld, int64_t r,
                                                         int w, double *__restrict__ dst, int64_t ldd) {
  const int64_t total = r * ldd;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / ldd;
    const int j = (int)(t - i * ldd);
    dst[t] = (j < 8 * w && ((src[i * ld + (j >> 3)] >> (j & 7)) & 1)) ? 1.0 : 0.0;
  }
}
hipError_t launch_bits_widen(const uint8_t *src, int64_t ld, int64_t r, int w, double *dst, int64_t ldd,
                             hipStream_t s) {
  if (r <= 0) return hipSuccess;
  const int64_t blocks = (r * ldd + 255) / 256;
  bits_widen_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(src, ld, r, w, dst, ldd);
  return hipGetLastError();
}

// score[t] = rint(score[t]^2): a euclidean distance of 0/1 rows back to the integer under the root
__global__ __launch_bounds__(256) void bits_square_kernel(double *__restrict__ score, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < total) score[t] = rint(__dmul_rn(score[t], score[t]));
}
hipError_t launch_bits_square(double *score, int64_t total, hipStream_t s) {
  if (total <= 0) return hipSuccess;
  bits_square_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(score, total);
  return hipGetLastError();
}

}  // namespace pmm
