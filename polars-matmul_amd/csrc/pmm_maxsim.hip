// pmm_maxsim.hip -- late-interaction search (pmm_topk_f32_maxsim; DESIGN.md
// §4d "Multi-vector rows"): MaxSim(Q, D) = sum over the query's tokens of the
// max over the document's tokens of the engine's f32 pair score, for every
// (query row, listed document) pair.  Score: one composite key (okey32(score)
// << 32 | ~document) per pair into the u64 array laid out by the lists' own
// offsets -- the layout the range search's sort kernels and the candidate
// search's merge consume unchanged.  Decode: key -> (document, score) in the
// [m][k] planes.  No reference counterpart (the reference has one vector per
// row).
#include "pmm_device.h"

namespace pmm {

namespace {

constexpr int kChunk = 32;   // floats of a token row per K chunk: one 128-byte line
constexpr int kStride = 36;  // LDS row stride of a wave's document tile in floats (as cand_score_kernel's)
constexpr int kTile = 64 * kStride;  // a wave's tile: 64 document tokens x one K chunk
constexpr int kQPad = 4;     // the query block's row stride is dp + 4 floats (= 16 bytes mod 128, as kStride)

// LDS floats at padded dimension dp: the query block (32 x (dp + 4)), its 32
// token norms, the unit's running sums, four waves' document tiles
constexpr int lds_floats(int dp) { return 32 * (dp + kQPad) + 32 + kMaxsimRun + 4 * kTile; }
static_assert(lds_floats(kMaxsimMaxDp) * 4 <= 160 * 1024, "LDS budget");
static_assert(lds_floats(kMaxsimMaxDp + 32) * 4 > 160 * 1024, "kMaxsimMaxDp is the LDS budget's limit");

template <int NP>
__device__ __forceinline__ void ms_load(f32x4 (&b)[NP], const f32x4 *const (&src)[8], int t) {
#pragma unroll
  for (int i = 0; i < NP; i++) b[i] = src[i][t * (kChunk / 4)];
}

// registers {0, 2, 1, 3} of the fragment = the k pairs (8 qd, +1) (+2, +3)
// (+4, +5) (+6, +7), lane half h holding the pair's element h (gemm_f32_kernel)
__device__ __forceinline__ void ms_kpair(f32x4 &x) {
  auto r0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[0]), __float_as_uint(x[1]), false, false);
  auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[2]), __float_as_uint(x[3]), false, false);
  x[0] = __uint_as_float(r0[0]);
  x[1] = __uint_as_float(r0[1]);
  x[2] = __uint_as_float(r1[0]);
  x[3] = __uint_as_float(r1[1]);
}

// K chunk t: registers -> the wave's tile -> fragments -> 16 MFMA substeps per
// accumulator block in natural K order; the registers then take chunk t + 2
template <bool TWO>
__device__ __forceinline__ void ms_step(f32x4 (&b)[TWO ? 8 : 4], const f32x4 *const (&src)[8], int t, int nch,
                                        float *tw, const float *tr, const float *qrow, int h, f32x16 &acc0,
                                        f32x16 &acc1) {
  constexpr int NP = TWO ? 8 : 4;
  wave_sync();  // (the tile's last reads are done)
#pragma unroll
  for (int i = 0; i < NP; i++) *(f32x4 *)(tw + i * 8 * kStride) = b[i];
  wave_sync();
  if (t + 2 < nch) ms_load<NP>(b, src, t + 2);
#pragma unroll
  for (int qd = 0; qd < 4; qd++) {
    const int co = 8 * qd + 4 * h;
    f32x4 av = *(const f32x4 *)(qrow + t * kChunk + co);
    f32x4 b0 = *(const f32x4 *)(tr + co);
    f32x4 b1 = TWO ? *(const f32x4 *)(tr + 32 * kStride + co) : b0;
    ms_kpair(av);
    ms_kpair(b0);
    if (TWO) ms_kpair(b1);
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
      const int js = ((jj & 1) << 1) | (jj >> 1);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[js], b0[js], acc0, 0, 0, 0);
      if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[js], b1[js], acc1, 0, 0, 0);
    }
  }
}

// the chains of 32 query tokens x 32 (64 with TWO) document tokens over all of dp
template <bool TWO>
__device__ __forceinline__ void ms_block(const f32x4 *const (&src)[8], int nch, float *tw, const float *tr,
                                         const float *qrow, int h, f32x16 &acc0, f32x16 &acc1) {
  constexpr int NP = TWO ? 8 : 4;
  f32x4 b0[NP], b1[NP];
  ms_load<NP>(b0, src, 0);
  if (nch > 1) ms_load<NP>(b1, src, 1);
  int t = 0;
  for (; t + 1 < nch; t += 2) {
    ms_step<TWO>(b0, src, t, nch, tw, tr, qrow, h, acc0, acc1);
    ms_step<TWO>(b1, src, t + 1, nch, tw, tr, qrow, h, acc0, acc1);
  }
  if (t < nch) ms_step<TWO>(b0, src, t, nch, tw, tr, qrow, h, acc0, acc1);
}

template <int S>
__device__ __forceinline__ float ms_max_xor(float v, int lane) {
  return fmaxf(v, __uint_as_float(lane_xor_u32<S>(__float_as_uint(v), lane)));
}

}  // namespace

// One workgroup = one unit: query row u.row against the documents at places
// [u.start, u.start + kMaxsimRun) of its list, which the four waves take in
// turn.  The row's tokens go 32 at a time: a block is staged once into LDS
// (zero-padded to 32 rows and dp columns) and every document of the unit is
// scored against it before the next block, the pair's sum so far waiting in
// LDS -- so a pair's maxima are added in token order whatever the query's
// length.  Per document a wave walks its tokens 64 at a time (two 32 x 32
// accumulator blocks in flight; one when 32 or fewer are left): their rows'
// 128-byte pieces are loaded with eight lanes per row (every request a whole
// line), pass through the wave's own LDS tile and feed v_mfma_f32_32x32x2_f32
// with K in natural order, so an accumulator is the chain acc = fmaf(q[u],
// d[u], acc) from +0.0f (the padded columns add +0.0 products: they can turn a
// -0.0 chain into +0.0, which no maximum's sum can tell).  Epilogue per block:
// exact_score per element, the columns past the document's end at -inf, an
// element-wise running fmaxf (a NaN pair score is dropped); at the document's
// end one cross-lane max over the 32 columns of each lane half and the 32 row
// maxima added in token order, rows past the query's end left out.  Rows and
// columns of padding clamp their address to the document's last token.
template <int METRIC>
__global__ __launch_bounds__(256) void maxsim_score_kernel(MaxsimScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ms_smem[];
  const int dp = a.dp, qst = dp + kQPad;
  float *qs = ms_smem;             // [32][qst]
  float *qn_l = qs + 32 * qst;     // [32]
  float *sums = qn_l + 32;         // [kMaxsimRun]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float *tile = sums + kMaxsimRun + wv * kTile;
  const int r32 = lane & 31, h = lane >> 5;
  const int row = __builtin_amdgcn_readfirstlane((int)a.unit[blockIdx.x].row);
  const int64_t o = a.offsets[row], cnt = a.offsets[row + 1] - o;
  const int64_t p0 = (int64_t)a.unit[blockIdx.x].start;
  const int run = (int)(cnt - p0 < (int64_t)kMaxsimRun ? cnt - p0 : (int64_t)kMaxsimRun);
  const int64_t q0 = a.q_offsets[row];
  const int Lq = (int)(a.q_offsets[row + 1] - q0);
  const int nqb = Lq > 0 ? (Lq + 31) / 32 : 1;  // (a row without tokens: every sum is +0.0; its list is cut to nothing)
  const int nch = dp / kChunk;
  const float ninf = -__builtin_inff();

  float *tw = tile + (lane >> 3) * kStride + (lane & 7) * 4;  // + 8 i rows
  const float *tr = tile + r32 * kStride;
  const float *qrow = qs + r32 * qst;

  for (int qb = 0; qb < nqb; qb++) {
    const int nq = Lq - qb * 32 < 32 ? Lq - qb * 32 : 32;  // the block's tokens (<= 0: none)
    __syncthreads();  // (the previous block's reads are done)
    for (int i = threadIdx.x; i < 32 * (dp / 4); i += 256) {
      const int r = i / (dp / 4), c4 = i - r * (dp / 4);
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (r < nq) v = *(const f32x4 *)(a.q + (q0 + qb * 32 + r) * a.ldq + 4 * c4);
      *(f32x4 *)(qs + r * qst + 4 * c4) = v;
    }
    if (threadIdx.x < 32)
      qn_l[threadIdx.x] = (METRIC == kMetricCosine && (int)threadIdx.x < nq) ? a.qn[q0 + qb * 32 + threadIdx.x] : 0.0f;
    __syncthreads();
    float qv[16];
#pragma unroll
    for (int e = 0; e < 16; e++) qv[e] = qn_l[acc_row(e, h)];

    for (int ci = wv; ci < run; ci += 4) {
      const int64_t p = p0 + ci;
      const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ids[o + p]);
      // the two refusals (reported by the host after the call's wait): bit 0 a
      // list that does not ascend strictly, bit 1 an id that is no document
      unsigned bad = 0u;
      if (qb == 0) {
        if (p > 0 && a.ids[o + p - 1] >= id) bad |= 1u;
        if (id >= a.n_docs) bad |= 2u;
      }
      const uint32_t cid = id < a.n_docs ? id : a.n_docs - 1u;  // clamped before any address is formed
      const int64_t t0 = a.doc_offsets[cid];
      const int Ld = (int)(a.doc_offsets[cid + 1] - t0);  // >= 1 (the creator refuses an empty document)
      const float *drows = a.c + t0 * a.ldc;

      float mx[16];
#pragma unroll
      for (int e = 0; e < 16; e++) mx[e] = ninf;
      for (int tk0 = 0; tk0 < Ld; tk0 += 64) {
        // lane l loads 16 bytes (l & 7) of the rows of tokens tk0 + 8 i + (l >> 3)
        const f32x4 *src[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
          int tkn = tk0 + 8 * i + (lane >> 3);
          tkn = tkn < Ld ? tkn : Ld - 1;
          src[i] = (const f32x4 *)(drows + (int64_t)tkn * a.ldc) + (lane & 7);
        }
        const bool two = tk0 + 32 < Ld;
        f32x16 acc0 = {}, acc1 = {};
        if (two) ms_block<true>(src, nch, tw, tr, qrow, h, acc0, acc1);
        else ms_block<false>(src, nch, tw, tr, qrow, h, acc0, acc1);
        {
          const int j = tk0 + r32;
          const float cv = METRIC == kMetricCosine ? a.cn[t0 + (j < Ld ? j : Ld - 1)] : 0.0f;
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const float v = exact_score<METRIC>(acc0[e], qv[e], cv);
            mx[e] = fmaxf(mx[e], j < Ld ? v : ninf);
          }
        }
        if (two) {
          const int j = tk0 + 32 + r32;
          const float cv = METRIC == kMetricCosine ? a.cn[t0 + (j < Ld ? j : Ld - 1)] : 0.0f;
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const float v = exact_score<METRIC>(acc1[e], qv[e], cv);
            mx[e] = fmaxf(mx[e], j < Ld ? v : ninf);
          }
        }
      }
      // the row maxima: over the 32 columns of each lane half, then lane 0's
      // (rows acc_row(e, 0)) and lane 32's (rows acc_row(e, 1)) to every lane
      float m0[16], m1[16];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        float v = mx[e];
        v = ms_max_xor<1>(v, lane);
        v = ms_max_xor<2>(v, lane);
        v = ms_max_xor<4>(v, lane);
        v = ms_max_xor<8>(v, lane);
        v = ms_max_xor<16>(v, lane);
        m0[e] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), 0));
        m1[e] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), 32));
      }
      // one sequential sum in token order, from the blocks before
      float s = qb == 0 ? 0.0f : sums[ci];
#pragma unroll
      for (int g = 0; g < 4; g++) {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (8 * g + i < nq) s = s + m0[4 * g + i];
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (8 * g + 4 + i < nq) s = s + m1[4 * g + i];
      }
      if (lane == 0) {
        if (qb + 1 < nqb) sums[ci] = s;
        // A NaN score's key part is 0 and sorts last; the composite is still
        // never 0 (~cid is not 0), which keeps 0 free for the sort kernels' padding.
        else a.keys[o + p] = ((u64)okey32(s) << 32) | (u64)(~cid);
        if (bad) atomicOr(a.flag, bad);
      }
    }
  }
}

// One thread per slot of the [m][k] planes.  Slot (row, j < len) takes key j
// of the row's sorted keys (at keys[src[row]]); the score is the key's (a
// MaxSim score is never -0.0, so no zero's sign is recomputed).  The other
// slots are filled (index 0xFFFFFFFF, score +0.0) and slot 0 writes the row's
// length: min(k, listed documents), 0 for a row without tokens.
__global__ __launch_bounds__(256) void maxsim_decode_kernel(MaxsimDecodeArgs a) {
  const int64_t total = (int64_t)a.m * a.k;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const int64_t row = t / a.k, j = t - row * a.k;
    const int64_t cnt = a.offsets[row + 1] - a.offsets[row];
    const int64_t len = a.q_offsets[row + 1] == a.q_offsets[row] ? 0 : (cnt < a.k ? cnt : a.k);
    if (j == 0) a.out_len[row] = (uint32_t)len;
    if (j >= len) {
      a.out_idx[t] = 0xFFFFFFFFu;
      a.out_score[t] = 0.0f;
      continue;
    }
    const u64 key = a.keys[a.src[row] + j];
    a.out_idx[t] = ~(uint32_t)key;
    a.out_score[t] = dekey32((uint32_t)(key >> 32));
  }
}

size_t maxsim_lds_bytes(int dp) { return (size_t)lds_floats(dp) * 4; }

template <int METRIC>
static hipError_t launch_maxsim_score_t(const MaxsimScoreArgs &a, hipStream_t s) {
  static bool attr_set = false;  // opt in to > 64 KiB dynamic LDS
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void *)maxsim_score_kernel<METRIC>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  maxsim_score_kernel<METRIC><<<(unsigned)a.units, 256, maxsim_lds_bytes(a.dp), s>>>(a);
  return hipGetLastError();
}

hipError_t launch_maxsim_score(const MaxsimScoreArgs &a, hipStream_t s) {
  if (a.units <= 0) return hipSuccess;
  if (a.n_docs == 0 || a.dp <= 0 || a.dp % kChunk != 0 || a.dp > kMaxsimMaxDp || a.ldc < a.dp || a.ldq < a.dp ||
      (a.metric != kMetricCosine && a.metric != kMetricDot))
    return hipErrorInvalidValue;
  return a.metric == kMetricCosine ? launch_maxsim_score_t<kMetricCosine>(a, s)
                                   : launch_maxsim_score_t<kMetricDot>(a, s);
}

hipError_t launch_maxsim_decode(const MaxsimDecodeArgs &a, hipStream_t s) {
  const int64_t total = (int64_t)a.m * a.k;
  if (total <= 0) return hipSuccess;
  const int64_t blocks = (total + 255) / 256;
  maxsim_decode_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace pmm
