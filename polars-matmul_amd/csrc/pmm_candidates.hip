// pmm_candidates.hip -- candidate search (pmm_topk_f32_candidates; DESIGN.md
// §4d): exact top-k of every query row over its own list of corpus rows.
// Score: one composite key (okey32(rank value) << 32 | ~id) per candidate into
// the u64 array laid out by the caller's offsets -- the layout the range
// search's sort kernels (pmm_range.hip) consume.  Rows longer than the in-LDS
// sort are sorted piece by piece and merged by rank counting.  Decode: key ->
// (index, score) in the [m][k] planes by the top-k epilogue's rules.  No
// reference counterpart (the reference has no candidate lists).
#include "pmm_device.h"

namespace pmm {

namespace {

constexpr int kChunk = 32;    // floats of a row per K chunk: one 128-byte line
constexpr int kStride = 36;   // LDS row stride in floats (128 + 16 bytes: one
                              // access width of padding, so the 16 lanes of a
                              // ds_read_b128 group hit 16 different slots)
constexpr int kPieces = 8;    // load instructions per chunk: 8 rows x 8 lanes x 16 B each

__device__ __forceinline__ void cand_load(f32x4 (&b)[kPieces], const f32x4 *const (&src)[kPieces], int t) {
#pragma unroll
  for (int i = 0; i < kPieces; i++) b[i] = src[i][t * (kChunk / 4)];
}

// chunk t: registers -> the wave's tile -> the lane's own row -> the chain;
// the registers then take chunk t + 2
__device__ __forceinline__ float cand_step(f32x4 (&b)[kPieces], const f32x4 *const (&src)[kPieces], int t, int nch,
                                           int d, float *tw, const float *tr, const float *__restrict__ qr,
                                           float acc) {
  wave_sync();  // (the tile's last reads are done)
#pragma unroll
  for (int i = 0; i < kPieces; i++) *(f32x4 *)(tw + i * 8 * kStride) = b[i];
  wave_sync();
  if (t + 2 < nch) cand_load(b, src, t + 2);
  const float *qc = qr + t * kChunk;
  const int ne = d - t * kChunk;  // (padded columns stay out: +0.0 * +0.0 would turn a -0.0 chain positive)
  if (ne >= kChunk) {
    f32x4 x[kChunk / 4];
#pragma unroll
    for (int e = 0; e < kChunk / 4; e++) x[e] = *(const f32x4 *)(tr + 4 * e);
#pragma unroll
    for (int e = 0; e < kChunk / 4; e++) {
      acc = fmaf(qc[4 * e + 0], x[e].x, acc);
      acc = fmaf(qc[4 * e + 1], x[e].y, acc);
      acc = fmaf(qc[4 * e + 2], x[e].z, acc);
      acc = fmaf(qc[4 * e + 3], x[e].w, acc);
    }
  } else {
    for (int e = 0; e < ne; e++) acc = fmaf(qc[e], tr[e], acc);
  }
  return acc;
}

}  // namespace

// One workgroup = one unit: query row u.row against its candidates [u.start,
// u.start + 256), 64 per wave, one lane per candidate.  Per K chunk a wave
// loads its 64 rows' 128-byte pieces with eight lanes per row (every request a
// whole line), passes them through its own LDS tile and reads its lane's row
// back, then extends the lane's chain acc = fmaf(q[t], c[t], acc) by the
// chunk -- natural K order from +0.0f over exactly d elements, the f32 path's
// arithmetic.  Two chunks of loads stay in flight per lane.  The query
// elements are wave-uniform (scalar loads).  No workgroup barrier: a wave only
// reads the tile it wrote.
template <int METRIC>
__global__ __launch_bounds__(256) void cand_score_kernel(const float *__restrict__ q, const float *__restrict__ c,
                                                         const float *__restrict__ qn, const float *__restrict__ cn,
                                                         const int64_t *__restrict__ offsets,
                                                         const uint32_t *__restrict__ ids,
                                                         const CandUnit *__restrict__ units, int64_t ldq, int64_t ldc,
                                                         uint32_t n, int d, u64 *__restrict__ keys,
                                                         unsigned *__restrict__ flag) {
  __shared__ __attribute__((aligned(16))) float tile[4][64 * kStride];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = __builtin_amdgcn_readfirstlane((int)units[blockIdx.x].row);
  const int64_t o = offsets[row], cnt = offsets[row + 1] - o;
  const int64_t j0 = (int64_t)units[blockIdx.x].start + wv * 64;
  if (j0 >= cnt) return;  // (the whole wave)
  const int64_t j = j0 + lane;
  const bool live = j < cnt;
  const uint32_t id = live ? ids[o + j] : 0u;
  // the two refusals (reported by the host after the call's wait): bit 0 a
  // row that does not ascend strictly, bit 1 an id that is no corpus row
  unsigned bad = 0u;
  if (live && j > 0 && ids[o + j - 1] >= id) bad |= 1u;
  if (live && id >= n) bad |= 2u;
  // clamped before any address is formed; a lane past the row's count takes
  // the wave's first candidate again (loaded, not stored)
  uint32_t cid = id < n ? id : n - 1u;
  const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)cid);
  if (!live) cid = first;

  // lane l loads 16 bytes (l & 7) of the rows of candidates 8 i + (l >> 3)
  const f32x4 *src[kPieces];
#pragma unroll
  for (int i = 0; i < kPieces; i++) {
    const uint32_t r = (uint32_t)__shfl((int)cid, i * 8 + (lane >> 3), 64);
    src[i] = (const f32x4 *)(c + (int64_t)r * ldc) + (lane & 7);
  }
  float *tw = &tile[wv][(lane >> 3) * kStride + (lane & 7) * 4];  // + 8 i rows
  const float *tr = &tile[wv][lane * kStride];
  const float *qr = q + (int64_t)row * ldq;
  const int nch = (d + kChunk - 1) / kChunk;

  f32x4 b0[kPieces], b1[kPieces];
  float acc = 0.0f;
  cand_load(b0, src, 0);
  if (nch > 1) cand_load(b1, src, 1);
  int t = 0;
  for (; t + 1 < nch; t += 2) {
    acc = cand_step(b0, src, t, nch, d, tw, tr, qr, acc);
    acc = cand_step(b1, src, t + 1, nch, d, tw, tr, qr, acc);
  }
  if (t < nch) acc = cand_step(b0, src, t, nch, d, tw, tr, qr, acc);

  const float qv = METRIC == kMetricDot ? 0.0f : qn[row];
  const float cv = METRIC == kMetricDot ? 0.0f : cn[cid];
  const float sc = exact_score<METRIC>(acc, qv, cv);
  // A NaN score's key part is 0 and sorts last among the row's candidates; the
  // whole composite is still never 0 (an id is below n < 2^32 - 1, so ~id is
  // not 0), which keeps 0 free for the sort kernels' padding.
  if (live) keys[o + j] = ((u64)okey32(METRIC == kMetricEuclidean ? -sc : sc) << 32) | (u64)(~cid);
  if (bad) atomicOr(flag, bad);
}

// A row longer than the in-LDS sort was sorted piece by piece (pieces [first,
// first + T) of the piece offsets `po`); the first kout keys of the row's order
// go to dst.  Only the first min(kout, length) keys of a piece can be among
// them; the rank of such a key is the number of keys above it over all the
// pieces (its own place in its piece, a bisection in the others, each stopped
// at kout).  The keys of a row are distinct, so every rank below kout is
// written exactly once.  One workgroup per piece.
__global__ __launch_bounds__(256) void cand_merge_kernel(const u64 *__restrict__ keys,
                                                         const int64_t *__restrict__ po,
                                                         const CandPiece *__restrict__ pieces,
                                                         u64 *__restrict__ dst) {
  const CandPiece p = pieces[blockIdx.x];
  const int64_t b = po[p.self], len = po[p.self + 1] - b;
  const int64_t take = len < (int64_t)p.kout ? len : (int64_t)p.kout;
  for (int64_t j = threadIdx.x; j < take; j += 256) {
    const u64 key = keys[b + j];
    int64_t rank = j;
    for (uint32_t t = p.first; t < p.first + p.T && rank < (int64_t)p.kout; t++) {
      if (t == p.self) continue;
      const int64_t tb = po[t], tl = po[t + 1] - tb;
      int64_t lo = 0, hi = tl < (int64_t)p.kout ? tl : (int64_t)p.kout;  // keys [0, lo) are above, [hi, ..) are not (or past kout)
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[tb + mid] > key) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank < (int64_t)p.kout) dst[p.dst + rank] = key;
  }
}

// One thread per slot of the [m][k] planes.  Slot (row, j < len) takes key j
// of the row's sorted keys (at keys[src[row]]): the score is the key's (a zero
// euclidean distance leaves as +0.0); the keys fold -0 onto +0, so a +0.0
// cosine or dot product is recomputed by the reference's arithmetic and takes
// that zero's sign, as range_decode_kernel does.  The other slots are filled
// (index 0xFFFFFFFF, score +0.0) and slot 0 writes the row's length.
__global__ __launch_bounds__(256) void cand_decode_kernel(CandDecodeArgs a) {
  const int64_t total = (int64_t)a.m * a.k;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const int64_t row = t / a.k, j = t - row * a.k;
    const int64_t cnt = a.offsets[row + 1] - a.offsets[row];
    const int64_t len = cnt < a.k ? cnt : a.k;
    if (j == 0) a.out_len[row] = (uint32_t)len;
    if (j >= len) {
      a.out_idx[t] = 0xFFFFFFFFu;
      a.out_score[t] = 0.0f;
      continue;
    }
    const u64 key = a.keys[a.src[row] + j];
    const uint32_t col = ~(uint32_t)key;
    const float v = dekey32((uint32_t)(key >> 32));
    float sc = a.metric == kMetricEuclidean ? 0.0f - v : v;
    if (a.metric != kMetricEuclidean && __float_as_uint(sc) == 0u) {
      const float *qr = a.q + row * a.ldq, *cr = a.c + (int64_t)col * a.ldc;
      float acc = 0.0f;
      for (int i = 0; i < a.d; i++) acc = fmaf(qr[i], cr[i], acc);
      // (a dot product is its chain: no norms are read)
      const float ex = a.metric == kMetricDot ? acc : exact_score<kMetricCosine>(acc, a.qn[row], a.cn[col]);
      if (ex == 0.0f) sc = ex;
    }
    a.out_idx[t] = col;
    a.out_score[t] = sc;
  }
}

hipError_t launch_cand_score(const CandScoreArgs &a, hipStream_t s) {
  if (a.units <= 0) return hipSuccess;
  if (a.n == 0 || a.d <= 0) return hipErrorInvalidValue;
#define PMM_CAND_LAUNCH(MET)                                                                                      \
  cand_score_kernel<MET><<<(unsigned)a.units, 256, 0, s>>>(a.q, a.c, a.qn, a.cn, a.offsets, a.ids, a.unit, a.ldq, \
                                                           a.ldc, a.n, a.d, a.keys, a.flag)
  if (a.metric == kMetricCosine) PMM_CAND_LAUNCH(kMetricCosine);
  else if (a.metric == kMetricDot) PMM_CAND_LAUNCH(kMetricDot);
  else PMM_CAND_LAUNCH(kMetricEuclidean);
#undef PMM_CAND_LAUNCH
  return hipGetLastError();
}

hipError_t launch_cand_merge(const unsigned long long *keys, const int64_t *piece_offsets, const CandPiece *pieces,
                             int npieces, unsigned long long *dst, hipStream_t s) {
  if (npieces <= 0) return hipSuccess;
  cand_merge_kernel<<<(unsigned)npieces, 256, 0, s>>>(keys, piece_offsets, pieces, dst);
  return hipGetLastError();
}

hipError_t launch_cand_decode(const CandDecodeArgs &a, hipStream_t s) {
  const int64_t total = (int64_t)a.m * a.k;
  if (total <= 0) return hipSuccess;
  const int64_t blocks = (total + 255) / 256;
  cand_decode_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace pmm
