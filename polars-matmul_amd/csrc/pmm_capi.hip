// pmm_capi.hip -- C ABI (include/pmm.h) and host orchestration.
//
// Host side of the hot path that the reference implements in
// src/matmul.rs:295-519 (dispatch, extraction, k clipping, error texts) and
// src/lib.rs:15-55 (the FFI boundary).  Here it owns: per-thread HIP stream
// and scratch arena, upload/padding of host inputs, the work decomposition of
// the fused kernel, and the launch sequence norms -> fused GEMM+top-k ->
// merge.  All device work of one call is enqueued on one stream; host calls
// synchronise that stream once at the end.
#include "pmm_internal.h"
#include "../../include/pmm.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

using namespace pmm;

namespace {

constexpr const char *kVersion = "0.1.4+mi355x.r1";
constexpr size_t kMaterialiseBudget = size_t(2) << 30;  // bytes of score chunk (f64/large-k/matmul)

// The budget of one call's score or result chunk: kMaterialiseBudget, which
// PMM_MATERIALISE_BUDGET (bytes, per call; a test knob) lowers so that a small
// call runs its row-chunk loop past the first chunk.  A value outside
// [1, kMaterialiseBudget] or with anything but decimal digits is ignored: the
// knob can only shrink a chunk.  (Sizing and running read it separately: a
// caller of pmm_topk_workspace_bytes sets it identically for both.)
size_t materialise_budget() {
  const char *e = getenv("PMM_MATERIALISE_BUDGET");
  if (!e || !*e) return kMaterialiseBudget;
  unsigned long long v = 0;
  for (const char *p = e; *p; p++) {
    if (*p < '0' || *p > '9' || v > kMaterialiseBudget) return kMaterialiseBudget;
    v = v * 10 + (unsigned)(*p - '0');
  }
  return (v >= 1 && v <= kMaterialiseBudget) ? (size_t)v : kMaterialiseBudget;
}

thread_local std::string t_err;

int fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  t_err = buf;
  return code;
}

// pmm_topk_f32_device / pmm_topk_bf16_device: a row stride of `ld` elements of `elem` bytes
// against kMaxRowStrideBytes (pmm_internal.h), before anything is enqueued.
int check_row_stride(const char *name, int64_t ld, int elem) {
  if (ld <= kMaxRowStrideBytes / elem) return PMM_OK;
  return fail(PMM_ERR_ARG,
              "%s=%lld is a row stride above %lld bytes (%lld elements), the largest this entry takes: its "
              "kernels address up to %d rows through one 2^31-byte buffer descriptor",
              name, (long long)ld, (long long)kMaxRowStrideBytes, (long long)(kMaxRowStrideBytes / elem),
              kDescRowsMax);
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(PMM_ERR_HIP, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_),      \
                  __FILE__, __LINE__, #expr);                                           \
  } while (0)

struct DeviceInfo {
  bool probed = false;
  bool ok = false;
  int cus = 256;
  std::string arch;
};
constexpr int kMaxDevices = 64;
std::mutex g_dev_mu;
DeviceInfo g_dev[kMaxDevices];  // fixed storage: readers index it without the lock

// Corpus sharding over several devices for the host entry points
// (pmm_set_devices): process-wide, empty = one device.
std::mutex g_devs_mu;
std::vector<int> g_devs;
std::vector<int> devices_snapshot() {
  std::lock_guard<std::mutex> lk(g_devs_mu);
  return g_devs;
}
// The device host entry points run on when a device list is set: its first
// entry (the root, which also merges a sharded search), else -1 (the thread's
// pmm_set_device choice or the current device).  A one-entry list therefore
// moves all host work to that device; work that is not sharded (f32 k > 1024,
// .pmm.matmul, int8 rows) runs on the root of a longer list.
int list_root() {
  std::lock_guard<std::mutex> lk(g_devs_mu);
  return g_devs.empty() ? -1 : g_devs[0];
}

struct TimingRec {
  const char *name;
  hipEvent_t a, b;
  int dev;
};

// Per-thread, per-device scratch arena.  Host entry points use it on the
// thread's own stream and synchronise before returning; device entry points
// called with workspace = NULL use it on the CALLER's stream and return
// without synchronising.  `ev` is recorded behind the last device-API use, and
// a use on a different stream first waits for it, so two streams never work
// in the same bytes at once.
struct ArenaSlot {
  void *p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  hipStream_t last = nullptr;
  bool used = false;
};

struct ThreadCtx {
  int device = -1;                   // pmm_set_device's choice for host calls (-1: current)
  std::vector<hipStream_t> streams;  // per device, created lazily, never destroyed
  std::vector<hipStream_t> copy_streams;  // per device: host uploads overlapped with compute
  std::vector<ArenaSlot> arena;      // per device
  bool timing = false;
  std::vector<TimingRec> recs;
  // events of read timing records, per device, reused (an event creation per
  // timed launch is host time comparable to a small problem's whole step)
  std::vector<std::vector<hipEvent_t>> free_events;
};
thread_local ThreadCtx t_ctx;

hipEvent_t timing_event(int dev) {
  if ((int)t_ctx.free_events.size() <= dev) t_ctx.free_events.resize(dev + 1);
  auto &v = t_ctx.free_events[dev];
  hipEvent_t e = nullptr;
  if (!v.empty()) {
    e = v.back();
    v.pop_back();
  } else {
    (void)hipEventCreate(&e);
  }
  return e;
}

// Restores the caller's current HIP device when a host entry point switched it.
struct DevScope {
  int prev = -1;
  ~DevScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Probes device `dev` once (gfx950 or a PMM_ERR_NODEVICE failure).
int probe_device(int dev) {
  if (dev < 0 || dev >= kMaxDevices) return fail(PMM_ERR_NODEVICE, "HIP device %d out of range", dev);
  std::lock_guard<std::mutex> lk(g_dev_mu);
  DeviceInfo &di = g_dev[dev];
  if (!di.probed) {
    hipDeviceProp_t p;
    hipError_t e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return fail(PMM_ERR_NODEVICE, "no HIP device %d: %s", dev, hipGetErrorString(e));
    di.probed = true;
    di.arch = p.gcnArchName;
    di.cus = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    di.ok = di.arch.rfind("gfx950", 0) == 0;
  }
  if (!di.ok)
    return fail(PMM_ERR_NODEVICE, "libpmm is built for gfx950 (MI355X); HIP device %d is %s", dev,
                di.arch.c_str());
  return PMM_OK;
}

// CUs to plan for: the probed device's, 256 before any probe (no GPU: the
// planners still run, see pmm_shard_plan).
int device_cus(int dev) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  return (dev >= 0 && dev < kMaxDevices && g_dev[dev].probed) ? g_dev[dev].cus : 256;
}

// Device-pointer entry points (scope == NULL) run on the caller's current
// device and leave it alone.  Host entry points pass a scope: they run on
// `want` (a corpus handle's device), else on pmm_set_device's choice for this
// thread, else on the current device, and restore the current device on return.
int ensure_device(int *dev_out, DevScope *scope = nullptr, int want = -1) {
  int cur = 0;
  HIP_TRY(hipGetDevice(&cur));
  int dev = cur;
  if (scope) dev = want >= 0 ? want : (t_ctx.device >= 0 ? t_ctx.device : cur);
  if (int rc = probe_device(dev)) return rc;
  if (dev != cur) {
    HIP_TRY(hipSetDevice(dev));
    scope->prev = cur;
  }
  *dev_out = dev;
  return PMM_OK;
}

int thread_stream(int dev, hipStream_t *s, bool copy = false) {
  std::vector<hipStream_t> &v = copy ? t_ctx.copy_streams : t_ctx.streams;
  if ((int)v.size() <= dev) v.resize(dev + 1, nullptr);
  if (!v[dev]) HIP_TRY(hipStreamCreateWithFlags(&v[dev], hipStreamNonBlocking));
  *s = v[dev];
  return PMM_OK;
}

// Grow-only per-thread, per-device scratch (see ArenaSlot).  A use on another
// stream than the last device-API use waits for that use's event; growing
// waits for both, so in-flight work never sees its buffer freed.
int arena(int dev, hipStream_t s, size_t bytes, void **p) {
  if ((int)t_ctx.arena.size() <= dev) t_ctx.arena.resize(dev + 1);
  ArenaSlot &a = t_ctx.arena[dev];
  if (!a.ev) HIP_TRY(hipEventCreateWithFlags(&a.ev, hipEventDisableTiming));
  if (a.used && a.last != s) HIP_TRY(hipStreamWaitEvent(s, a.ev, 0));
  if (a.bytes < bytes) {
    if (a.p) {
      if (a.used) HIP_TRY(hipEventSynchronize(a.ev));
      HIP_TRY(hipStreamSynchronize(s));
      HIP_TRY(hipFree(a.p));
      a.p = nullptr;
      a.bytes = 0;
    }
    size_t want = bytes + bytes / 8;
    HIP_TRY(hipMalloc(&a.p, want));
    a.bytes = want;
  }
  // debug knob (read per call, so a test can toggle it): PMM_ARENA_POISON = a
  // byte value, decimal or 0x..: the whole slot, slack included, is filled with
  // it on this use's stream, behind the waits above and ahead of everything the
  // caller enqueues, so a call that reads scratch it has not written reads the
  // poison instead of an earlier call's leftovers.  Every entry acquires the
  // arena once per call and per device, so no fill lands on bytes still in use.
  if (const char *pe = getenv("PMM_ARENA_POISON")) {
    char *end = nullptr;
    const long v = strtol(pe, &end, 0);
    if (end != pe) HIP_TRY(hipMemsetAsync(a.p, (int)(v & 0xFF), a.bytes, s));
  }
  *p = a.p;
  return PMM_OK;
}

// Marks the end of a device-API use of the arena on stream s (no host sync).
int arena_record(int dev, hipStream_t s) {
  ArenaSlot &a = t_ctx.arena[dev];
  HIP_TRY(hipEventRecord(a.ev, s));
  a.last = s;
  a.used = true;
  return PMM_OK;
}

size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
// Consecutive regions of an arena, each starting 256-byte aligned.
struct Layout {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += al256(bytes);
    return o;
  }
};
int next_pow2(int x, int lo = 64) {
  int p = lo;
  while (p < x) p <<= 1;
  return p;
}
int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// What the rows of one type (PMM_DTYPE_*) look like on the device, wherever
// they sit (a call's arena, a corpus handle's shard): the one statement of the
// element and norm widths, the padding rule and the norm arrays kept per row.
struct RowKind {
  size_t elem;       // bytes of a row element
  int64_t align;     // elements a row's zero-padded stride is a multiple of (the kernels' K step)
  size_t norm_elem;  // bytes of a norm
  // norm arrays per row, n entries each.  The f32 layout (f32 and bf16 rows,
  // the latter's of the rounded rows): [norm | 1/norm | squared norm | squared
  // norm * (1 - 2^-18)]; f64: [norm | squared norm].
  int norm_arrays;
  int euclid_array;  // which of them euclidean reads (cosine reads array 0, dot none)
  // the offset, in norms, of the array `metric` reads in a shard of n rows (-1: none)
  int64_t norm_offset(int metric, int64_t n) const {
    return metric == kMetricCosine ? 0 : metric == kMetricEuclidean ? euclid_array * n : -1;
  }
};
RowKind row_kind(int dtype) {
  switch (dtype) {
    case PMM_DTYPE_F64: return RowKind{8, 16, 8, 2, 1};
    case PMM_DTYPE_BF16: return RowKind{2, kBf16DAlign, 4, 4, 2};
    // int8: [u32 sum of squares | f32 1 / sqrt(sum)]; the i8 entries read both by name
    case PMM_DTYPE_I8: return RowKind{1, kI8DAlign, 4, 2, 0};
    // bit rows (d = w packed bytes): [u32 popcount]
    case PMM_DTYPE_BITS: return RowKind{1, kBitsAlign, 4, 1, 0};
    default: return RowKind{4, 32, 4, 4, 2};
  }
}
// The row stride, in elements, of d columns of this row type.
int64_t padded_dim(int dtype, int64_t d) {
  const int64_t a = row_kind(dtype).align;
  return cdiv(d, a) * a;
}

struct Timed {
  hipStream_t s;
  TimingRec rec{};
  bool on;
  Timed(const char *name, hipStream_t st) : s(st), on(t_ctx.timing) {
    if (on) {
      rec.name = name;
      (void)hipGetDevice(&rec.dev);
      rec.a = timing_event(rec.dev);
      rec.b = timing_event(rec.dev);
      (void)hipEventRecord(rec.a, s);
    }
  }
  ~Timed() {
    if (on) {
      (void)hipEventRecord(rec.b, s);
      t_ctx.recs.push_back(rec);
    }
  }
};

// ---------------------------------------------------------------------------
// Work decomposition of the persistent GEMM: units = QB query blocks x S
// corpus splits of tps tiles.  Minimise rounds * (tps + overhead) over all tps
// so the last round of units fills the chip, subject to the candidate-buffer
// memory budget (M * S * capg * 8 bytes).
// ---------------------------------------------------------------------------
struct Plan {
  int variant = 0;
  int QB = 0, T = 0, tps = 0, S = 0, units = 0, grid = 0, capg = 0, P = 0, qb_full = 0;
  int ctrig = 0;  // compaction trigger (GemmF32Args::ctrig)
  int segs = 0;   // candidate segments per row (S, or 2 S for the column-split f32 variant)
  size_t off_counter = 0, off_gthr = 0, off_cnt = 0, off_cand = 0, off_qn = 0, off_cn = 0;
  size_t off_wq = 0;
  // fire-and-forget bf16 kernel (variant -6): guess sample size and rank,
  // region capacity; survivor counts, regions, the re-run row list
  int ff_ns = 0, ff_j = 0, ffcap = 0;
  size_t off_ffcnt = 0, off_ffreg = 0, off_fb = 0;
  size_t total = 0;
};

void plan_units(int64_t m, int64_t n, int bm, int bn, int cus, double unit_overhead, int64_t max_S,
                Plan &p, bool whole_blocks = false) {
  p.QB = (int)cdiv(m, bm);
  p.T = (int)cdiv(n, bn);
  double best = 1e300;
  int best_tps = p.T;
  for (int tps = 1; tps <= p.T; tps++) {
    const int64_t S = cdiv(p.T, tps);
    if (S > max_S) continue;
    if (tps > 1 && cdiv(p.T, tps - 1) == S) continue;  // same S, fewer tiles: dominated
    const int64_t units = (int64_t)p.QB * S;
    // whole_blocks (wave-specialised bf16 kernel): floor(QB / grid) * grid
    // query blocks run whole, split by split, the rest as split units
    const int64_t grid = std::min<int64_t>(units, cus);
    const int64_t rounds = whole_blocks && p.QB >= grid
                               ? (p.QB / grid) * S + cdiv((p.QB % grid) * S, grid)
                               : cdiv(units, cus);
    const double cost = (double)rounds * (tps + unit_overhead) + 1e-4 * (double)S;
    if (cost < best) {
      best = cost;
      best_tps = tps;
    }
  }
  p.tps = best_tps;
  p.S = (int)cdiv(p.T, p.tps);
  p.units = p.QB * p.S;
  p.grid = (int)std::min<int64_t>(p.units, cus);
  p.qb_full = (whole_blocks && p.QB >= p.grid) ? (p.QB / p.grid) * p.grid : 0;
}

// Tile-shape variant: PMM_GEMM_VARIANT overrides; otherwise the preferred
// order below, skipping variants whose LDS (staging + per-wave scratch) does
// not fit in the CU's 160 KiB.
// Small problems (fewer than 4 x CUs 256 x 256 tiles: the reference's own
// 1000 x 10000 benchmark size) fill the chip better with 128 x 128 tiles.
int choose_variant(int mode, int capg, int64_t m = 1 << 30, int64_t n = 1 << 30, int cus = 256) {
  // (read per call, so a test can force each variant in turn)
  const char *ev = getenv("PMM_GEMM_VARIANT");
  const int env = ev ? atoi(ev) : -1;
  if (env >= 0 && env < 6 && (env != 5 || mode == 0) && gemm_f32_lds_bytes(env, mode, capg) <= 160 * 1024)
    return env;
  if (cdiv(m, 256) * cdiv(n, 256) < 4 * (int64_t)cus && gemm_f32_lds_bytes(0, mode, capg) <= 160 * 1024) {
    // 128 x 128 tiles, or for the fused top-k 128 x 64 (variant 4) when its
    // finer units give a shorter makespan: per unit, tps tiles of bn / 128
    // (128-column tile times, the thin tile's extra overhead at 12%) plus
    // half a tile of unit start.  c1: 3 tiles per unit on 216 CUs, or 5 thin
    // tiles on 256 -> fused kernel 82 -> 76 us, c2 80 -> 74-75
    // (profiles/r3_c1/variant4_ab.txt).
    if (mode == 0 && gemm_f32_lds_bytes(4, mode, capg) <= 160 * 1024) {
      auto makespan = [&](int v) {
        Plan q;
        plan_units(m, n, gemm_f32_bm(v), gemm_f32_bn(v), cus, 0.5, 1 << 20, q);
        const double tile = gemm_f32_bn(v) / 128.0 * (v == 4 ? 1.12 : 1.0);
        return (double)cdiv(q.units, cus) * (q.tps * tile + 0.5);
      };
      if (makespan(4) < makespan(0)) return 4;
    }
    return 0;
  }
  // measured on c3 (100k x 1M x 768 cosine k=100): v3 136.9, v2 133.1, v1 120.5 TFLOP/s
  static const int order[4] = {3, 2, 0, 1};
  for (int v : order)
    if (gemm_f32_lds_bytes(v, mode, capg) <= 160 * 1024) return v;
  return 0;
}

// bf16 kernel choice: the wave-specialised kernel (pmm_bf16_ws_kernel.h)
// whenever its LDS carve holds the compaction scratch (k <= 448);
// PMM_BF16_WS=0 forces the one-wave-per-SIMD kernel (pmm_bf16_kernel.h).
// Read per call, so tests can exercise both.
bool bf16_ws_enabled(int capg, int64_t d) {
  const char *e = getenv("PMM_BF16_WS");
  if (e && atoi(e) == 0) return false;
  const int dp = (int)padded_dim(PMM_DTYPE_BF16, d);
  return capg <= kBf16WsMaxCapg && gemm_bf16_ws_lds_bytes(capg, dp) <= 160 * 1024;
}



// compute = PMM_COMPUTE_F32: the f32 kernel (variant chosen by LDS fit);
// PMM_COMPUTE_BF16: the wave-specialised bf16 kernel (variant -2, 128 x 64
// tiles, 8 waves) or the 4-wave one (variant -1, 128 x 128 tiles).
// Fire-and-forget 256-row bf16 kernel (pmm_bf16_ff_kernel.h): PMM_BF16_FF=1
// (read per call).  Needs a corpus long enough for its guessed threshold: a
// sample of ns_g <= n / 16 rows whose j-th best leaves about n j / ns_g >= 4 k
// scores per row, N < 2^26, and a padded D the kernel's registers hold.
int ff_guess_j() {
  const char *e = getenv("PMM_FF_J");
  return e ? std::max(1, atoi(e)) : 5;
}
int64_t ff_guess_ns(int64_t n) { return std::min<int64_t>(2048, (n / 16) / 32 * 32); }
// The kernel is not part of the product library (it measured slower than the
// wave-specialised kernel): it is compiled into
// libpmm_ff.so (`make ff`, -DPMM_WITH_FF), which the GPU tests load beside
// libpmm.so as the shipped kernel's bit-exact cross-check.
bool bf16_ff_enabled(int64_t k, int64_t n, int64_t d) {
#ifndef PMM_WITH_FF
  (void)k, (void)n, (void)d;
  return false;
#else
  const char *e = getenv("PMM_BF16_FF");
  const int mode = e ? atoi(e) : 0;  // 2 (tests): whenever the kernel can run, however bad the guess
  if (mode == 0) return false;
  const int dp = (int)padded_dim(PMM_DTYPE_BF16, d);
  const int64_t ns = ff_guess_ns(n);
  const bool guess_ok = (double)n * ff_guess_j() / (double)ns >= 4.0 * (double)k;
  return ns >= 256 && ns >= ff_guess_j() && (guess_ok || mode == 2) && k + 64 <= 8192 && n < (1 << 26) &&
         gemm_bf16_ff_lds_bytes(dp) > 0 && gemm_bf16_ff_lds_bytes(dp) <= 160 * 1024;
#endif
}

// allow_ff = false: the re-run of the rows the fire-and-forget kernel could not
// prove exact (they go to the wave-specialised kernel).
int plan_topk(int64_t m, int64_t n, int64_t d, int64_t k, int metric, int cus, Plan &p,
              int compute = PMM_COMPUTE_F32, bool allow_ff = true) {
  // testing knob: plan for fewer workgroups (small problems then take the
  // whole-query-block schedule that only full-size runs reach otherwise);
  // read per call so a test can set and clear it
  if (const char *ce = getenv("PMM_CUS")) {
    const int c = atoi(ce);
    if (c > 0 && c < cus) cus = c;
  }
  // Candidate buffer capacity per (row, split): a compaction keeps k, so a
  // bigger buffer compacts less often but prunes with an older threshold.
  // With selection-based compaction (wave_kth_u64, capg <= 512) 1.5x the
  // power of two measured best (c4 155 -> 151 ms, c3 1082 -> 1077 ms);
  // beyond 512 the compaction sorts, which needs a power of two.
  p.capg = next_pow2((int)k + 64, 128);
  if (p.capg * 3 / 2 <= 512) p.capg = p.capg * 3 / 2;
  {
    // experiment knob: candidate buffer capacity (>= k + 64, multiple of 8)
    const int cap_env = getenv("PMM_CAPG") ? atoi(getenv("PMM_CAPG")) : 0;  // (per call)
    if (cap_env > 0 && k + 64 <= 512) p.capg = std::max<int>(((int)k + 64 + 7) / 8 * 8, std::min(cap_env, 512) / 8 * 8);
  }
  const bool bf16 = compute == PMM_COMPUTE_BF16;
  const bool ffk = bf16 && allow_ff && bf16_ff_enabled(k, n, d);
  const bool ws = bf16 && !ffk && bf16_ws_enabled(p.capg, d);
  // the wave-specialised kernel on 16x16x32: twice the power of two (512 at
  // k = 100) compacts less often; c4 alternated twice on one box: 131.0 /
  // 130.5 vs 132.0 / 131.5 ms per launch (256: 135.4 / 135.0;
  // profiles/r4_ws16/capg_ab.txt)
  if (ws && !getenv("PMM_CAPG") && 2 * next_pow2((int)k + 64, 128) <= kBf16WsMaxCapg &&
      bf16_ws_enabled(2 * next_pow2((int)k + 64, 128), d))
    p.capg = 2 * next_pow2((int)k + 64, 128);
  p.variant = bf16 ? (ffk ? -6 : ws ? -2 : -1) : choose_variant(0, p.capg, m, n, cus);
  const int bm = bf16 ? (ffk ? kBf16FfBM : kBf16BM) : gemm_f32_bm(p.variant);
  const int bn = bf16 ? (ffk ? kBf16FfBN : ws ? kBf16WsBN : kBf16BN) : gemm_f32_bn(p.variant);
  const size_t per_S = (size_t)m * p.capg * 8 + (size_t)m * 4;
  const size_t cand_budget = size_t(8) << 30;
  int64_t max_S = std::max<int64_t>(1, (int64_t)(cand_budget / std::max<size_t>(per_S, 1)));
  // a bf16 unit starts by loading its 128 query rows into registers (about
  // two tiles' worth of time): longer splits amortise it
  // Wave-specialised kernel: floor(QB / grid) * grid query blocks run whole
  // (one workgroup carries a block's row state across all splits: 46% fewer
  // survivors at c4), the rest as split units.  Measured 9% slower with the
  // LDS-sort compaction (the longer-lived buffers compact twice as often);
  // with selection-based compaction 2% faster at c4 (149.5 -> 146.8 ms) and
  // the merge reads one segment per row.  PMM_BF16_WHOLE=0: split units only.
  const char *we = getenv("PMM_BF16_WHOLE");
  const char *fe = getenv("PMM_F32_WHOLE");
  // f32 kernel: the same split of units (PMM_F32_WHOLE=0: split units only).
  // At c3 the GEMM time is unchanged (1076 ms either way) and the merge reads
  // 0.89 GB instead of 2.17 GB (0.40 vs 0.65 ms).
  const bool whole = bf16 ? (ws && !ffk && !(we && atoi(we) == 0)) : !(fe && atoi(fe) == 0);
  // unit overhead in tiles: loading the unit's query rows into registers
  // (Two 128 x 128 f32 workgroups per CU -- 196 registers and 74 KiB of LDS
  // let them co-reside -- planned for 512 slots measured slower at c1: 0.129
  // vs 0.118 ms, profiles/r3_c1/wpc_variant_ab.txt.)
  plan_units(m, n, bm, bn, cus, bf16 ? (ffk ? 8.0 : ws ? 4.0 : 2.0) : 0.5, max_S, p, whole);
  if (ffk) {
    // expected survivors of the guessed threshold per row, n j / ns, and per
    // (row, split); a row's count varies with the sample's j-th (a Gamma(j)
    // quantile: 3x the mean is rare), a region's (64 rows) much less
    p.ff_ns = (int)ff_guess_ns(n);
    p.ff_j = ff_guess_j();
    const double e_row = (double)n * p.ff_j / p.ff_ns;
    const double e_rs = e_row * std::min<double>(1.0, (double)p.tps * bn / (double)n);
    p.capg = (int)std::max<int64_t>(k + 64, ((int64_t)(3.0 * e_rs) + 64 + 63) / 64 * 64);
    // (the seed's sample of ns scores per row lives in the candidate lists)
    p.capg = (int)std::max<int64_t>(p.capg, cdiv((int64_t)p.ff_ns, 2 * p.S));
    p.ffcap = (int)(((int64_t)(1.5 * 64.0 * e_rs) + 256 + 63) / 64 * 64);
    if (const char *ce = getenv("PMM_FF_CAP")) p.ffcap = std::max(64, atoi(ce));  // (tests: force overflows)
  }
  // Compaction trigger: a row's buffer is compacted (its k-th selected, the
  // row threshold raised to it) once it holds more than ctrig entries.  A
  // drain round adds at most 64 per row, so ctrig <= capg - 64.
  p.ctrig = p.capg - 64;
  if (const char *te = getenv("PMM_CTRIG")) {  // (experiment knob, per call)
    const int t = atoi(te);
    if (t > 0) p.ctrig = std::max<int>((int)k + 8, std::min(t, p.capg - 64));
  }
  // merge_kernel's per-row LDS capacity: at least 512, so a row's candidate
  // lists rarely need a compaction before the final one (c1: ~400 survivors
  // of the seed threshold per row; P = 128 compacted ~6 times, 23 us)
  p.P = std::min(8192, std::max(512, next_pow2(2 * (int)k + 64, 128)));
  size_t off = 0;
  p.off_counter = off;
  off += 256;
  p.off_gthr = off;
  off = al256(off + (size_t)m * 8);
  p.segs = p.S * (bf16 ? 1 : gemm_f32_segs(p.variant));
  p.off_cnt = off;
  off = al256(off + (size_t)m * p.segs * 4);
  p.off_cand = off;
  off = al256(off + (size_t)m * p.segs * p.capg * 8);
  p.off_qn = off;  // [norms m | inverse norms m]
  off = al256(off + (metric != kMetricDot ? (size_t)m * 8 : 0));
  p.off_cn = off;  // [norms n | inverse norms n]
  off = al256(off + (metric != kMetricDot ? (size_t)n * 8 : 0));
  p.off_wq = off;  // f32 kernel: per-wave survivor queues, grid x waves x (32 x BN) u64
  off = al256(off + (bf16 ? 0 : (size_t)p.grid * gemm_f32_nw(p.variant) * 32 * bn * 8));
  if (ffk) {
    p.off_ffcnt = off;  // [units][4 waves]
    off = al256(off + (size_t)p.units * 4 * 4);
    p.off_ffreg = off;  // [units][4 waves][ffcap]
    off = al256(off + (size_t)p.units * 4 * p.ffcap * 8);
    p.off_fb = off;  // [count | rows m]
    off = al256(off + 16 + (size_t)m * 4);
  }
  p.total = off;
  (void)d;
  return PMM_OK;
}

// Materialised path (k > kFusedMaxK, f32): rows per chunk and workspace.
struct MatPlan {
  int64_t rows = 0;
  int P = 0, P2 = 0;
  bool global_sort = false;
  size_t off_counter = 0, off_qn = 0, off_cn = 0, off_scores = 0, off_keys = 0, total = 0;
};

void plan_materialise(int64_t m, int64_t n, int64_t k, size_t elem, MatPlan &p) {
  p.P = next_pow2(2 * (int)std::min<int64_t>(k, 1 << 20) + 64, 128);
  p.global_sort = (k > (kRowSelMaxP - 64) / 2) || p.P > kRowSelMaxP;
  p.P2 = p.global_sort ? next_pow2((int)n, 2) : 0;
  size_t per_row = (size_t)n * elem + (p.global_sort ? (size_t)p.P2 * 16 : 0);
  p.rows = std::max<int64_t>(1, std::min<int64_t>(m, (int64_t)(materialise_budget() / per_row)));
  size_t off = 0;
  p.off_counter = off;
  off += 256;
  p.off_qn = off;
  off = al256(off + (size_t)m * elem);
  p.off_cn = off;
  off = al256(off + (size_t)n * elem);
  p.off_scores = off;
  off = al256(off + (size_t)p.rows * n * elem);
  p.off_keys = off;
  off = al256(off + (p.global_sort ? (size_t)p.rows * p.P2 * 16 : 0));
  p.total = off;
}

// Page-locks a caller's host output buffer for the duration of a call so the
// D2H copy of an m x n result runs at full link rate instead of through the
// runtime's pageable staging (PMM_PIN_OUTPUT=0 disables; a failed
// registration just leaves the copy pageable).
struct HostPin {
  void *p = nullptr;
  HostPin(void *ptr, size_t bytes) {
    static const bool on = !(getenv("PMM_PIN_OUTPUT") && atoi(getenv("PMM_PIN_OUTPUT")) == 0);
    // already page-locked (pmm_host_alloc's buffers, or the caller's): nothing to do
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess && at.type == hipMemoryTypeHost) return;
    (void)hipGetLastError();
    if (on && bytes >= (size_t(8) << 20) && hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess)
      p = ptr;
    else
      (void)hipGetLastError();
  }
  ~HostPin() {
    if (p) (void)hipHostUnregister(p);
  }
};

int check_metric(int metric) {
  if (metric != kMetricCosine && metric != kMetricDot && metric != kMetricEuclidean)
    return fail(PMM_ERR_ARG, "invalid metric id %d", metric);
  return PMM_OK;
}

// Store-mode GEMM over rows [0, rows) of q into out (ldo), raw or transformed.
// counter_zeroed: the caller's fill already zeroed *counter (no extra launch).
int gemm_store_f32(const float *q, int64_t ldq, int64_t rows, const float *c, int64_t ldc, int64_t n,
                   int64_t d, int metric, int store_metric, const float *qn, const float *cn,
                   float *out, int64_t ldo, unsigned *counter, int cus, hipStream_t s,
                   const char *label = nullptr, bool counter_zeroed = false) {
  Plan p;
  p.variant = choose_variant(1, 0, rows, n, cus);
  plan_units(rows, n, gemm_f32_bm(p.variant), gemm_f32_bn(p.variant), cus, 0.1, 1 << 20, p);
  GemmF32Args a{};
  a.q = q;
  a.c = c;
  a.qn = qn;
  a.cn = cn;
  a.ldq = ldq;
  a.ldc = ldc;
  a.M = (int)rows;
  a.N = (int)n;
  a.D = (int)d;
  a.k = 0;
  a.capg = 0;
  a.metric = metric;
  a.QB = p.QB;
  a.S = p.S;
  a.tps = p.tps;
  a.ntiles = p.T;
  a.units = p.units;
  a.counter = counter;
  a.out = out;
  a.ldo = ldo;
  a.store_metric = store_metric;
  if (!counter_zeroed) HIP_TRY(hipMemsetAsync(counter, 0, 4, s));
  Timed t(label ? label : (store_metric ? "gemm_f32_scores" : "gemm_f32_matmul"), s);
  HIP_TRY(launch_gemm_f32(a, p.variant, 1, p.grid, s));
  return PMM_OK;
}

// ---------------------------------------------------------------------------
// Argument builders: every fused launch (the f32 kernel, the bf16 kernels, the
// screen) and every merge fills its arguments here, so a workspace offset or a
// knob is read in one place.
// ---------------------------------------------------------------------------
// The fields every fused launch shares: shape, work decomposition and the
// plan's workspace regions at base w.  The caller adds its operands (rows,
// norms, strides).
GemmF32Args fused_args(int64_t m, int64_t n, int64_t dp, int64_t k, int metric, const Plan &p, char *w) {
  GemmF32Args a{};
  a.M = (int)m;
  a.N = (int)n;
  a.D = (int)dp;
  a.k = (int)k;
  a.capg = p.capg;
  a.ctrig = p.ctrig;
  a.metric = metric;
  a.QB = p.QB;
  // The kernels index a row's candidate segments with S.  The f32 kernel's
  // column-split variant keeps two segments per corpus split (segs = 2 S);
  // every other kernel has segs == S.
  a.S = p.segs;
  a.tps = p.tps;
  a.ntiles = p.T;
  a.units = p.units;
  a.qb_full = p.qb_full;
  a.counter = (unsigned *)(w + p.off_counter);
  a.cand = (unsigned long long *)(w + p.off_cand);
  a.wq = (unsigned long long *)(w + p.off_wq);
  a.cnt = (unsigned *)(w + p.off_cnt);
  a.gthr = (unsigned long long *)(w + p.off_gthr);
  return a;
}

// The bf16 kernels' launch knobs (the screen runs the same kernel: they hold
// there too).  Read once per process.
void set_bf16_knobs(GemmF32Args &a) {
  a.nst = 3;  // LDS ring slots of the bf16 kernel
  a.pf = 1;
  static const int defer_env = getenv("PMM_BF16_DEFER") ? atoi(getenv("PMM_BF16_DEFER")) : 1;
  a.defer = defer_env;
  static const int sync_env = getenv("PMM_BF16_SYNC") ? atoi(getenv("PMM_BF16_SYNC")) : 1;
  a.round_sync = sync_env;
  // round-barrier spin limit: workgroups of one round finish up to a few ms
  // apart (uneven epilogues); a workgroup that times out stops syncing
  static const int tmo_env = getenv("PMM_BF16_SYNC_TIMEOUT_US") ? atoi(getenv("PMM_BF16_SYNC_TIMEOUT_US")) : 20000;
  a.sync_timeout = tmo_env * 100;
}

// merge_kernel's loader 0: the candidate segments a fused launch with
// arguments `a` left, into m x k lists.
MergeArgs merge_cand_args(const GemmF32Args &a, const Plan &p, uint32_t index_base, uint32_t *out_idx,
                          float *out_score) {
  MergeArgs ma{};
  ma.cand = a.cand;
  ma.cnt = a.cnt;
  ma.gthr = a.gthr;
  ma.capg = p.capg;
  ma.M = a.M;
  ma.S = p.segs;
  ma.k_out = a.k;
  ma.P = p.P;
  ma.metric = a.metric;
  ma.index_base = index_base;
  ma.out_idx = out_idx;
  ma.out_score = out_score;
  return ma;
}

// merge_kernel's loader 1: `lists` (idx, score) lists of k_in entries per row
// (chunks of one corpus, device shards, the strided merge API; see MergeArgs
// for the strides).  sorted: every list is best-first, e.g. a top-k output.
MergeArgs merge_lists_args(const uint32_t *idx, const float *score, int64_t m, int64_t lists, int64_t k_in,
                           int64_t row_stride, int64_t list_stride, int64_t k_out, int metric, bool sorted,
                           uint32_t *out_idx, float *out_score) {
  MergeArgs ma{};
  ma.in_idx = idx;
  ma.in_score = score;
  ma.k_in = (int)k_in;
  ma.row_stride = row_stride;
  ma.list_stride = list_stride;
  ma.M = (int)m;
  ma.S = (int)lists;
  ma.sorted = sorted ? 1 : 0;
  ma.k_out = (int)k_out;
  ma.P = std::min(8192, next_pow2(2 * (int)k_out + 64, 128));
  ma.metric = metric;
  ma.out_idx = out_idx;
  ma.out_score = out_score;
  return ma;
}

// The call's workspace: the caller's when one is given (and large enough),
// else the thread's arena, whose use done() marks at the end of the call.
struct Workspace {
  char *w = nullptr;
  bool own = false;
  int dev = 0;
  hipStream_t s = nullptr;
  int done() const { return own ? arena_record(dev, s) : PMM_OK; }
};
int acquire_workspace(void *ws, size_t ws_bytes, size_t need, int dev, hipStream_t s, Workspace &out) {
  out.own = !ws;
  out.dev = dev;
  out.s = s;
  if (!ws) {
    if (int rc = arena(dev, s, need, &ws)) return rc;
  } else if ((uintptr_t)ws & 15) {
    // (the regions start at multiples of 256 from ws and hold 64-bit keys that
    // are updated atomically, 16-byte fills and the rows the kernels stage with
    // 16-byte loads)
    return fail(PMM_ERR_ARG, "the workspace needs a 16-byte-aligned address (got %p)", ws);
  } else if (ws_bytes < need) {
    return fail(PMM_ERR_ARG, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  }
  out.w = (char *)ws;
  return PMM_OK;
}

// One fused f32 pass (gemm_f32_kernel + merge_kernel) with arguments `a` over
// a planned workspace whose work counter and shared thresholds are already
// set (the caller has zeroed [w, w + p.off_cand): counter, thresholds, counts).
hipError_t run_fused_f32(GemmF32Args a, const Plan &p, uint32_t index_base, uint32_t *out_idx, float *out_score,
                         hipStream_t s) {
  // whole query blocks first (see gemm_f32_kernel's unit decode)
  if (p.qb_full) a.units = (int)(p.qb_full + (int64_t)(p.QB - p.qb_full) * p.S);
#ifdef PMM_LAB
  {
    static const int ablate = getenv("PMM_ABLATE") ? atoi(getenv("PMM_ABLATE")) : 0;
    a.ablate = ablate;
  }
  // per-phase cycle counters of the f32 kernel (make lab LAB=-DPMM_F32_STATS,
  // PMM_STATS=1): summed over waves, printed per call
  static const bool f32_stats = getenv("PMM_STATS") != nullptr;
  static unsigned long long *f32_stats_buf = nullptr;
  if (f32_stats) {
    if (!f32_stats_buf) {
      hipError_t e = hipMalloc(&f32_stats_buf, 128);
      if (e != hipSuccess) return e;
    }
    hipError_t e = hipMemsetAsync(f32_stats_buf, 0, 128, s);
    if (e != hipSuccess) return e;
    a.stats = f32_stats_buf;
  }
#endif
  {
    // (a mark beside the launch's record: pmm_timing_read matches substrings,
    // so the tile variant has a name of its own)
    static const char *const kVariant[6] = {"f32_variant/0", "f32_variant/1", "f32_variant/2",
                                            "f32_variant/3", "f32_variant/4", "f32_variant/5"};
    if (p.variant >= 0 && p.variant < 6) Timed mark(kVariant[p.variant], s);
  }
  {
    Timed t("gemm_f32_topk", s);
    hipError_t e = launch_gemm_f32(a, p.variant, 0, p.grid, s);
    if (e != hipSuccess) return e;
  }
#ifdef PMM_LAB
  if (f32_stats) {
    unsigned long long h[16];
    hipError_t e = hipMemcpyAsync(h, f32_stats_buf, 128, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    fprintf(stderr,
            "[pmm stats] gemm_f32 variant %d: units %d, S %d, tps %d, grid %d; wave cycles (sum): total %.4g, "
            "unit setup %.4g, K loops %.4g (barriers %.4g), epilogues %.4g (pre-filter + queueing %.4g, "
            "compactions %.4g; CNL flags + prefix sum %.4g); wave-tiles %llu, queued survivors %llu\n",
            p.variant, p.units, p.S, p.tps, p.grid, (double)h[0], (double)h[4], (double)h[2], (double)h[1],
            (double)h[3], (double)h[6], (double)h[7], (double)h[9], h[5], h[8]);
    a.stats = nullptr;
  }
#endif
  MergeArgs ma = merge_cand_args(a, p, index_base, out_idx, out_score);
#ifdef PMM_LAB
  {
    static const int ablate = getenv("PMM_MERGE_ABLATE") ? atoi(getenv("PMM_MERGE_ABLATE")) : 0;
    ma.ablate = ablate;
  }
#endif
  Timed t("merge_topk", s);
  return launch_merge(ma, 0, s);
}

// ---------------------------------------------------------------------------
// Screened f32 top-k (cosine).  The wave-specialised bf16
// kernel runs over bf16 images of Q and C as a conservative screen -- it keeps
// every column whose exact score could reach the row's k-th, by a proven
// slack -- and the few hundred kept candidates per row are re-scored with the
// f32 path's arithmetic, so indices, scores and tie order are the f32
// kernel's bit for bit at about 1/16 of its matrix-pipe time.
// ---------------------------------------------------------------------------
// Whether the bf16 MFMA kernels take the shape themselves (see the bf16
// compute path below for their limits).
bool bf16_native(int64_t d, int64_t k, int64_t n) {
  return padded_dim(PMM_DTYPE_BF16, d) <= kBf16MaxD && n < (int64_t(1) << 27) &&
         next_pow2((int)std::min<int64_t>(k, 1 << 20) + 64, 128) <= kBf16MaxCapg;
}
constexpr int64_t kScreenMaxK = 192;      // k + its 2 eps band + a drain round fit capg = 512
constexpr int64_t kScreenRerunRows = 1024;  // rows per f32 re-run launch
// m * n * d from which the screen is chosen without the knob.  Below it the
// f32 kernel's launch is short against the screen's fixed passes (rounding the
// corpus, seed, re-score, the count read-back).  Measured at D = 768, k = 100
// (profiles/screen_c3/crossover.json): at 7.7e12 the screen wins 2.1-2.9x in
// both shapes; at 7.7e11 it wins only with a long corpus and few rows (1000 x
// 1M: 9.6 vs 13.3 ms) and loses at 10k x 100k and 100k x 10k; at 7.7e10 and
// below it loses.
constexpr double kScreenMinWork = 4e12, kScreenMinWorkLongCorpus = 5e11;

// The screened path's workspace behind the bf16 kernel's own plan (counter,
// thresholds, counts, candidates, norms), which starts it.
struct ScreenPlan {
  int64_t dpb = 0, dp = 0, rr = 0;
  bool ext = false;  // the corpus image is supplied (a handle's ScreenImage): no off_cb, no off_crel
  size_t off_qb = 0, off_cb = 0, off_rel = 0, off_eps = 0, off_bad = 0, off_ovf = 0, off_scal = 0, off_rows = 0,
         off_crel = 0, off_gq = 0, off_f32 = 0, f32_bytes = 0, total = 0;
};
// The guessed starting bound's slack t: a row's guess aims at rank t k of its
// n scores (launch_screen_guess).  Measured at c3 (profiles/screen_guess/):
// the screen kernel's time falls with t while the rows whose guess was too high
// (re-run by the f32 kernel) grow; the fastest t that keeps those rows under a
// tenth of one re-run launch.
constexpr double kScreenGuessSlack = 4.0;
// z with P(N(0,1) > z) = p, 0 < p < 0.5 (bisection on erfc; called once per call)
double normal_upper_quantile(double p) {
  double lo = 0.0, hi = 40.0;
  for (int i = 0; i < 80; i++) {
    const double mid = 0.5 * (lo + hi);
    if (0.5 * std::erfc(mid / std::sqrt(2.0)) > p) lo = mid;
    else hi = mid;
  }
  return 0.5 * (lo + hi);
}
// Whether a call's shape asks for the screen.  PMM_F32_SCREEN (read per call):
// 0 = never, 1 = wherever the limits allow, unset = from kScreenMinWork.
bool screen_wanted(int64_t m, int64_t n, int64_t d, int64_t k, int metric) {
  if (metric != kMetricCosine || k > kScreenMaxK || !bf16_native(d, k, n)) return false;
  const char *e = getenv("PMM_F32_SCREEN");
  if (e) return atoi(e) != 0;
  const double work = (double)m * (double)n * (double)padded_dim(PMM_DTYPE_F32, d);
  return work >= kScreenMinWork || (work >= kScreenMinWorkLongCorpus && n >= 100 * m);
}
// A corpus' share of the screen's inputs, computed once and kept by an f32
// corpus handle (CorpusShard::screen): what topk_f32_screened derives from C
// other than the exact norms and factors, which the handle holds already.
// Only a corpus without an unsafe row keeps one.
struct ScreenImage {
  uint16_t *cb = nullptr;  // n x roundup(d, 128) bf16 bit patterns, zero-padded
  float *crel = nullptr;   // per row: [residual bound n | unsafe flag n]
  float max_rel = 0.0f;    // the maximum residual bound over the rows
};
size_t screen_image_bytes(int64_t n, int64_t d) {
  return (size_t)n * padded_dim(PMM_DTYPE_BF16, d) * 2 + (size_t)n * 8;
}
// b: the bf16 kernel's plan of the call (padded D = roundup(d, 128));
// corpus_image: the caller supplies a ScreenImage, so the workspace leaves out
// the corpus' bf16 rows and per-row residuals
void plan_screen(int64_t m, int64_t n, int64_t d, int64_t k, int metric, int cus, const Plan &b, ScreenPlan &sp,
                 bool corpus_image = false) {
  sp.dpb = padded_dim(PMM_DTYPE_BF16, d);
  sp.dp = padded_dim(PMM_DTYPE_F32, d);
  sp.ext = corpus_image;
  size_t off = b.total;
  sp.off_qb = off;
  off = al256(off + (size_t)m * sp.dpb * 2);
  sp.off_cb = off;
  if (!corpus_image) off = al256(off + (size_t)n * sp.dpb * 2);
  sp.off_rel = off;
  off = al256(off + (size_t)m * 4);
  sp.off_eps = off;
  off = al256(off + (size_t)m * 4);
  sp.off_bad = off;  // [bad m | ovf m | scal 64 words]: one fill
  off = al256(off + (size_t)m * 4);
  sp.off_ovf = off;
  off = al256(off + (size_t)m * 4);
  sp.off_scal = off;  // [0] max corpus residual, [1] corpus unsafe, [2] re-run rows
  off += 256;
  sp.off_rows = off;
  off = al256(off + (size_t)m * 4);
  sp.off_crel = off;  // per corpus row: [residual n | unsafe flag n]
  if (!corpus_image) off = al256(off + (size_t)n * 8);
  // re-run: gathered query rows, their lists, and the f32 path's own workspace
  // (sized for the whole call, which an unsafe corpus sends there)
  sp.rr = std::min<int64_t>(m, kScreenRerunRows);
  sp.off_gq = off;  // [rows rr x dp | their indices rr x k | their scores rr x k] (rerun_rows' layout)
  off = al256(off + (size_t)sp.rr * sp.dp * 4);
  off = al256(off + (size_t)sp.rr * k * 4);
  off = al256(off + (size_t)sp.rr * k * 4);
  sp.off_f32 = off;
  {
    Plan f;
    plan_topk(m, n, sp.dp, k, metric, cus, f);
    sp.f32_bytes = f.total;
    if (sp.rr < m) {
      plan_topk(sp.rr, n, sp.dp, k, metric, cus, f);
      sp.f32_bytes = std::max(sp.f32_bytes, f.total);
    }
  }
  sp.total = off + sp.f32_bytes;
}

// ---------------------------------------------------------------------------
// The route of one fused top-k call, decided once by route_topk.  Sizing
// (pmm_topk_workspace_bytes), accounting (pmm_topk_merge_bytes) and the
// executors (topk_f32_device_impl, topk_bf16_device_impl) all read it; none
// of them decides again.
// ---------------------------------------------------------------------------
enum class Route {
  kF32Fused,         // gemm_f32_kernel + merge
  kF32Screened,      // bf16 screen + exact f32 re-score (cosine, large)
  kF32Materialised,  // k > kFusedMaxK: score chunks + row select
  kBf16Native,       // the bf16 MFMA kernels (wave-specialised or one-wave, by p.variant)
  kBf16Widened,      // bf16 rows past the bf16 kernels' limits: widened to f32, searched by the f32 path
};
struct TopkRoute {
  Route kind = Route::kF32Fused;
  // A fused kernel leaves candidates to merge_kernel: every route but the
  // materialised one and the widened path's inner search at k > kFusedMaxK.
  bool fused = true;
  // fused: the plan whose candidate counts the merge reads -- the f32
  // kernel's, the bf16 kernel's (native, screened) or the widened path's inner
  // f32 search's
  Plan p;
  ScreenPlan sp;  // screened: the workspace behind p
  MatPlan mp;     // !fused
  // widened: the f32 images of Q at 0 and of C at off_wc, rows of dpw floats,
  // and the inner f32 search's workspace at base
  int64_t dpw = 0;
  size_t off_wc = 0, base = 0;
  size_t total = 0;
};

// allow_screen = false: a caller whose call cannot screen (thresholds carried
// between corpus chunks, cached corpus norms without a screen image, per-device
// shards, the widened bf16 path, the screen's own re-runs); allow_ff = false: the fire-and-forget
// kernel's re-run.
// d may arrive already padded (callers name d, roundup(d, 32) or, for bf16,
// roundup(d, 128)): every decision and size below reads d through one of those
// roundings, so the route is the same.  The one exception is the widened bf16
// path, whose f32 rows are roundup(d, 32) wide: a d padded to 128 sizes more.
// corpus_image = true: the screened route of a corpus handle, whose ScreenImage
// stands for the corpus' share of the screen's workspace (plan_screen).
TopkRoute route_topk(int64_t m, int64_t n, int64_t d, int64_t k, int metric, int compute, int cus,
                     bool allow_screen, bool allow_ff, bool corpus_image = false) {
  TopkRoute r;
  const int64_t dp = padded_dim(PMM_DTYPE_F32, d);
  if (compute == PMM_COMPUTE_BF16) {
    if (bf16_native(d, k, n)) {
      r.kind = Route::kBf16Native;
      plan_topk(m, n, padded_dim(PMM_DTYPE_BF16, d), k, metric, cus, r.p, PMM_COMPUTE_BF16, allow_ff);
      r.total = r.p.total;
      return r;
    }
    r = route_topk(m, n, dp, k, metric, PMM_COMPUTE_F32, cus, false, false);
    r.kind = Route::kBf16Widened;
    r.dpw = dp;
    r.off_wc = al256((size_t)m * dp * 4);
    r.base = r.off_wc + al256((size_t)n * dp * 4);
    r.total += r.base;
    return r;
  }
  if (k > kFusedMaxK) {
    r.kind = Route::kF32Materialised;
    r.fused = false;
    plan_materialise(m, n, k, 4, r.mp);
    r.total = r.mp.total;
    return r;
  }
  if (allow_screen && screen_wanted(m, n, d, k, metric)) {
    // the wave-specialised kernel, with room above k for the kept band before
    // a drain round could pass the segment's end
    plan_topk(m, n, padded_dim(PMM_DTYPE_BF16, d), k, metric, cus, r.p, PMM_COMPUTE_BF16, allow_ff);
    if (r.p.variant == -2 && r.p.capg <= kBf16WsMaxCapg && r.p.ctrig >= k + k / 2 + 32 &&
        r.p.ctrig <= r.p.capg - 64) {
      r.kind = Route::kF32Screened;
      plan_screen(m, n, d, k, metric, cus, r.p, r.sp, corpus_image);
      r.total = r.sp.total;
      return r;
    }
    r.p = Plan();
  }
  r.kind = Route::kF32Fused;
  plan_topk(m, n, dp, k, metric, cus, r.p);
  r.total = r.p.total;
  return r;
}

// Re-runs the query rows listed on the device in rows[0 .. r): gathers them
// (row_bytes of each, at row stride ld_bytes, both multiples of 16) into a
// dense block, has run(block, idx, score, ws) search the block into dense
// r x k lists with a workspace of ws_need bytes, and scatters the lists to the
// rows' places in out_idx / out_score.  Block, lists and workspace lie in
// [buf, buf + buf_bytes) when they fit, else in an allocation of the call's
// own, freed after a stream synchronisation.
template <typename Run>
int rerun_rows(const void *q, int64_t ld_bytes, int64_t row_bytes, const int *rows, int64_t r, int64_t k,
               size_t ws_need, char *buf, size_t buf_bytes, uint32_t *out_idx, float *out_score, hipStream_t s,
               const char *what, Run run) {
  const size_t o_i = al256((size_t)r * row_bytes), o_s = o_i + al256((size_t)r * k * 4),
               o_w = o_s + al256((size_t)r * k * 4);
  char *tmp = nullptr;
  hipError_t e = hipSuccess;
  if (o_w + ws_need > buf_bytes) {
    e = hipMalloc(&tmp, o_w + ws_need);
    buf = tmp;
  }
  uint32_t *gi = (uint32_t *)(buf + o_i);
  float *gs = (float *)(buf + o_s);
  int rc = PMM_OK;
  if (e == hipSuccess) e = launch_gather_rows(q, ld_bytes / 16, rows, (int)r, (int)(row_bytes / 16), buf, s);
  if (e == hipSuccess) rc = run(buf, gi, gs, buf + o_w);
  if (e == hipSuccess && rc == PMM_OK) e = launch_scatter_lists(gi, gs, rows, (int)r, (int)k, out_idx, out_score, s);
  if (tmp) {
    const hipError_t e2 = hipStreamSynchronize(s);  // (before the buffer is freed)
    (void)hipFree(tmp);
    if (e == hipSuccess) e = e2;
  }
  if (e != hipSuccess) return fail(PMM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return rc;
}

// The fused route's executor over its acquired workspace w (p.total bytes).
// d is the logical dimension (norms follow ndarray's order over exactly d
// elements); the GEMM runs over dp = roundup(d, 32), the rows being
// zero-padded up to dp.
// c_norms: optional precomputed corpus norms for `metric` laid out as
// [n norms | n pre-filter factors] (a pmm_corpus handle's cache); NULL =
// compute them in this call.  c_pre (with c_norms): the pre-filter factors
// when they do not follow the norms at c_norms + n (a slice of a handle's
// arrays: one group's segment of a partitioned handle).
// keep_gthr: the workspace's shared per-row thresholds already hold a lower
// bound of the rows' k-th best from earlier corpus chunks (see
// topk_f32_host_chunked); they are kept instead of zeroed, so this chunk
// only returns what can still enter the top-k (possibly fewer than k per row:
// the rest are empty slots, which the chunk merge skips).
int topk_f32_fused(const Plan &p, const float *q, int64_t ldq, int64_t m, const float *c, int64_t ldc, int64_t n,
                   int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *out_idx, float *out_score,
                   char *w, hipStream_t s, int cus, const float *c_norms, bool keep_gthr,
                   const float *c_pre = nullptr) {
  const int64_t dp = padded_dim(PMM_DTYPE_F32, d);
  float *qn = (float *)(w + p.off_qn), *cn = (float *)(w + p.off_cn);
  if (c_norms) cn = const_cast<float *>(c_norms);
  // Threshold seeding.  When every unit spans few corpus tiles (small
  // problems: the reference's own benchmark size), a unit starts cold: its
  // first tile's scores nearly all survive the pre-filter and are re-scored
  // exactly, appended and compacted, which took most of the kernel's time.
  // Instead, the scores of the first ns corpus rows are computed first --
  // by seed_dots_kernel as fmaf chains in natural K order (bit-identical to
  // the main pass's MFMA chain and epilogue arithmetic), or, past its
  // limits or with PMM_SEED_GEMM=1, by the MFMA main loop in store mode into
  // the still unused candidate buffers -- and one wave per row selects the
  // k-th best composite of that sample: (that key - 1) is an exact lower
  // bound of the row's final k-th best and seeds the shared threshold.
  // Sample size max(256, 8k): at c1 128 / 256 / 512 / 1024 rows measured
  // 0.170 / 0.163 / 0.174 / 0.192 ms per call (tools/experiments/gpu_seedns.sh).
  int64_t ns = std::min<int64_t>(n, next_pow2((int)std::max<int64_t>(256, 8 * k), 256));
  if (const char *ne = getenv("PMM_SEED_NS")) ns = std::min<int64_t>(n, std::max<int64_t>(atoll(ne), k));
  const char *se = getenv("PMM_SEED");
  // (only when most query blocks run as split units: a block run whole
  // carries its threshold across the corpus and gains nothing from the
  // seed, which costs m * ns * d fmaf on the vector units -- at a c3 shard
  // of 8, 100k x 125k x 768 with 256 of 391 blocks whole, 9.3 ms for no
  // GEMM time saved; tools/experiments/shard_shapes.py, profiles/r4_shards/)
  const bool mostly_split = 2 * (int64_t)p.qb_full < (int64_t)p.QB;
  bool seed = (se ? atoi(se) != 0
                  : ((int64_t)p.tps * gemm_f32_bn(p.variant) < 8192 && n >= 4 * ns && mostly_split)) &&
              ns >= k && ns < n && ns <= kSeedMaxNs && !keep_gthr && seed_span_fits(ns, ldc, 4) &&
              (size_t)m * ns * 4 <= p.off_qn - p.off_cand;
  GemmF32Args a = fused_args(m, n, dp, k, metric, p, w);
  a.q = q;
  a.c = c;
  a.qn = qn;
  a.cn = cn;
  a.cpre = c_pre ? c_pre : cn + n;
  a.ldq = ldq;
  a.ldc = ldc;
  // Seeded small problems: one prologue launch (seed + norms + fills).
  const bool one_prologue = seed && dp <= kSeedDotsMaxD && ldq % 4 == 0 && ldc % 4 == 0 &&
                            !(((uintptr_t)q | (uintptr_t)c | (uintptr_t)w) & 15) && p.off_gthr % 16 == 0 &&
                            p.off_cnt % 16 == 0 && p.off_cand % 16 == 0 && !getenv("PMM_SEED_GEMM");
  if (one_prologue) {
    {
      // (a mark: which form of seed blocks the prologue takes)
      static const char *const kForm[3] = {"seed_form/fmaf", "seed_form/lds", "seed_form/mfma"};
      Timed mark(kForm[seeded_prologue_form(n, (int)dp, (int)ns)], s);
    }
    Timed t("gemm_f32_seed", s);
    HIP_TRY(launch_seeded_prologue(q, ldq, (int)m, c, ldc, n, (int)d, (int)dp, (int)ns, (int)k, metric, qn, cn,
                                   !c_norms, a.gthr, w, p.off_gthr, w + p.off_cnt, p.off_cand - p.off_cnt, s));
  } else {
    // one fill zeroes the work counters (the main pass's and the seed store
    // pass's), thresholds and buffer counts [0, off_cand); with the norms
    // pair kernel the fill rides in the same launch
    const bool fill_in_norms =
        metric != kMetricDot && !c_norms && !keep_gthr && p.off_cand % 16 == 0 && ((uintptr_t)w & 15) == 0;
    if (keep_gthr) {
      HIP_TRY(hipMemsetAsync(w + p.off_counter, 0, p.off_gthr - p.off_counter, s));
      HIP_TRY(hipMemsetAsync(w + p.off_cnt, 0, p.off_cand - p.off_cnt, s));
    } else if (!fill_in_norms) {
      HIP_TRY(hipMemsetAsync(w, 0, p.off_cand, s));
    }
    if (metric != kMetricDot) {
      const int sq = metric == kMetricEuclidean;
      Timed t("norms_f32", s);
      if (c_norms) HIP_TRY(launch_norms_f32(q, m, d, ldq, sq, qn, nullptr, s));
      else HIP_TRY(launch_norms_pair_f32(q, m, ldq, qn, c, n, ldc, cn, cn + n, d, sq, s,
                                         fill_in_norms ? w : nullptr, fill_in_norms ? p.off_cand : 0));
    }
    if (seed) {
      // PMM_SEED_GEMM=1 or outside the one-launch limits: the sample's
      // scores from the fused kernel's main loop in store mode, then a
      // select launch
      float *sample = (float *)a.cand;
      int rc = gemm_store_f32(q, ldq, m, c, ldc, ns, dp, metric, 1, qn, cn, sample, ns, a.counter + 16, cus, s,
                              "gemm_f32_seed", true);
      if (rc) return rc;
      Timed t("seed_select", s);
      HIP_TRY(launch_seed_select(sample, ns, (int)m, (int)ns, (int)k, metric, a.gthr, s));
    }
  }
  HIP_TRY(run_fused_f32(a, p, index_base, out_idx, out_score, s));
  // (under a keep_gthr chunk merge too: the merge folds the zeros again and
  // takes them back from these lists, launch_zero_sign_lists; an empty slot is
  // skipped)
  HIP_TRY(launch_zero_sign_f32(q, ldq, c, ldc, qn, cn, (int)m, n, (int)d, (int)k, metric, index_base, out_idx,
                               out_score, s));
  return PMM_OK;
}

// The materialised route's executor (k beyond the fused path: score chunks,
// row-selected) over its acquired workspace w (p.total bytes).
int topk_f32_materialised(const MatPlan &p, const float *q, int64_t ldq, int64_t m, const float *c, int64_t ldc,
                          int64_t n, int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *out_idx,
                          float *out_score, char *w, hipStream_t s, int cus, const float *c_norms) {
  const int64_t dp = padded_dim(PMM_DTYPE_F32, d);
  float *qn = (float *)(w + p.off_qn), *cn = (float *)(w + p.off_cn);
  float *sc = (float *)(w + p.off_scores);
  if (c_norms) cn = const_cast<float *>(c_norms);
  if (metric != kMetricDot) {
    const int sq = metric == kMetricEuclidean;
    HIP_TRY(launch_norms_f32(q, m, d, ldq, sq, qn, nullptr, s));
    if (!c_norms) HIP_TRY(launch_norms_f32(c, n, d, ldc, sq, cn, nullptr, s));
  }
  for (int64_t r0 = 0; r0 < m; r0 += p.rows) {
    const int64_t rows = std::min<int64_t>(p.rows, m - r0);
    int rc = gemm_store_f32(q + r0 * ldq, ldq, rows, c, ldc, n, dp, metric, 1, qn + r0, cn, sc, n,
                            (unsigned *)(w + p.off_counter), cus, s);
    if (rc) return rc;
    if (!p.global_sort) {
      RowSelArgs ra{};
      ra.scores = sc;
      ra.lds = n;
      ra.rows = (int)rows;
      ra.N = (int)n;
      ra.k = (int)k;
      ra.P = p.P;
      ra.metric = metric;
      ra.is_f64 = 0;
      ra.index_base = index_base;
      ra.out_idx = out_idx + r0 * k;
      ra.out_score = out_score + r0 * k;
      HIP_TRY(launch_rowselect(ra, s));
    } else {
      HIP_TRY(launch_rowsort_global(sc, n, (int)rows, (int)n, 0, metric, w + p.off_keys, p.P2,
                                    (int)k, index_base, out_idx + r0 * k, out_score + r0 * k, s));
    }
  }
  // (the row select's keys fold the zeros, and the stored scores ran over the padded dimension)
  HIP_TRY(launch_zero_sign_f32(q, ldq, c, ldc, qn, cn, (int)m, n, (int)d, (int)k, metric, index_base, out_idx,
                               out_score, s));
  return PMM_OK;
}

// The screened route's executor over its acquired workspace w (r.total bytes).
// img (with c_norms = the corpus' [norms n | factors n]; r planned with
// corpus_image): a handle's call, which launches nothing over C before the
// seed -- the corpus' share of the inputs is read from the handle -- and
// prepares Q in one pass (screen_prepare_kernel).
int topk_f32_screened(const TopkRoute &r, const float *q, int64_t ldq, int64_t m, const float *c, int64_t ldc,
                      int64_t n, int64_t d, int64_t k, uint32_t index_base, uint32_t *out_idx, float *out_score,
                      char *w, hipStream_t s, int cus, const ScreenImage *img = nullptr,
                      const float *c_norms = nullptr) {
  const int metric = kMetricCosine;
  const ScreenPlan &sp = r.sp;
  const Plan &p = r.p;
  float *qn = (float *)(w + p.off_qn);
  const float *cn = img ? c_norms : (float *)(w + p.off_cn);
  uint16_t *qb = (uint16_t *)(w + sp.off_qb);
  const uint16_t *cb = img ? img->cb : (uint16_t *)(w + sp.off_cb);
  float *rel = (float *)(w + sp.off_rel), *eps = (float *)(w + sp.off_eps);
  unsigned *bad = (unsigned *)(w + sp.off_bad), *ovf = (unsigned *)(w + sp.off_ovf);
  unsigned *scal = (unsigned *)(w + sp.off_scal);
  int *rows = (int *)(w + sp.off_rows);
  HIP_TRY(hipMemsetAsync(w, 0, p.off_gthr + (size_t)m * 8, s));
  if (p.qb_full) HIP_TRY(hipMemsetAsync(w + p.off_cnt, 0, (size_t)m * p.S * 4, s));
  HIP_TRY(hipMemsetAsync(w + sp.off_ovf, 0, sp.off_rows - sp.off_ovf, s));
  if (img) {
    // the query rows' exact norms, image, residuals and flags in one read; the
    // corpus' maximum residual from the handle (scal[1], corpus unsafe, stays 0)
    Timed t("norms_f32/prepare", s);
    HIP_TRY(launch_screen_prepare(q, m, d, ldq, qb, sp.dpb, qn, nullptr, rel, bad, nullptr, s));
    uint32_t bits;
    memcpy(&bits, &img->max_rel, 4);
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)scal, (int)bits, 1, s));
  } else {
    // per operand one read: the exact norms and factors (the unscreened path's
    // bits), the bf16 image, the rounding residuals and the unsafe flags
    Timed t("norms_f32/round", s);
    float *wcn = (float *)(w + p.off_cn), *crel = (float *)(w + sp.off_crel);
    HIP_TRY(launch_screen_prepare(q, m, d, ldq, qb, sp.dpb, qn, nullptr, rel, bad, nullptr, s));
    HIP_TRY(launch_screen_prepare(c, n, d, ldc, (uint16_t *)(w + sp.off_cb), sp.dpb, wcn, wcn + n, crel,
                                  (unsigned *)(crel + n), scal, s));
  }
  GemmF32Args a = fused_args(m, n, sp.dpb, k, metric, p, w);
  a.qb = qb;
  a.cb = cb;
  a.qn = qn;
  a.cn = cn;
  a.cpre = cn + n;
  a.ldq = sp.dpb;
  a.ldc = sp.dpb;
  set_bf16_knobs(a);
  const bool debug = getenv("PMM_SCREEN_DEBUG") != nullptr;
  a.eps = eps;
  a.ovf = ovf;
  {
    // the bf16 kernel's seed over the images (k-th approximate score of the
    // first ns columns), lowered by eps into a bound of the exact k-th
    const int64_t ns = kSeedMaxNs;
    const int seed_env = getenv("PMM_BF16_SEED") ? atoi(getenv("PMM_BF16_SEED")) : 1;  // (per call)
    const bool seeded = seed_env && 4 * k <= ns && n >= 8 * ns && (size_t)m * ns * 4 <= p.off_qn - p.off_cand;
    Timed t("seed_bf16/screen", s);
    if (seeded) {
      float *sample = (float *)a.cand;
      HIP_TRY(launch_seed_bf16_ws(a, sample, (int)ns, s));
      HIP_TRY(launch_seed_select(sample, ns, (int)m, (int)ns, (int)k, metric, a.gthr, s));
    }
    HIP_TRY(launch_screen_prep(rel, scal, (int)m, (int)sp.dpb, eps, a.gthr, seeded ? 1 : 0, s));
    // A guessed bound near each row's final k-th, extrapolated from the same
    // sample (screen_guess_kernel): the target rank is t k of n, t the slack
    // (PMM_SCREEN_GUESS_T, default kScreenGuessSlack).  PMM_SCREEN_GUESS=0:
    // no guess, the rows start from the seed's proven bound alone.
    const int guess_env = getenv("PMM_SCREEN_GUESS") ? atoi(getenv("PMM_SCREEN_GUESS")) : 1;  // (per call)
    double slack = kScreenGuessSlack;
    if (const char *te = getenv("PMM_SCREEN_GUESS_T")) slack = atof(te);
    const double tail = slack * (double)k / (double)n;
    if (seeded && guess_env && slack >= 1.0 && tail < (double)k / (double)ns) {
      // (in the rows' residuals' place: screen_prep was their last reader)
      uint32_t *guess = (uint32_t *)rel;
      HIP_TRY(launch_screen_guess((const float *)a.cand, (int)m, (int)ns, (float)normal_upper_quantile(tail), eps,
                                  guess, s));
      a.guess = guess;
    }
  }
#ifdef PMM_SCREEN_CEILING
  // Experiment build only (make ab AB=-DPMM_SCREEN_CEILING; tools/experiments/
  // screen_ceiling.py): start every row from the bound an earlier call on the
  // same inputs ended with -- a proven bound, so the results do not change --
  // which is the best start any guessed threshold could give the screen kernel.
  if (const char *f = getenv("PMM_SCREEN_GTHR_LOAD")) {
    std::vector<uint64_t> hb((size_t)m);
    FILE *fp = fopen(f, "rb");
    const bool ok = fp && fread(hb.data(), 8, (size_t)m, fp) == (size_t)m;
    if (fp) fclose(fp);
    if (!ok) return fail(PMM_ERR_ARG, "PMM_SCREEN_GTHR_LOAD: cannot read %lld bounds from %s", (long long)m, f);
    HIP_TRY(hipMemcpyAsync(a.gthr, hb.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
#endif
  {
    Timed t("gemm_f32_topk/screen", s);
    HIP_TRY(launch_gemm_bf16_ws(a, p.grid, s, true));
  }
#ifdef PMM_SCREEN_CEILING
  if (const char *f = getenv("PMM_SCREEN_GTHR_SAVE")) {
    std::vector<uint64_t> hb((size_t)m);
    HIP_TRY(hipMemcpyAsync(hb.data(), a.gthr, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    FILE *fp = fopen(f, "wb");
    const bool ok = fp && fwrite(hb.data(), 8, (size_t)m, fp) == (size_t)m;
    if (fp) fclose(fp);
    if (!ok) return fail(PMM_ERR_ARG, "PMM_SCREEN_GTHR_SAVE: cannot write %s", f);
  }
#endif
  {
    Timed t("merge_topk/rescore", s);
    ScreenFinishArgs fa{};
    fa.q = q;
    fa.c = c;
    fa.ldq = ldq;
    fa.ldc = ldc;
    fa.qn = qn;
    fa.cn = cn;
    fa.eps = eps;
    fa.M = (int)m;
    fa.N = (int)n;
    fa.dp = (int)sp.dp;
    fa.S = p.S;
    fa.capg = p.capg;
    fa.k = (int)k;
    fa.cand = a.cand;
    fa.cnt = a.cnt;
    fa.gthr = a.gthr;
    fa.stat = debug ? scal + 4 : nullptr;
    fa.guess = a.guess;
    fa.ovf = ovf;
    HIP_TRY(launch_screen_rescore(fa, s));
  }
  {
    Timed t("merge_topk", s);
    HIP_TRY(launch_merge(merge_cand_args(a, p, index_base, out_idx, out_score), 0, s));
  }
  HIP_TRY(launch_zero_sign_f32(q, ldq, c, ldc, qn, cn, (int)m, n, (int)d, (int)k, metric, index_base, out_idx,
                               out_score, s));
  // Rows the screen could not finish (unsafe, or a band that outgrew its
  // segment) and an unsafe corpus: one read-back, then the f32 kernel.
  HIP_TRY(launch_screen_collect(ovf, bad, (int)m, scal + 2, rows, s));
  unsigned h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, scal, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // Many rows to re-run (a crowded corpus: clustered embeddings can fill the
  // 2 eps band of most rows): one f32 launch over the whole call is cheaper
  // than serial launches of kScreenRerunRows rows, each of which streams the
  // corpus for a few query blocks.
  const bool whole = h[1] != 0 || (int64_t)h[2] * 8 > m + 8 * kScreenRerunRows;
  if (debug) {
    float rc;
    memcpy(&rc, &h[0], 4);
    fprintf(stderr,
            "[pmm screen] S=%d tps=%d qb_full=%d capg=%d ctrig=%d corpus_residual=%.6g corpus_unsafe=%u "
            "rerun_rows=%u overflowed=%u whole_call_f32=%d rescored=%u max_per_row=%u kept=%u m=%lld handle=%d "
            "guess=%d guess_missed=%u\n",
            p.S, p.tps, p.qb_full, p.capg, p.ctrig, rc, h[1], h[2], h[3], whole ? 1 : 0, h[4], h[5], h[6],
            (long long)m, img ? 1 : 0, a.guess ? 1 : 0, h[7]);
  }
  // The f32 kernel's runs never screen (k <= kScreenMaxK: always its fused
  // route); plan_screen reserved their workspace at off_f32.
  if (whole) {
    const TopkRoute f = route_topk(m, n, d, k, metric, PMM_COMPUTE_F32, cus, false, false);
    return topk_f32_fused(f.p, q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score, w + sp.off_f32,
                          s, cus, c_norms, false);
  }
  for (int64_t r0 = 0; r0 < (int64_t)h[2]; r0 += sp.rr) {
    const int64_t nr = std::min<int64_t>(sp.rr, (int64_t)h[2] - r0);
    // (a smaller launch may plan more corpus splits: outside the reserved
    // bytes rerun_rows takes a buffer of its own)
    const TopkRoute f = route_topk(nr, n, d, k, metric, PMM_COMPUTE_F32, cus, false, false);
    const int rc = rerun_rows(q, ldq * 4, sp.dp * 4, rows + r0, nr, k, f.total, w + sp.off_gq, sp.total - sp.off_gq,
                              out_idx, out_score, s, "screen re-run",
                              [&](const char *gq, uint32_t *gi, float *gs, char *fw) {
                                return topk_f32_fused(f.p, (const float *)gq, sp.dp, nr, c, ldc, n, d, k, metric,
                                                      index_base, gi, gs, fw, s, cus, c_norms, false);
                              });
    if (rc) return rc;
  }
  return PMM_OK;
}

// The f32 kernel's search of a route that does not screen (fused,
// materialised, or the widened bf16 path's inner search) over workspace w.
int topk_f32_unscreened(const TopkRoute &r, const float *q, int64_t ldq, int64_t m, const float *c, int64_t ldc,
                        int64_t n, int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *out_idx,
                        float *out_score, char *w, hipStream_t s, int cus, const float *c_norms, bool keep_gthr,
                        const float *c_pre = nullptr) {
  return r.fused ? topk_f32_fused(r.p, q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score, w, s, cus,
                                  c_norms, keep_gthr, c_pre)
                 : topk_f32_materialised(r.mp, q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score, w,
                                         s, cus, c_norms);
}

// Executes an f32 route (route_topk's, for this m, n, d, k, metric) in the
// caller's workspace, or the arena when ws is NULL.
int topk_f32_device_impl(const TopkRoute &route, const float *q, int64_t ldq, int64_t m, const float *c, int64_t ldc,
                         int64_t n, int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *out_idx,
                         float *out_score, void *ws, size_t ws_bytes, hipStream_t s, int dev,
                         const float *c_norms = nullptr, bool keep_gthr = false,
                         const ScreenImage *img = nullptr, const float *c_pre = nullptr) {
  const int cus = g_dev[dev].cus;
  const int64_t dp = padded_dim(PMM_DTYPE_F32, d);
  // What the screen asks of a call and route_topk cannot see (row strides and
  // alignment of the rows it rounds, norms it computes itself or reads beside
  // a handle's image, thresholds it starts from zero): without it the call
  // takes the unscreened route, whose workspace the screened one contains
  // (plan_screen reserves it).
  TopkRoute plain;
  const TopkRoute *r = &route;
  if (route.kind == Route::kF32Screened &&
      ((c_norms != nullptr) != (img != nullptr) || route.sp.ext != (img != nullptr) || keep_gthr || ldq % 4 != 0 ||
       ldc % 4 != 0 || ldq < dp || ldc < dp || (((uintptr_t)q | (uintptr_t)c) & 15))) {
    plain = route_topk(m, n, d, k, metric, PMM_COMPUTE_F32, cus, false, false);
    r = &plain;
  }
  Workspace W;
  if (int rc = acquire_workspace(ws, ws_bytes, r->total, dev, s, W)) return rc;
  const int rc = r->kind == Route::kF32Screened
                     ? topk_f32_screened(*r, q, ldq, m, c, ldc, n, d, k, index_base, out_idx, out_score, W.w, s, cus,
                                         img, c_norms)
                     : topk_f32_unscreened(*r, q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score,
                                           W.w, s, cus, c_norms, keep_gthr, c_pre);
  return rc ? rc : W.done();
}

// bf16 compute path over device bf16 rows (row strides ldq / ldc >=
// roundup(d, 128), zero-padded); d is the logical dimension.
//
// The bf16 MFMA kernels hold a wave's 32 query rows x padded D in registers
// (D <= 768), their candidate buffers take k <= 960 and pack the column into
// 27 bits.  Outside that (configs[4]'s D = 1024, larger k, n >= 2^27) the
// bf16 operands are widened to f32 -- exactly: a bf16 value is an f32 with
// its low 16 bits zero -- and searched by the f32 path.  The result is the
// exact top-k of the bf16-rounded rows with f32 products and a k-ordered f32
// sum (the f32 path's bit-exact chain), so it meets the bf16 bar; the f32
// MFMA runs at 1/16 of the bf16 rate, which the bench line of such a shape
// states.
//
// The native route's executor (the bf16 kernel of p.variant + merge) over its
// acquired workspace w (p.total bytes).
int topk_bf16_native(const Plan &p, const uint16_t *q, int64_t ldq, int64_t m, const uint16_t *c, int64_t ldc,
                     int64_t n, int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *out_idx,
                     float *out_score, char *w, hipStream_t s, const float *q_norms = nullptr,
                     const float *c_norms = nullptr) {
  const int64_t dp = padded_dim(PMM_DTYPE_BF16, d);
  // the precomputed arrays live outside w (a bf16 corpus handle's, and the
  // query norms its call's rounding pass wrote): the memset below cannot
  // reach them, and the workspace's own norm slots stay unused
  const float *qn = q_norms ? q_norms : (const float *)(w + p.off_qn);
  const float *cn = c_norms ? c_norms : (const float *)(w + p.off_cn);
  HIP_TRY(hipMemsetAsync(w, 0, p.off_gthr + (size_t)m * 8, s));
  if (p.qb_full) HIP_TRY(hipMemsetAsync(w + p.off_cnt, 0, (size_t)m * p.S * 4, s));
  if (metric != kMetricDot && (!q_norms || !c_norms)) {
    const int sq = metric == kMetricEuclidean;
    Timed t("norms_bf16", s);
    if (!q_norms) HIP_TRY(launch_norms_bf16(q, m, d, ldq, sq, (float *)(w + p.off_qn), nullptr, s));
    if (!c_norms)
      HIP_TRY(launch_norms_bf16(c, n, d, ldc, sq, (float *)(w + p.off_cn), (float *)(w + p.off_cn) + n, s));
  }
  GemmF32Args a = fused_args(m, n, dp, k, metric, p, w);
  a.qb = q;
  a.cb = c;
  a.qn = qn;
  a.cn = cn;
  a.cpre = cn + n;
  a.ldq = ldq;
  a.ldc = ldc;
  set_bf16_knobs(a);
#ifdef PMM_LAB
  {
    static const int ablate = getenv("PMM_ABLATE") ? atoi(getenv("PMM_ABLATE")) : 0;
    a.ablate = ablate;
  }
#endif
  {
#ifdef PMM_LAB
    static const bool stats = getenv("PMM_STATS") != nullptr;
#else
    constexpr bool stats = false;  // (per-phase cycle counters: lab build only)
#endif
    static unsigned long long *stats_buf = nullptr;
    if (stats) {
      if (!stats_buf) HIP_TRY(hipMalloc(&stats_buf, 128));
      HIP_TRY(hipMemsetAsync(stats_buf, 0, 128, s));
      a.stats = stats_buf;
    }
    {
      // Threshold seed (wave-specialised kernel): unseeded, every row starts
      // at "accept all" and its threshold only rises at compactions (every
      // ~220 appends), so a row queues and re-scores ~2k survivors over a 1M
      // corpus.  The k-th best of the first ns columns -- scored bit for bit
      // as the main pass scores them -- minus 1 is an exact lower bound of
      // the row's final k-th best: the main pass starts from it.
      const int seed_env = getenv("PMM_BF16_SEED") ? atoi(getenv("PMM_BF16_SEED")) : 1;  // (read per call: tests toggle it)
      int64_t ns = kSeedMaxNs;
      if (const char *ne = getenv("PMM_SEED_NS")) ns = std::max<int64_t>(32, std::min<int64_t>(atoll(ne), kBf16SeedMaxNs) / 32 * 32);
      if (seed_env && p.variant == -2 && 4 * k <= ns && n >= 8 * ns && seed_span_fits(ns, ldc, 2) &&
          (size_t)m * ns * 4 <= p.off_qn - p.off_cand) {
        float *sample = (float *)a.cand;
        Timed t("seed_bf16", s);
        HIP_TRY(launch_seed_bf16_ws(a, sample, (int)ns, s));
        HIP_TRY(launch_seed_select(sample, ns, (int)m, (int)ns, (int)k, metric, a.gthr, s));
      }
    }
    if (p.variant == -6) {
#ifdef PMM_WITH_FF
      // fire-and-forget 256-row kernel: the guessed threshold (the j-th best
      // of an exact ns-row sample, minus 1), the pass, the exact re-score and
      // bucketing into the candidate lists; rows it cannot prove exact are
      // re-run below
      float *sample = (float *)a.cand;
      // (its guessed threshold needs the sample: no unseeded form)
      if (!seed_span_fits(p.ff_ns, ldc, 2))
        return fail(PMM_ERR_ARG, "ldc=%lld: the fire-and-forget kernel's %d-row sample does not fit one descriptor",
                    (long long)ldc, p.ff_ns);
      {
        Timed t("seed_bf16", s);
        HIP_TRY(launch_seed_bf16_ws(a, sample, p.ff_ns, s));
        HIP_TRY(launch_seed_select(sample, p.ff_ns, (int)m, p.ff_ns, p.ff_j, metric, a.gthr, s));
      }
      a.qb_full = 0;
      a.ffreg = (unsigned long long *)(w + p.off_ffreg);
      a.ffcnt = (unsigned *)(w + p.off_ffcnt);
      a.ffcap = p.ffcap;
      {
        Timed t("gemm_bf16_topk/ff", s);
        HIP_TRY(launch_gemm_bf16_ff(a, p.grid, s));
      }
      HIP_TRY(hipMemsetAsync(w + p.off_fb, 0, 16, s));
      {
        Timed t("ff_bucket", s);
        HIP_TRY(launch_ff_bucket(a, (unsigned *)(w + p.off_fb), (int *)(w + p.off_fb + 16), s));
      }
#endif
    } else {
      // (the suffix names the kernel; pmm_timing_read matches substrings)
      Timed t(p.variant == -2 ? "gemm_bf16_topk/ws" : "gemm_bf16_topk/one-wave", s);
      HIP_TRY(p.variant == -2 ? launch_gemm_bf16_ws(a, p.grid, s) : launch_gemm_bf16(a, p.grid, s));
    }
    if (stats) {
      unsigned long long h[16];
      HIP_TRY(hipMemcpyAsync(h, stats_buf, 128, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (p.variant == -2)
        fprintf(stderr,
                "[pmm stats] gemm_bf16_ws: units %d, S %d, tps %d, sync timeouts %llu, survivors "
                "%llu; MFMA-wave cycles %.3g; epilogue-wave cycles: DMA issue %.3g, epilogue "
                "%.3g, vmcnt waits %.3g, barriers %.3g of %.3g; compactions %.3g (%llu rows), "
                "survivor queueing %.3g, drains %.3g\n",
                p.units, p.S, p.tps, h[2], h[0], (double)h[1], (double)h[3], (double)h[4],
                (double)h[5], (double)h[6], (double)h[7], (double)h[8], h[9], (double)h[10],
                (double)h[11]);
      else
      fprintf(stderr,
              "[pmm stats] gemm_bf16: queued %llu, LDS-queue tiles %llu, sync timeouts %llu, "
              "compactions %llu, units %d, S %d, tps %d; wave cycles: K-loop %.3g, extract %.3g, "
              "pass 2 %.3g\n",
              h[0], h[1], h[2], h[3], p.units, p.S, p.tps, (double)h[4], (double)h[5], (double)h[6]);
    }
  }
  Timed t("merge_topk", s);
  HIP_TRY(launch_merge(merge_cand_args(a, p, index_base, out_idx, out_score), 0, s));
  return PMM_OK;
}

#ifdef PMM_WITH_FF
// The fire-and-forget kernel's rows that it could not prove exact (fewer than
// k candidates at or above the guessed threshold, or a dropped survivor):
// their query rows are gathered and re-run on the wave-specialised kernel
// against the whole corpus, and their lists replace the merge's.  Reads the
// row count back (a stream synchronisation) and allocates the re-run's
// buffers itself (rerun_rows without a buffer: hipMalloc, outside the caller's
// workspace): test-library behaviour only (libpmm_ff.so), never in libpmm.so.
// Rare: the guess leaves about n j / ns scores per row against the k needed.
int ff_rerun(const uint16_t *q, int64_t ldq, int64_t m, const uint16_t *c, int64_t ldc, int64_t n, int64_t d,
             int64_t k, int metric, uint32_t index_base, uint32_t *out_idx, float *out_score, const unsigned *fb,
             hipStream_t s, int cus) {
  unsigned nfb = 0;
  HIP_TRY(hipMemcpyAsync(&nfb, fb, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (getenv("PMM_FF_DEBUG")) fprintf(stderr, "[pmm ff] re-run rows %u of %lld\n", nfb, (long long)m);
  if (nfb == 0) return PMM_OK;
  // the row list stays on the device (gather and scatter kernels read it);
  // whole rows of ldq elements are gathered, so the block keeps the stride
  const int64_t nr = nfb;
  const TopkRoute f = route_topk(nr, n, d, k, metric, PMM_COMPUTE_BF16, cus, false, false);
  return rerun_rows(q, ldq * 2, ldq * 2, (const int *)(fb + 4), nr, k, f.total, nullptr, 0, out_idx, out_score, s,
                    "ff re-run", [&](const char *gq, uint32_t *gi, float *gs, char *fw) {
                      return topk_bf16_native(f.p, (const uint16_t *)gq, ldq, nr, c, ldc, n, d, k, metric, index_base,
                                              gi, gs, fw, s);
                    });
}
#endif  // PMM_WITH_FF

// Executes a bf16 route (route_topk's, for this m, n, d, k, metric) in the
// caller's workspace, or the arena when ws is NULL.
int topk_bf16_device_impl(const TopkRoute &r, const uint16_t *q, int64_t ldq, int64_t m, const uint16_t *c,
                          int64_t ldc, int64_t n, int64_t d, int64_t k, int metric, uint32_t index_base,
                          uint32_t *out_idx, float *out_score, void *ws, size_t ws_bytes, hipStream_t s, int dev,
                          const float *q_norms = nullptr, const float *c_norms = nullptr) {
  // q_norms / c_norms: optional precomputed norms of this metric (q: m norms;
  // c: [n norms | n pre-filter factors], a bf16 corpus handle's), outside the
  // workspace; the native route then launches no norms kernel for them.  The
  // widened route computes its own from the widened rows (the same values).
  const int cus = g_dev[dev].cus;
  Workspace W;
  if (int rc = acquire_workspace(ws, ws_bytes, r.total, dev, s, W)) return rc;
  char *w = W.w;
  int rc;
  if (r.kind == Route::kBf16Widened) {
    // widened to f32 and searched by the f32 path, which never screens here
    float *wq = (float *)w, *wc = (float *)(w + r.off_wc);
    {
      Timed t("bf16_widen", s);
      HIP_TRY(launch_bf16_to_f32(q, m, d, ldq, wq, r.dpw, s));
      HIP_TRY(launch_bf16_to_f32(c, n, d, ldc, wc, r.dpw, s));
    }
    rc = topk_f32_unscreened(r, wq, r.dpw, m, wc, r.dpw, n, d, k, metric, index_base, out_idx, out_score, w + r.base,
                             s, cus, nullptr, false);
  } else {
    rc = topk_bf16_native(r.p, q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score, w, s,
                          metric == kMetricDot ? nullptr : q_norms, metric == kMetricDot ? nullptr : c_norms);
#ifdef PMM_WITH_FF
    if (rc == PMM_OK && r.p.variant == -6)
      rc = ff_rerun(q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score,
                    (const unsigned *)(w + r.p.off_fb), s, cus);
#endif
  }
  return rc ? rc : W.done();
}

// Upload a host matrix rows x d into a device buffer with row stride dp,
// zero-padding columns d..dp-1.
int upload_padded(void *dst, const void *src, int64_t rows, int64_t d, int64_t dp, size_t elem,
                  hipStream_t s) {
  if (rows <= 0) return PMM_OK;
  Timed t("h2d", s);  // bench.py's end-to-end breakdown (pmm_timing_*)
  if (dp == d) {
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)rows * d * elem, hipMemcpyHostToDevice, s));
  } else {
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)rows * dp * elem, s));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)dp * elem, src, (size_t)d * elem, (size_t)d * elem,
                             (size_t)rows, hipMemcpyHostToDevice, s));
  }
  return PMM_OK;
}

// The end of a host top-k call: both m x k result lists (f32 or f64 scores)
// to the host, and the call's one synchronisation.
template <typename Score>
int download_lists(uint32_t *out_idx, Score *out_score, const void *idx, const void *score, int64_t m, int64_t k,
                   hipStream_t s) {
  {
    Timed t("d2h", s);
    HIP_TRY(hipMemcpyAsync(out_idx, idx, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_score, score, (size_t)m * k * sizeof(Score), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return PMM_OK;
}

int validate_sizes(int64_t m, int64_t n, int64_t d, int64_t k, bool topk, bool allow_k_gt_n = false) {
  if (m < 0 || n < 0 || d < 0) return fail(PMM_ERR_ARG, "negative size (m=%lld n=%lld d=%lld)",
                                           (long long)m, (long long)n, (long long)d);
  if (m > INT32_MAX || n > (int64_t)UINT32_MAX - 1 || n > INT32_MAX)
    return fail(PMM_ERR_ARG, "size out of range (m=%lld n=%lld)", (long long)m, (long long)n);
  if (topk) {
    if (k < 0) return fail(PMM_ERR_ARG, "k must be >= 0 (got %lld)", (long long)k);
    if (k > n && !allow_k_gt_n)
      return fail(PMM_ERR_ARG, "k (%lld) must be <= n (%lld): clip k to n first", (long long)k,
                  (long long)n);
  }
  return PMM_OK;
}

// A non-empty call needs every buffer it names (the reference never passes
// null; a binding that does gets an error instead of a fault).
template <typename... P>
int need_buffers(P... p) {
  return ((p != nullptr) && ...) ? PMM_OK : fail(PMM_ERR_ARG, "null argument");
}

// Host-buffer f32 top-k over a large corpus with the upload overlapped with
// compute.  The corpus is cut into chunks: a small first one (uploaded, with
// the queries, before any compute) and CHUNKS-1 equal ones.  Chunk i + 1 is
// copied on the thread's copy stream while chunk i's fused top-k runs on the
// compute stream; each chunk's list carries global indices (index_base) into
// a [chunks][2][m][k] buffer (index plane, score plane), merged in place at
// the end -- the sharded path's merge, on one device.  The shared per-row
// thresholds carry from chunk to chunk (keep_gthr): a chunk's k-th composite
// is a lower bound of the global k-th, so later chunks start pruned and the
// result equals the one-launch result bit for bit.
constexpr size_t kChunkedMinBytes = size_t(256) << 20;  // corpus bytes from which uploads overlap
constexpr int kChunks = 4;

int topk_f32_host_chunked(const float *q, int64_t m, const float *c, int64_t n, int64_t d, int64_t k,
                          int metric, uint32_t *out_idx, float *out_score) {
  int dev, rc;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, list_root()))) return rc;
  hipStream_t s, cs;
  if ((rc = thread_stream(dev, &s)) || (rc = thread_stream(dev, &cs, true))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_F32, d);
  int64_t bnd[kChunks + 1];
  bnd[0] = 0;
  bnd[1] = std::max<int64_t>(k, n / 16);
  for (int i = 2; i <= kChunks; i++) bnd[i] = bnd[1] + (n - bnd[1]) * (i - 1) / (kChunks - 1);
  // (chunks carry thresholds over: unscreened)
  TopkRoute route[kChunks];
  size_t ws_need = 0;
  for (int i = 0; i < kChunks; i++) {
    route[i] = route_topk(m, bnd[i + 1] - bnd[i], d, k, metric, PMM_COMPUTE_F32, g_dev[dev].cus, false, false);
    ws_need = std::max(ws_need, route[i].total);
  }
  Layout L;
  const size_t off_q = L.take((size_t)m * dp * 4), off_c = L.take((size_t)n * dp * 4);
  const size_t off_l = L.take((size_t)kChunks * 2 * m * k * 4);
  const size_t off_i = L.take((size_t)m * k * 4), off_s = L.take((size_t)m * k * 4), off_w = L.off;
  void *base;
  if ((rc = arena(dev, s, off_w + ws_need, &base))) return rc;
  char *b = (char *)base;
  uint32_t *li = (uint32_t *)(b + off_l);
  hipEvent_t ev[kChunks + 1] = {};
  // One exit for every failure after the copy stream may have work queued:
  // the copy stream writes into the arena, so it is drained before the arena
  // can be reused or grown (freed) by a later call, and the events are freed.
  auto finish = [&](int code) {
    if (code != PMM_OK) {
      (void)hipStreamSynchronize(cs);
      (void)hipStreamSynchronize(s);
    }
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
    return code;
  };
#define CHUNK_TRY(expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return finish(fail(PMM_ERR_HIP, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), \
                         __FILE__, __LINE__, #expr));                                     \
  } while (0)
  for (auto &e : ev) CHUNK_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // the copy stream must not overwrite the arena before earlier compute on
  // the compute stream is done with it
  hipEvent_t ready = ev[kChunks];
  CHUNK_TRY(hipEventRecord(ready, s));
  CHUNK_TRY(hipStreamWaitEvent(cs, ready, 0));
  if ((rc = upload_padded(b + off_q, q, m, d, dp, 4, cs))) return finish(rc);
  for (int i = 0; i < kChunks; i++) {
    const int64_t lo = bnd[i], rows = bnd[i + 1] - bnd[i];
    // a pageable copy returns once staged: chunk i + 1 is copied while the
    // device computes chunk i
    if ((rc = upload_padded(b + off_c + (size_t)lo * dp * 4, c + lo * d, rows, d, dp, 4, cs))) return finish(rc);
    CHUNK_TRY(hipEventRecord(ev[i], cs));
    CHUNK_TRY(hipStreamWaitEvent(s, ev[i], 0));
    rc = topk_f32_device_impl(route[i], (const float *)(b + off_q), dp, m, (const float *)(b + off_c) + lo * dp, dp,
                              rows, d, k, metric, (uint32_t)lo, li + (size_t)i * 2 * m * k,
                              (float *)(li + (size_t)i * 2 * m * k + (size_t)m * k), b + off_w, ws_need, s,
                              dev, nullptr, i > 0);
    if (rc) return finish(rc);
  }
  // (each chunk's lists are a top-k output: best first)
  const MergeArgs ma = merge_lists_args(li, (const float *)(li + (size_t)m * k), m, kChunks, k, k, 2 * m * k, k, metric,
                                        true, (uint32_t *)(b + off_i), (float *)(b + off_s));
  {
    Timed t("merge_chunks", s);
    CHUNK_TRY(launch_merge(ma, 1, s));
    // (the chunks' zero scores carry their signs; the merge's keys fold them)
    if (metric != kMetricEuclidean)
      CHUNK_TRY(launch_zero_sign_lists(ma.in_idx, ma.in_score, kChunks, (int)k, k, 2 * m * k, (int)m, (int)k,
                                       ma.out_idx, ma.out_score, s));
  }
  {
    Timed t("d2h", s);
    CHUNK_TRY(hipMemcpyAsync(out_idx, b + off_i, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
    CHUNK_TRY(hipMemcpyAsync(out_score, b + off_s, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
  }
  CHUNK_TRY(hipStreamSynchronize(s));
#undef CHUNK_TRY
  return finish(PMM_OK);
}

// ---------------------------------------------------------------------------
// f64 top-k (src/matmul.rs:449-468 -> src/metrics.rs:258-311 + src/topk.rs:6-39)
// on device rows of stride >= roundup(d, 16), zero-padded.  k <= kFusedMaxK:
// the fused chunked scan of pmm_f64.hip (no M x N matrix); a row whose buffer
// overflowed (adversarial data: every chunk beats the last) or k above the
// fused limit: the materialised path (f64 GEMM store + row select), which also
// serves as the PMM_F64_FUSED=0 reference.
// ---------------------------------------------------------------------------
// The schedule of a chunked scan (the f64 scan here, the int8 scan of
// topk_i8_device_impl), stated once.  A row keeps a candidate buffer of `cap`
// entries; a pass takes the `mc` query rows whose buffers fit the budget; the
// first chunk of `s0` columns fills half a buffer (accept-all), later chunks
// are g times the columns seen.  After `seen` columns the threshold is the
// k-th best of them, so a chunk of g * seen columns from the same distribution
// leaves ~g * X survivors in a row, X ~ Gamma(k) (the k-th order statistic's
// quantile times seen).  Its spread is k^-1/2 of its mean whatever `seen` is,
// so g is sized for the tail, not the mean: with
// P(X > k + t) <= exp(-t^2 / (2 (k + t))) and t = 23 + sqrt(529 + 46 k)
// (a per-row, per-chunk tail of e^-23 ~ 1e-10), g (k + t) <= cap - k keeps
// every row inside its buffer.  (g = (cap/2 - k) / k, sized for the mean,
// overflowed some row of nearly every call at 4096 x 1M: the whole call
// then re-ran materialised, 257 vs 209 ms; profiles/r4_f64/.)  Adversarial
// orders still overflow; each scan has its own fallback for them.
constexpr size_t kF64CandBudget = size_t(1) << 30;
struct ChunkSchedule {
  int cap = 0;
  int64_t mc = 0, s0 = 0, g = 1;
};
int chunk_cap(int64_t k) {
  return std::min(4096, std::max(1024, next_pow2(4 * (int)std::min<int64_t>(k, kFusedMaxK) + 256)));
}
// cap: chunk_cap(k), or a smaller buffer a test asks for (PMM_I8_CAP)
ChunkSchedule chunk_schedule(int64_t m, int64_t n, int64_t k, int cap) {
  ChunkSchedule c;
  c.cap = cap;
  c.mc = std::max<int64_t>(1, std::min<int64_t>(m, (int64_t)(kF64CandBudget / ((size_t)cap * 16))));
  c.s0 = std::min<int64_t>(n, cap / 2);
  const double tail = 23.0 + std::sqrt(529.0 + 46.0 * (double)k);
  c.g = std::max<int64_t>(1, (int64_t)((double)(cap - k) / ((double)k + tail)));
  return c;
}

struct F64Plan {
  ChunkSchedule sched;
  size_t off_qn = 0, off_cn = 0, off_tkey = 0, off_tidx = 0, off_cnt = 0, off_cand = 0, off_flag = 0,
         off_mat = 0, total = 0;
};

void plan_f64(int64_t m, int64_t n, int64_t k, F64Plan &p) {
  p.sched = chunk_schedule(m, n, k, chunk_cap(k));
  const int64_t mc = p.sched.mc;
  size_t off = 0;
  p.off_flag = off;
  off += 256;
  p.off_qn = off;
  off = al256(off + (size_t)m * 8);
  p.off_cn = off;
  off = al256(off + (size_t)n * 8);
  p.off_tkey = off;
  off = al256(off + (size_t)mc * 8);
  p.off_tidx = off;
  off = al256(off + (size_t)mc * 4);
  p.off_cnt = off;
  off = al256(off + (size_t)mc * 4);
  p.off_cand = off;
  off = al256(off + (size_t)mc * p.sched.cap * 16);
  p.total = off;
}


// Fused scan or materialised scores, by the size of the M x N f64 score
// matrix the materialised path writes and re-reads (device API, cosine,
// k = 10, D = 256; profiles/r4_f64/f64_sizes.jsonl): 1000 x 10000 (80 MB)
// materialised 0.239 ms vs fused 0.348 (its chunk launches, selects and
// overflow check); 1000 x 100000 (0.8 GB) 2.02 vs 1.40; 4096 x 1M (33 GB)
// 209 vs 47.6.  The threshold sits between the first two.  PMM_F64_FUSED=1
// / 0 forces either (read per call: tests compare both paths).
constexpr double kF64FusedMinMatrixBytes = 256.0 * 1024.0 * 1024.0;
bool f64_fused_enabled(int64_t m, int64_t n) {
  const char *e = getenv("PMM_F64_FUSED");
  if (e && *e) return atoi(e) != 0;
  return (double)m * (double)n * 8.0 > kF64FusedMinMatrixBytes;
}

// Which path a call takes, decided once per call (the workspace is sized for
// it and the device code follows it, whatever PMM_F64_FUSED says meanwhile).
bool f64_use_fused(int64_t m, int64_t n, int64_t k) { return k <= kFusedMaxK && f64_fused_enabled(m, n); }

// Workspace of one f64 top-k call: the materialised path's alone when the call
// takes it; the fused scan's and the materialised path's (its overflow
// fallback reuses the workspace) otherwise.  (Sizing every call for both held
// up to 1 GiB of candidate buffers next to a small score matrix.)
size_t f64_workspace_bytes(int64_t m, int64_t n, int64_t k, bool fused) {
  MatPlan mp;
  plan_materialise(m, n, k, 8, mp);
  if (!fused) return mp.total;
  F64Plan p;
  plan_f64(m, n, k, p);
  return std::max(p.total, mp.total);
}

// cn_pre: the corpus rows' norms of this metric already on the device (a
// corpus handle's, computed at creation by the same kernel), else nullptr.
int topk_f64_materialised(const double *dq, int64_t ldq, int64_t m, const double *dc, int64_t ldc, int64_t n,
                          int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *oi, double *os,
                          char *w, hipStream_t s, const double *cn_pre = nullptr) {
  // (planned again here, after f64_workspace_bytes sized w: the same rule on
  // the same sizes, and the budget the same thread read a moment before in the
  // same entry call -- the environment does not change under a running call)
  MatPlan p;
  plan_materialise(m, n, k, 8, p);
  double *qn = (double *)(w + p.off_qn), *cn = (double *)(w + p.off_cn);
  double *sc = (double *)(w + p.off_scores);
  if (metric != kMetricDot) {
    const int sq = metric == kMetricEuclidean;
    HIP_TRY(launch_norms_f64(dq, m, d, ldq, sq, qn, s));
    if (cn_pre) cn = (double *)cn_pre;
    else HIP_TRY(launch_norms_f64(dc, n, d, ldc, sq, cn, s));
  }
  const int64_t dp = padded_dim(PMM_DTYPE_F64, d);
  for (int64_t r0 = 0; r0 < m; r0 += p.rows) {
    const int64_t rows = std::min<int64_t>(p.rows, m - r0);
    {
      Timed t("gemm_f64_scores", s);
      HIP_TRY(launch_gemm_f64_store(dq + r0 * ldq, ldq, dc, ldc, qn + r0, cn, (int)rows, (int)n, (int)dp, metric,
                                    1, sc, n, s));
    }
    if (!p.global_sort) {
      RowSelArgs ra{};
      ra.scores = sc;
      ra.lds = n;
      ra.rows = (int)rows;
      ra.N = (int)n;
      ra.k = (int)k;
      ra.P = p.P;
      ra.metric = metric;
      ra.is_f64 = 1;
      ra.index_base = index_base;
      ra.out_idx = oi + r0 * k;
      ra.out_score = os + r0 * k;
      Timed t("select_f64_rows", s);
      HIP_TRY(launch_rowselect(ra, s));
    } else {
      HIP_TRY(launch_rowsort_global(sc, n, (int)rows, (int)n, 1, metric, w + p.off_keys, p.P2, (int)k, index_base,
                                    oi + r0 * k, os + r0 * k, s));
    }
  }
  // the sign of zero scores (the f32 lists' pass, in f64)
  HIP_TRY(launch_zero_sign_f64(dq, ldq, dc, ldc, qn, cn, (int)m, n, (int)d, (int)k, metric, index_base, oi, os, s));
  return PMM_OK;
}

// flag_copy (the sharded path): instead of waiting here for the fused scan's
// overflow flag, enqueue a copy of it to flag_copy (device memory) and return;
// the caller checks it once every device has finished and re-runs an
// overflowed shard with topk_f64_materialised.
int topk_f64_device_impl(const double *dq, int64_t ldq, int64_t m, const double *dc, int64_t ldc, int64_t n,
                         int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *oi, double *os, char *w,
                         hipStream_t s, bool fused, const double *cn_pre = nullptr, unsigned *flag_copy = nullptr) {
  if (!fused)
    return topk_f64_materialised(dq, ldq, m, dc, ldc, n, d, k, metric, index_base, oi, os, w, s, cn_pre);
  F64Plan p;
  plan_f64(m, n, k, p);
  const int64_t dp = padded_dim(PMM_DTYPE_F64, d);
  double *qn = (double *)(w + p.off_qn), *cn = (double *)(w + p.off_cn);
  unsigned *flag = (unsigned *)(w + p.off_flag);
  if (metric != kMetricDot) {
    const int sq = metric == kMetricEuclidean;
    Timed t("norms_f64", s);
    HIP_TRY(launch_norms_f64(dq, m, d, ldq, sq, qn, s));
    if (cn_pre) cn = (double *)cn_pre;
    else HIP_TRY(launch_norms_f64(dc, n, d, ldc, sq, cn, s));
  }
  const ChunkSchedule &sched = p.sched;  // (chunk_schedule; an overflowed call falls back below)
  HIP_TRY(hipMemsetAsync(flag, 0, 4, s));
  for (int64_t r0 = 0; r0 < m; r0 += sched.mc) {
    const int rows = (int)std::min<int64_t>(sched.mc, m - r0);
    unsigned long long *tkey = (unsigned long long *)(w + p.off_tkey);
    uint32_t *tidx = (uint32_t *)(w + p.off_tidx);
    unsigned *cnt = (unsigned *)(w + p.off_cnt);
    Ent *cand = (Ent *)(w + p.off_cand);
    HIP_TRY(launch_f64_reset(tkey, tidx, cnt, rows, (unsigned)sched.s0, s));
    F64TopkArgs a{};
    a.q = dq + r0 * ldq;
    a.c = dc;
    a.qn = qn + r0;
    a.cn = cn;
    a.ldq = ldq;
    a.ldc = ldc;
    a.M = rows;
    a.D = (int)dp;
    a.metric = metric;
    a.tkey = tkey;
    a.tidx = tidx;
    a.cnt = cnt;
    a.cand = cand;
    a.cap = sched.cap;
    F64SelArgs sa{};
    sa.cand = cand;
    sa.cnt = cnt;
    sa.cap = sched.cap;
    sa.M = rows;
    sa.k = (int)k;
    sa.P = sched.cap;
    sa.tkey = tkey;
    sa.tidx = tidx;
    sa.metric = metric;
    sa.index_base = index_base;
    sa.out_idx = oi + r0 * k;
    sa.out_score = os + r0 * k;
    sa.overflow = flag;
    int64_t seen = 0, chunk = sched.s0;
    while (seen < n) {
      const int64_t cc = std::min<int64_t>(chunk, n - seen);
      a.col0 = (int)seen;
      a.ncol = (int)cc;
      a.accept_all = seen == 0;  // (s0 <= cap / 2)
      {
        Timed t("gemm_f64_topk", s);
        HIP_TRY(launch_gemm_f64_topk(a, s));
      }
      seen += cc;
      sa.mode = seen < n ? 0 : 1;
      {
        Timed t("select_f64", s);
        HIP_TRY(launch_f64_select(sa, s));
      }
      chunk = seen * sched.g;
    }
  }
  // the sign of zero scores (an overflowed call's lists are redone below, with theirs)
  HIP_TRY(launch_zero_sign_f64(dq, ldq, dc, ldc, qn, cn, (int)m, n, (int)d, (int)k, metric, index_base, oi, os, s));
  if (flag_copy) {
    HIP_TRY(hipMemcpyAsync(flag_copy, flag, 4, hipMemcpyDeviceToDevice, s));
    return PMM_OK;
  }
  // an overflowed row dropped candidates: redo the call on the materialised path
  unsigned of = 0;
  HIP_TRY(hipMemcpyAsync(&of, flag, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (of) return topk_f64_materialised(dq, ldq, m, dc, ldc, n, d, k, metric, index_base, oi, os, w, s, cn_pre);
  return PMM_OK;
}

// ---------------------------------------------------------------------------
// Corpus-sharded top-k over several devices from ONE host thread (the
// drop-in boundary's multi-GPU path; pmm_set_devices), for f32 rows, bf16
// compute and f64 rows (Polars' default Float64 columns): one memory plan
// (plan_sharded) and one driver (topk_sharded).  SURVEY 8e's plan in one
// process: the corpus is row-sharded (contiguous, sizes differ by <= 1), every
// device gets the queries and searches its shard with index_base = the shard's
// first global row, the shards' m x k lists are copied peer-to-peer (xGMI)
// into the root device's gather buffer and k-way merged there.  All devices
// work concurrently: every launch is asynchronous on the device's own stream
// of this thread; the root waits on per-shard events.  Each shard's list is
// the exact top-k of its rows under the row type's total order, so the merged
// list equals the one-device result bit for bit.
// ---------------------------------------------------------------------------
// One shard.  The rows and norms are of the search's row type: f32, f64, or
// bf16 rows with f32 norms under bf16 compute.
struct ShardSrc {
  int dev;
  int64_t lo, rows;
  const void *host;       // host corpus rows [lo, lo + rows), row stride d (f32 for bf16 compute), or
  const void *dev_rows;   // a corpus handle's resident rows at their padded stride
  const void *dev_norms;  // with dev_rows: the handle's norm array of this metric (nullptr for dot)
};

// The shards of n host rows (row stride d, elements of `elem` bytes) over a
// device list: one per listed device, at most n, contiguous, sizes differing by
// at most one.
int64_t shard_lo(int64_t n, int G, int g) { return n * g / G; }  // shard g: rows [n g / G, n (g + 1) / G)
std::vector<ShardSrc> host_shards(const std::vector<int> &devs, const void *c, int64_t n, int64_t d, size_t elem) {
  const int G = (int)std::min<int64_t>((int64_t)devs.size(), n);
  std::vector<ShardSrc> sh(G);
  for (int g = 0; g < G; g++) {
    const int64_t lo = shard_lo(n, G, g), hi = shard_lo(n, G, g + 1);
    sh[g] = ShardSrc{devs[g], lo, hi - lo, (const char *)c + (size_t)lo * d * elem, nullptr, nullptr};
  }
  return sh;
}

std::mutex g_peer_mu;
bool g_peer_tried[kMaxDevices][kMaxDevices];

// Lets `dev` read `peer`'s memory directly (xGMI) when the platform allows;
// a peer copy works either way, so failures are ignored.
void enable_peer(int dev, int peer) {
  if (dev == peer) return;
  std::lock_guard<std::mutex> lk(g_peer_mu);
  if (g_peer_tried[dev][peer]) return;
  g_peer_tried[dev][peer] = true;
  int can = 0;
  if (hipDeviceCanAccessPeer(&can, dev, peer) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(peer, 0);
  (void)hipGetLastError();
}

// What differs between the row types.
struct ShardRows {
  int dtype;                     // PMM_DTYPE_F32, _BF16 (f32 host rows and queries, searched as bf16) or _F64
  size_t host_elem, score_elem;  // bytes of a host row (and query) element, of a score
  // bf16: host rows and queries go up unpadded as f32 (staging rows of stride
  // d) and are rounded into a second, padded copy, which the kernels read
  bool staged;
  // f64: a shard is searched for k_g = min(k, rows) entries (a shorter list is
  // written compact, then laid behind empty slots: idx 0xFFFFFFFF, score NaN);
  // its fused scan's overflow flag has a slot in its device's plan, read once
  // every device has finished; a list's index and score planes are aligned
  // separately (f64_kway_merge_kernel).  f32, bf16: the kernels pad a short
  // list themselves, nothing is deferred, a list is one [2][m][k] block
  // (merge_kernel's strided loader, as for RCCL-gathered lists).
  bool f64;
};
ShardRows shard_rows(int dtype) {
  if (dtype == PMM_DTYPE_F64) return ShardRows{dtype, 8, 8, false, true};
  return ShardRows{dtype, 4, 4, dtype == PMM_DTYPE_BF16, false};
}

// Memory plan (pure: no HIP call, so the CPU tests check it through
// pmm_shard_plan).  One DevPlan per DISTINCT device of the list, in order of
// first use: that device's queries once, one workspace (its shards run in
// stream order), and per shard (ShardSlot) the uploaded rows (host shards only)
// and its lists; the root plan (the first shard's device) also holds the
// gathered lists of all G shards and the merged output.
struct DevPlan {
  int dev = 0;
  hipStream_t s = nullptr;
  char *base = nullptr;
  size_t off_q = 0, off_qb = 0, off_flags = 0, off_ws = 0, ws_bytes = 0, total = 0;
};
struct ShardSlot {
  int64_t k = 0;       // entries the shard is searched for (ShardRows::f64)
  bool fused = false;  // f64: the fused scan, whose flag is word `slot` at off_flags
  int slot = 0;        // the shard's place among its device's shards
  TopkRoute route;     // f32, bf16 (never screened)
  size_t off_c = 0, off_cb = 0;  // uploaded rows; bf16: their rounded copy
  size_t off_ti = 0, off_ts = 0, off_li = 0, off_ls = 0;  // the compact list of a short f64 shard; the m x k list
};
struct ShardLayout {
  ShardRows rt;
  int64_t m = 0, d = 0, dp = 0, k = 0;
  int metric = 0;
  std::vector<DevPlan> dps;
  std::vector<int> plan_of;  // shard -> index into dps
  std::vector<ShardSlot> sl;
  // in the root plan: shard g's gathered planes at off_gi / off_gs + g * gstride entries, the output planes
  size_t off_gi = 0, off_gs = 0, gstride = 0, off_oi = 0, off_os = 0;
};

void plan_sharded(int dtype, const std::vector<ShardSrc> &sh, int64_t m, int64_t d, int64_t k, int metric,
                  ShardLayout &L) {
  const int G = (int)sh.size();
  const ShardRows rt = shard_rows(dtype);
  const int64_t dp = padded_dim(dtype, d);
  const size_t mk = (size_t)m * k;
  L = ShardLayout{rt, m, d, dp, k, metric};
  L.plan_of.resize(G);
  L.sl.assign(G, ShardSlot());
  for (int g = 0; g < G; g++) {
    int j = 0;
    while (j < (int)L.dps.size() && L.dps[j].dev != sh[g].dev) j++;
    if (j == (int)L.dps.size()) {
      L.dps.push_back(DevPlan());
      L.dps[j].dev = sh[g].dev;
    }
    L.plan_of[g] = j;
  }
  // an index plane and a score plane of `count` entries each, from off on
  auto planes = [&](size_t &off, size_t count, size_t &oi, size_t &os) {
    oi = off;
    os = rt.f64 ? al256(off + count * 4) : off + count * 4;
    off = al256(os + count * rt.score_elem);
  };
  const size_t up_row = (size_t)(rt.staged ? d : dp) * rt.host_elem, rounded_row = rt.staged ? (size_t)dp * 2 : 0;
  for (int j = 0; j < (int)L.dps.size(); j++) {
    DevPlan &p = L.dps[j];
    size_t off = 0;
    p.off_q = off;
    off = al256(off + (size_t)m * up_row);
    p.off_qb = off;
    off = al256(off + (size_t)m * rounded_row);
    int ns = 0;
    for (int g = 0; g < G; g++) {
      if (L.plan_of[g] != j) continue;
      ShardSlot &t = L.sl[g];
      const int64_t rows = sh[g].rows;
      t.slot = ns++;
      t.k = rt.f64 ? std::min<int64_t>(k, rows) : k;
      if (rt.f64) {
        t.fused = f64_use_fused(m, rows, t.k);
        p.ws_bytes = std::max(p.ws_bytes, f64_workspace_bytes(m, rows, t.k, t.fused));
      } else {
        t.route = route_topk(m, rows, d, k, metric, rt.staged ? PMM_COMPUTE_BF16 : PMM_COMPUTE_F32,
                             device_cus(p.dev), false, true);
        p.ws_bytes = std::max(p.ws_bytes, t.route.total);
      }
      t.off_c = off;
      if (sh[g].host) off = al256(off + (size_t)rows * up_row);
      t.off_cb = off;
      if (sh[g].host) off = al256(off + (size_t)rows * rounded_row);  // (resident: the handle's rows)
      t.off_ti = t.off_ts = off;
      if (t.k < k) planes(off, (size_t)m * t.k, t.off_ti, t.off_ts);
      planes(off, mk, t.off_li, t.off_ls);
    }
    p.off_flags = off;
    if (rt.f64) off = al256(off + (size_t)ns * 4);
    p.off_ws = off;
    off = al256(off + p.ws_bytes);
    p.total = off;
  }
  DevPlan &rp = L.dps[L.plan_of[0]];
  size_t off = rp.total;
  L.off_gi = off;
  if (rt.f64) {  // [G][m][k] index plane, [G][m][k] score plane
    L.gstride = mk;
    L.off_gs = al256(off + (size_t)G * mk * 4);
    off = al256(L.off_gs + (size_t)G * mk * 8);
  } else {  // [G][2][m][k]
    L.gstride = 2 * mk;
    L.off_gs = off + mk * 4;
    off = al256(off + (size_t)G * 2 * mk * 4);
  }
  planes(off, mk, L.off_oi, L.off_os);
  rp.total = off;
}

// Every planned device's stream of this thread and an arena of its plan's size.
int acquire_devices(std::vector<DevPlan> &dps) {
  for (auto &p : dps) {
    HIP_TRY(hipSetDevice(p.dev));
    if (int rc = thread_stream(p.dev, &p.s)) return rc;
    void *b;
    if (int rc = arena(p.dev, p.s, p.total, &b)) return rc;
    p.base = (char *)b;
  }
  return PMM_OK;
}

// The per-shard completion events of a sharded search and its one exit: a
// failure first drains every device's stream (queued work writes into the
// arenas), then the events are destroyed on their devices.
struct ShardedExit {
  std::vector<DevPlan> &dps;
  const std::vector<ShardSrc> &sh;
  std::vector<hipEvent_t> ev;
  ShardedExit(std::vector<DevPlan> &dps_, const std::vector<ShardSrc> &sh_) : dps(dps_), sh(sh_), ev(sh_.size(), nullptr) {}
  int operator()(int code) {
    if (code != PMM_OK)
      for (auto &p : dps) {
        (void)hipSetDevice(p.dev);
        (void)hipStreamSynchronize(p.s);
      }
    for (size_t g = 0; g < ev.size(); g++)
      if (ev[g]) {
        (void)hipSetDevice(sh[g].dev);
        (void)hipEventDestroy(ev[g]);
      }
    return code;
  }
};

// What a row type supplies to the driver, each on the shard's device (current)
// and stream.  f32 and bf16 compute: shard g's host rows to the device and its
// fused top-k with global indices.
int search_shard_f32(const ShardLayout &L, int g, const ShardSrc &x) {
  const DevPlan &p = L.dps[L.plan_of[g]];
  const ShardSlot &t = L.sl[g];
  const int64_t m = L.m, d = L.d, dp = L.dp;
  uint32_t *li = (uint32_t *)(p.base + t.off_li);
  float *ls = (float *)(p.base + t.off_ls);
  // (a resident shard brings its norms; the query norms are this call's)
  const float *cn = x.host ? nullptr : (const float *)x.dev_norms;
  if (L.rt.staged) {
    const uint16_t *cb = (const uint16_t *)x.dev_rows;
    if (x.host) {
      HIP_TRY(hipMemcpyAsync(p.base + t.off_c, x.host, (size_t)x.rows * d * 4, hipMemcpyHostToDevice, p.s));
      HIP_TRY(launch_f32_to_bf16((const float *)(p.base + t.off_c), x.rows, d, d, (uint16_t *)(p.base + t.off_cb), dp,
                                 p.s));
      cb = (const uint16_t *)(p.base + t.off_cb);
    }
    return topk_bf16_device_impl(t.route, (const uint16_t *)(p.base + p.off_qb), dp, m, cb, dp, x.rows, d, L.k,
                                 L.metric, (uint32_t)x.lo, li, ls, p.base + p.off_ws, p.ws_bytes, p.s, p.dev, nullptr,
                                 cn);
  }
  const float *c = (const float *)x.dev_rows;
  if (x.host) {
    if (int rc = upload_padded(p.base + t.off_c, x.host, x.rows, d, dp, 4, p.s)) return rc;
    c = (const float *)(p.base + t.off_c);
  }
  return topk_f32_device_impl(t.route, (const float *)(p.base + p.off_q), dp, m, c, dp, x.rows, d, L.k, L.metric,
                              (uint32_t)x.lo, li, ls, p.base + p.off_ws, p.ws_bytes, p.s, p.dev, cn);
}

// f64: the same with topk_f64_device_impl, which copies the fused scan's
// overflow flag into the shard's slot instead of waiting for it.  rerun: the
// shard again on the materialised path (its rows are on the device already).
int search_shard_f64(const ShardLayout &L, int g, const ShardSrc &x, bool rerun) {
  const DevPlan &p = L.dps[L.plan_of[g]];
  const ShardSlot &t = L.sl[g];
  const int64_t m = L.m, d = L.d, dp = L.dp, k = L.k;
  const double *q = (const double *)(p.base + p.off_q), *cn = (const double *)x.dev_norms;
  const double *c = x.host ? (const double *)(p.base + t.off_c) : (const double *)x.dev_rows;
  unsigned *flag = (unsigned *)(p.base + p.off_flags) + t.slot;
  if (!rerun) {
    if (x.host)
      if (int rc = upload_padded(p.base + t.off_c, x.host, x.rows, d, dp, 8, p.s)) return rc;
    HIP_TRY(hipMemsetAsync(flag, 0, 4, p.s));
  }
  uint32_t *li = (uint32_t *)(p.base + t.off_li), *oi = li;
  double *ls = (double *)(p.base + t.off_ls), *os = ls;
  if (t.k < k) {
    oi = (uint32_t *)(p.base + t.off_ti);
    os = (double *)(p.base + t.off_ts);
    HIP_TRY(hipMemsetAsync(li, 0xFF, (size_t)m * k * 4, p.s));
    HIP_TRY(hipMemsetAsync(ls, 0xFF, (size_t)m * k * 8, p.s));  // (all-ones f64: a NaN)
  }
  const int rc = rerun ? topk_f64_materialised(q, dp, m, c, dp, x.rows, d, t.k, L.metric, (uint32_t)x.lo, oi, os,
                                               p.base + p.off_ws, p.s, cn)
                       : topk_f64_device_impl(q, dp, m, c, dp, x.rows, d, t.k, L.metric, (uint32_t)x.lo, oi, os,
                                              p.base + p.off_ws, p.s, t.fused, cn, t.fused ? flag : nullptr);
  if (rc) return rc;
  if (t.k < k) {
    HIP_TRY(hipMemcpy2DAsync(li, (size_t)k * 4, oi, (size_t)t.k * 4, (size_t)t.k * 4, (size_t)m,
                             hipMemcpyDeviceToDevice, p.s));
    HIP_TRY(hipMemcpy2DAsync(ls, (size_t)k * 8, os, (size_t)t.k * 8, (size_t)t.k * 8, (size_t)m,
                             hipMemcpyDeviceToDevice, p.s));
  }
  return PMM_OK;
}

// f64, once every device has finished: an overflowed shard re-runs
// materialised (its rows, its workspace), as one device would.
int rerun_overflowed_f64(const ShardLayout &L, int g, const ShardSrc &x) {
  const DevPlan &p = L.dps[L.plan_of[g]];
  if (!L.sl[g].fused) return PMM_OK;
  unsigned of = 0;
  HIP_TRY(hipMemcpy(&of, (unsigned *)(p.base + p.off_flags) + L.sl[g].slot, 4, hipMemcpyDeviceToHost));
  return of ? search_shard_f64(L, g, x, true) : PMM_OK;
}

// The root's k-way merge of the G gathered lists (each best first) into the
// output planes, on the root's stream.
int merge_shards(const ShardLayout &L, int G, const DevPlan &rp) {
  const int64_t m = L.m, k = L.k;
  uint32_t *gi = (uint32_t *)(rp.base + L.off_gi), *oi = (uint32_t *)(rp.base + L.off_oi);
  if (L.rt.f64) {
    F64MergeArgs ma{};
    ma.gi = gi;
    ma.gs = (double *)(rp.base + L.off_gs);
    ma.list_stride = m * k;
    ma.M = (int)m;
    ma.G = G;
    ma.k = (int)k;
    ma.metric = L.metric;
    ma.out_idx = oi;
    ma.out_score = (double *)(rp.base + L.off_os);
    Timed t("merge_devices_f64", rp.s);
    HIP_TRY(launch_f64_merge(ma, rp.s));
    return PMM_OK;
  }
  const MergeArgs ma = merge_lists_args(gi, (const float *)(rp.base + L.off_gs), m, G, k, k, 2 * m * k, k, L.metric,
                                        true, oi, (float *)(rp.base + L.off_os));
  Timed t("merge_devices", rp.s);
  HIP_TRY(launch_merge(ma, 1, rp.s));
  // (the shards' zero scores carry their signs; the merge's keys fold them)
  if (L.metric != kMetricEuclidean)
    HIP_TRY(launch_zero_sign_lists(ma.in_idx, ma.in_score, G, (int)k, k, 2 * m * k, (int)m, (int)k, ma.out_idx,
                                   ma.out_score, rp.s));
  return PMM_OK;
}

// The driver.  q, out_score: f32 (dtype f32, bf16) or f64.
int topk_sharded(int dtype, const void *q, int64_t m, int64_t d, int64_t k, int metric, const std::vector<ShardSrc> &sh,
                 uint32_t *out_idx, void *out_score) {
  const int G = (int)sh.size();
  DevScope restore;
  HIP_TRY(hipGetDevice(&restore.prev));
  const int root = sh[0].dev;
  for (const ShardSrc &x : sh)
    if (int rc = probe_device(x.dev)) return rc;
  ShardLayout L;
  plan_sharded(dtype, sh, m, d, k, metric, L);
  const ShardRows &rt = L.rt;
  std::vector<DevPlan> &dps = L.dps;
  DevPlan &rp = dps[L.plan_of[0]];
  if (int rc = acquire_devices(dps)) return rc;
  ShardedExit finish(dps, sh);
#define SH_TRY(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return finish(fail(PMM_ERR_HIP, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), \
                         __FILE__, __LINE__, #expr));                                     \
  } while (0)
#define SH_RC(expr)                        \
  do {                                     \
    int rc_ = (expr);                      \
    if (rc_ != PMM_OK) return finish(rc_); \
  } while (0)
  // queries to every device
  for (auto &p : dps) {
    SH_TRY(hipSetDevice(p.dev));
    if (rt.staged) {
      SH_TRY(hipMemcpyAsync(p.base + p.off_q, q, (size_t)m * d * 4, hipMemcpyHostToDevice, p.s));
      SH_TRY(launch_f32_to_bf16((const float *)(p.base + p.off_q), m, d, d, (uint16_t *)(p.base + p.off_qb), L.dp,
                                p.s));
    } else {
      SH_RC(upload_padded(p.base + p.off_q, q, m, d, L.dp, rt.host_elem, p.s));
    }
  }
  // per shard: rows, top-k with global indices, completion event.  All devices
  // work concurrently: every launch is asynchronous on the device's own stream
  // of this thread.  f64 defers the events behind the overflow flags, which are
  // read only once every device is done.
  auto record = [&](int g) -> int {
    HIP_TRY(hipEventCreateWithFlags(&finish.ev[g], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(finish.ev[g], dps[L.plan_of[g]].s));
    return PMM_OK;
  };
  for (int g = 0; g < G; g++) {
    SH_TRY(hipSetDevice(sh[g].dev));
    SH_RC(rt.f64 ? search_shard_f64(L, g, sh[g], false) : search_shard_f32(L, g, sh[g]));
    if (!rt.f64) SH_RC(record(g));
  }
  if (rt.f64) {
    for (auto &p : dps) {
      SH_TRY(hipSetDevice(p.dev));
      SH_TRY(hipStreamSynchronize(p.s));
    }
    for (int g = 0; g < G; g++) {
      SH_TRY(hipSetDevice(sh[g].dev));
      SH_RC(rerun_overflowed_f64(L, g, sh[g]));
      SH_RC(record(g));
    }
  }
  // gather into the root (peer copies over xGMI; the root waits on the shards'
  // events), merge, download
  SH_TRY(hipSetDevice(root));
  const size_t mk = (size_t)m * k;
  for (int g = 0; g < G; g++) {
    enable_peer(root, sh[g].dev);
    SH_TRY(hipStreamWaitEvent(rp.s, finish.ev[g], 0));
    const char *pb = dps[L.plan_of[g]].base;
    char *di = rp.base + L.off_gi + (size_t)g * L.gstride * 4;
    if (rt.f64) {
      SH_TRY(hipMemcpyPeerAsync(di, root, pb + L.sl[g].off_li, sh[g].dev, mk * 4, rp.s));
      SH_TRY(hipMemcpyPeerAsync(rp.base + L.off_gs + (size_t)g * L.gstride * 8, root, pb + L.sl[g].off_ls, sh[g].dev,
                                mk * 8, rp.s));
    } else {  // (a [2][m][k] block at both ends: one copy)
      SH_TRY(hipMemcpyPeerAsync(di, root, pb + L.sl[g].off_li, sh[g].dev, 2 * mk * 4, rp.s));
    }
  }
  SH_RC(merge_shards(L, G, rp));
  SH_TRY(hipMemcpyAsync(out_idx, rp.base + L.off_oi, mk * 4, hipMemcpyDeviceToHost, rp.s));
  SH_TRY(hipMemcpyAsync(out_score, rp.base + L.off_os, mk * rt.score_elem, hipMemcpyDeviceToHost, rp.s));
  SH_TRY(hipStreamSynchronize(rp.s));
#undef SH_TRY
#undef SH_RC
  return finish(PMM_OK);
}

// ---------------------------------------------------------------------------
// int8 top-k (pmm_i8.hip; DESIGN.md §4d "Int8 rows"): the f64 branch's answer for rows of
// signed bytes -- indices and f64 score bits -- from the int8 MFMA.  One route
// per call, decided here: the workspace is sized by it and the executor
// follows it.
//   native   padded d <= kI8MaxD and k <= kFusedMaxK: the chunked int8 scan
//            with an exact f64 finish; rows whose candidate buffer overflowed
//            (many equal rows at the k-th place) are re-run widened;
//   widened  otherwise: both sides widened to f64 in the workspace (exact) and
//            searched by topk_f64_device_impl, the old route at the old rate.
// ---------------------------------------------------------------------------
struct I8Route {
  bool native = false;
  ChunkSchedule sched;  // native
  size_t off_count = 0, off_qs = 0, off_qf = 0, off_cs = 0, off_cf = 0, off_tkey = 0, off_tidx = 0, off_cnt = 0,
         off_ovf = 0, off_rows = 0, off_cand = 0;
  bool fused64 = false;  // widened: the f64 path's own route
  int64_t dp64 = 0;
  size_t off_q64 = 0, off_c64 = 0, off_w64 = 0;
  size_t total = 0;
};

// The candidate-buffer capacity: chunk_cap's, which PMM_I8_CAP (per call; a
// power of two from 64 up, below the rule's value) lowers, so that a test
// reaches the overflow re-run with a small corpus.
int i8_cap(int64_t k) {
  const int cap = chunk_cap(k);
  const char *e = getenv("PMM_I8_CAP");
  const int v = e ? atoi(e) : 0;
  return (v >= 64 && v < cap && (v & (v - 1)) == 0) ? v : cap;
}

I8Route route_i8(int64_t m, int64_t n, int64_t d, int64_t k) {
  I8Route r;
  const int64_t dp = padded_dim(PMM_DTYPE_I8, d);
  r.native = dp <= kI8MaxD && k <= kFusedMaxK;
  size_t off = 0;
  if (!r.native) {
    r.dp64 = padded_dim(PMM_DTYPE_F64, d);
    r.fused64 = f64_use_fused(m, n, k);
    r.off_q64 = off;
    off = al256(off + (size_t)m * r.dp64 * 8);
    r.off_c64 = off;
    off = al256(off + (size_t)n * r.dp64 * 8);
    r.off_w64 = off;
    r.total = off + f64_workspace_bytes(m, n, k, r.fused64);
    return r;
  }
  r.sched = chunk_schedule(m, n, k, i8_cap(k));
  const int64_t mc = r.sched.mc;
  r.off_count = off;
  off += 256;
  r.off_qs = off;
  off = al256(off + (size_t)m * 4);
  r.off_qf = off;
  off = al256(off + (size_t)m * 4);
  r.off_cs = off;
  off = al256(off + (size_t)n * 4);
  r.off_cf = off;
  off = al256(off + (size_t)n * 4);
  r.off_tkey = off;
  off = al256(off + (size_t)mc * 4);
  r.off_tidx = off;
  off = al256(off + (size_t)mc * 4);
  r.off_cnt = off;
  off = al256(off + (size_t)mc * 4);
  r.off_ovf = off;
  off = al256(off + (size_t)mc * 4);
  r.off_rows = off;
  off = al256(off + (size_t)m * 4);
  r.off_cand = off;
  off = al256(off + (size_t)mc * r.sched.cap * 16);
  r.total = off;
  return r;
}

// The listed query rows (device `rows`, r of them) searched again on the f64
// path: they and the whole corpus widened into an allocation of the call's
// own, the lists scattered to the rows' places.  Synchronises.
int i8_rerun_rows(const int8_t *dq, int64_t ldq, const int *rows, int64_t r, const int8_t *dc, int64_t ldc, int64_t n,
                  int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *oi, double *os, hipStream_t s) {
  const int64_t dp64 = padded_dim(PMM_DTYPE_F64, d);
  const bool fused = f64_use_fused(r, n, k);
  const size_t o_c = al256((size_t)r * dp64 * 8), o_i = o_c + al256((size_t)n * dp64 * 8),
               o_s = o_i + al256((size_t)r * k * 4), o_w = o_s + al256((size_t)r * k * 8);
  char *tmp = nullptr;
  hipError_t e = hipMalloc(&tmp, o_w + f64_workspace_bytes(r, n, k, fused));
  if (e != hipSuccess) return fail(PMM_ERR_HIP, "int8 re-run allocation failed: %s", hipGetErrorString(e));
  int rc = PMM_OK;
  {
    Timed t("widen_i8_f64", s);
    e = launch_i8_widen(dq, ldq, rows, r, (int)d, (double *)tmp, dp64, s);
    if (e == hipSuccess) e = launch_i8_widen(dc, ldc, nullptr, n, (int)d, (double *)(tmp + o_c), dp64, s);
  }
  if (e == hipSuccess)
    rc = topk_f64_device_impl((const double *)tmp, dp64, r, (const double *)(tmp + o_c), dp64, n, d, k, metric,
                              index_base, (uint32_t *)(tmp + o_i), (double *)(tmp + o_s), tmp + o_w, s, fused);
  if (e == hipSuccess && rc == PMM_OK)
    e = launch_i8_scatter((const uint32_t *)(tmp + o_i), (const double *)(tmp + o_s), rows, r, (int)k, oi, os, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // (before the buffer is freed)
  (void)hipFree(tmp);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return fail(PMM_ERR_HIP, "int8 re-run failed: %s", hipGetErrorString(e));
  return rc;
}

// The executor over the route's workspace w (route.total bytes).  dq / dc:
// device rows of signed bytes, strides multiples of 16 and >= roundup(d, 64),
// zero-padded.  cs_pre / cf_pre: the corpus rows' sums of squares and factors
// already on the device (a handle's), else nullptr.  Synchronises the stream
// (the overflow count is read back).
int topk_i8_device_impl(const I8Route &r, const int8_t *dq, int64_t ldq, int64_t m, const int8_t *dc, int64_t ldc,
                        int64_t n, int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *oi, double *os,
                        char *w, hipStream_t s, const uint32_t *cs_pre = nullptr, const float *cf_pre = nullptr) {
  if (!r.native) {
    double *q64 = (double *)(w + r.off_q64), *c64 = (double *)(w + r.off_c64);
    {
      Timed t("widen_i8_f64", s);
      HIP_TRY(launch_i8_widen(dq, ldq, nullptr, m, (int)d, q64, r.dp64, s));
      HIP_TRY(launch_i8_widen(dc, ldc, nullptr, n, (int)d, c64, r.dp64, s));
    }
    if (int rc = topk_f64_device_impl(q64, r.dp64, m, c64, r.dp64, n, d, k, metric, index_base, oi, os, w + r.off_w64,
                                      s, r.fused64))
      return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return PMM_OK;
  }
  const int64_t dp = padded_dim(PMM_DTYPE_I8, d);
  unsigned *count = (unsigned *)(w + r.off_count);
  uint32_t *qs = (uint32_t *)(w + r.off_qs), *cs = (uint32_t *)(w + r.off_cs);
  float *qf = (float *)(w + r.off_qf), *cf = (float *)(w + r.off_cf);
  int *rows = (int *)(w + r.off_rows);
  HIP_TRY(hipMemsetAsync(count, 0, 4, s));
  {
    Timed t("norms_i8", s);
    HIP_TRY(launch_i8_norms(dq, m, ldq, (int)dp, qs, qf, s));
    if (cs_pre) {
      cs = (uint32_t *)cs_pre;
      cf = (float *)cf_pre;
    } else {
      HIP_TRY(launch_i8_norms(dc, n, ldc, (int)dp, cs, cf, s));
    }
  }
  const ChunkSchedule &sched = r.sched;
  for (int64_t r0 = 0; r0 < m; r0 += sched.mc) {
    const int rws = (int)std::min<int64_t>(sched.mc, m - r0);
    uint32_t *tkey = (uint32_t *)(w + r.off_tkey), *tidx = (uint32_t *)(w + r.off_tidx);
    unsigned *cnt = (unsigned *)(w + r.off_cnt), *ovf = (unsigned *)(w + r.off_ovf);
    Ent *cand = (Ent *)(w + r.off_cand);
    HIP_TRY(launch_i8_reset(tkey, tidx, cnt, ovf, rws, s));
    I8TopkArgs a{};
    a.q = dq + r0 * ldq;
    a.c = dc;
    a.qs = qs + r0;
    a.cs = cs;
    a.qf = qf + r0;
    a.cf = cf;
    a.ldq = ldq;
    a.ldc = ldc;
    a.M = rws;
    a.D = (int)dp;
    a.metric = metric;
    a.tkey = tkey;
    a.tidx = tidx;
    a.cnt = cnt;
    a.cand = cand;
    a.cap = sched.cap;
    I8SelArgs sa{};
    sa.cand = cand;
    sa.cnt = cnt;
    sa.cap = sched.cap;
    sa.M = rws;
    sa.k = (int)k;
    sa.P = sched.cap;
    sa.tkey = tkey;
    sa.tidx = tidx;
    sa.ovf = ovf;
    sa.metric = metric;
    sa.qs = qs + r0;
    sa.cs = cs;
    sa.index_base = index_base;
    sa.out_idx = oi + r0 * k;
    sa.out_score = os + r0 * k;
    int64_t seen = 0, chunk = sched.s0;
    while (seen < n) {
      const int64_t cc = std::min<int64_t>(chunk, n - seen);
      a.col0 = (int)seen;
      a.ncol = (int)cc;
      {
        Timed t("gemm_i8_topk", s);
        HIP_TRY(launch_gemm_i8_topk(a, s));
      }
      seen += cc;
      if (seen < n) {
        Timed t("select_i8", s);
        HIP_TRY(launch_i8_select(sa, s));
      } else {
        Timed t("i8_finish", s);
        HIP_TRY(launch_i8_finish(sa, s));
      }
      chunk = seen * sched.g;
    }
    HIP_TRY(launch_i8_collect(ovf, rws, (int)r0, count, rows, s));
  }
  // rows that dropped candidates: again, on the widened rows
  unsigned nov = 0;
  HIP_TRY(hipMemcpyAsync(&nov, count, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (nov) return i8_rerun_rows(dq, ldq, rows, nov, dc, ldc, n, d, k, metric, index_base, oi, os, s);
  return PMM_OK;
}

// What every int8 entry checks before it touches a device.
int validate_i8(int64_t m, int64_t n, int64_t d, int64_t k, int metric) {
  int rc = validate_sizes(m, n, d, k, true);
  if (rc) return rc;
  if ((rc = check_metric(metric))) return rc;
  if (d >= kI8DimLimit)
    return fail(PMM_ERR_UNSUPPORTED, "int8 rows take d < %d (got %lld): a sum of squares must fit in 32 bits",
                kI8DimLimit, (long long)d);
  return PMM_OK;
}

// ---------------------------------------------------------------------------
// Hamming top-k over bit rows (pmm_bits.hip; DESIGN.md §4d "Bit rows"): rows of
// w packed bytes, the integer distance popcount(q ^ c) as an f64 score, lower
// first, ties to the lower index.  One route per call, decided here: the
// workspace is sized by it and the executor follows it.
//   native   k <= kFusedMaxK: the chunked scan on the int8 MFMA with the
//            euclidean key over the rows' popcounts; rows whose candidate
//            buffer overflowed are gathered and scanned again in chunks of
//            cap - k columns, which cannot overflow (a select leaves at most k
//            entries), and their lists written to the rows' places;
//   widened  otherwise: both sides expanded to 0/1 f64 rows in the workspace
//            and searched by topk_f64_device_impl (euclidean); the score is
//            rint(s * s).
// ---------------------------------------------------------------------------
struct BitsRoute {
  bool native = false;
  ChunkSchedule sched;  // native
  size_t off_count = 0, off_qs = 0, off_cs = 0, off_tkey = 0, off_tidx = 0, off_cnt = 0, off_ovf = 0, off_rows = 0,
         off_gq = 0, off_gqs = 0, off_cand = 0;
  bool fused64 = false;  // widened: the f64 path's own route
  int64_t dp64 = 0;
  size_t off_q64 = 0, off_c64 = 0, off_w64 = 0;
  size_t total = 0;
};

// The candidate-buffer capacity: chunk_cap's, which PMM_BITS_CAP (per call; a
// power of two from 64 up, above k and below the rule's value) lowers, so that
// a test reaches the overflow re-run with a small corpus.
int bits_cap(int64_t k) {
  const int cap = chunk_cap(k);
  const char *e = getenv("PMM_BITS_CAP");
  const int v = e ? atoi(e) : 0;
  return (v >= 64 && v > k && v < cap && (v & (v - 1)) == 0) ? v : cap;
}

BitsRoute route_bits(int64_t m, int64_t n, int64_t w, int64_t k) {
  BitsRoute r;
  const int64_t dp = padded_dim(PMM_DTYPE_BITS, w);
  r.native = k <= kFusedMaxK;
  Layout L;
  if (!r.native) {
    r.dp64 = padded_dim(PMM_DTYPE_F64, 8 * w);
    r.fused64 = f64_use_fused(m, n, k);
    r.off_q64 = L.take((size_t)m * r.dp64 * 8);
    r.off_c64 = L.take((size_t)n * r.dp64 * 8);
    r.off_w64 = L.off;
    r.total = L.off + f64_workspace_bytes(m, n, k, r.fused64);
    return r;
  }
  r.sched = chunk_schedule(m, n, k, bits_cap(k));
  const int64_t mc = r.sched.mc;
  r.off_count = L.take(4);
  r.off_qs = L.take((size_t)m * 4);
  r.off_cs = L.take((size_t)n * 4);
  r.off_tkey = L.take((size_t)mc * 4);
  r.off_tidx = L.take((size_t)mc * 4);
  r.off_cnt = L.take((size_t)mc * 4);
  r.off_ovf = L.take((size_t)mc * 4);
  r.off_rows = L.take((size_t)m * 4);
  r.off_gq = L.take((size_t)m * dp);  // the re-run's gathered rows and their popcounts
  r.off_gqs = L.take((size_t)m * 4);
  r.off_cand = L.take((size_t)mc * r.sched.cap * 16);
  r.total = L.off;
  return r;
}

// The executor over the route's workspace w (route.total bytes).  dq / dc:
// device rows of packed bytes, strides multiples of 16 and >= roundup(wb, 16),
// zero-padded.  cs_pre: the corpus rows' popcounts already on the device (a
// handle's), else nullptr.  Synchronises the stream (the overflow count is
// read back).
int topk_bits_device_impl(const BitsRoute &r, const uint8_t *dq, int64_t ldq, int64_t m, const uint8_t *dc,
                          int64_t ldc, int64_t n, int64_t wb, int64_t k, uint32_t index_base, uint32_t *oi,
                          double *os, char *w, hipStream_t s, const uint32_t *cs_pre = nullptr) {
  if (!r.native) {
    double *q64 = (double *)(w + r.off_q64), *c64 = (double *)(w + r.off_c64);
    {
      Timed t("widen_bits_f64", s);
      HIP_TRY(launch_bits_widen(dq, ldq, m, (int)wb, q64, r.dp64, s));
      HIP_TRY(launch_bits_widen(dc, ldc, n, (int)wb, c64, r.dp64, s));
    }
    if (int rc = topk_f64_device_impl(q64, r.dp64, m, c64, r.dp64, n, 8 * wb, k, kMetricEuclidean, index_base, oi, os,
                                      w + r.off_w64, s, r.fused64))
      return rc;
    HIP_TRY(launch_bits_square(os, m * k, s));
    HIP_TRY(hipStreamSynchronize(s));
    return PMM_OK;
  }
  const int64_t dp = padded_dim(PMM_DTYPE_BITS, wb);
  unsigned *count = (unsigned *)(w + r.off_count);
  uint32_t *qs = (uint32_t *)(w + r.off_qs), *cs = (uint32_t *)(w + r.off_cs);
  int *rows = (int *)(w + r.off_rows);
  uint32_t *tkey = (uint32_t *)(w + r.off_tkey), *tidx = (uint32_t *)(w + r.off_tidx);
  unsigned *cnt = (unsigned *)(w + r.off_cnt), *ovf = (unsigned *)(w + r.off_ovf);
  Ent *cand = (Ent *)(w + r.off_cand);
  HIP_TRY(hipMemsetAsync(count, 0, 4, s));
  {
    Timed t("bits_popcount", s);
    HIP_TRY(launch_bits_popcount(dq, m, ldq, (int)dp, qs, s));
    if (cs_pre) {
      cs = (uint32_t *)cs_pre;
    } else {
      HIP_TRY(launch_bits_popcount(dc, n, ldc, (int)dp, cs, s));
    }
  }
  const ChunkSchedule &sched = r.sched;
  // One scan of `mq` rows (q, their popcounts pq) in passes of sched.mc.  map
  // nullptr: the schedule's growing chunks, lists to rows r0 .. of oi / os,
  // overflowed rows collected; map: the re-run of the gathered rows map[i], in
  // chunks of cap - k columns.
  auto scan = [&](const uint8_t *q, int64_t ld, const uint32_t *pq, int64_t mq, const int *map) -> int {
    for (int64_t r0 = 0; r0 < mq; r0 += sched.mc) {
      const int rws = (int)std::min<int64_t>(sched.mc, mq - r0);
      HIP_TRY(launch_i8_reset(tkey, tidx, cnt, ovf, rws, s));
      I8TopkArgs a{};
      a.q = (const int8_t *)(q + r0 * ld);
      a.c = (const int8_t *)dc;
      a.qs = pq + r0;
      a.cs = cs;
      a.ldq = ld;
      a.ldc = ldc;
      a.M = rws;
      a.D = (int)dp;
      a.metric = kMetricEuclidean;
      a.tkey = tkey;
      a.tidx = tidx;
      a.cnt = cnt;
      a.cand = cand;
      a.cap = sched.cap;
      I8SelArgs sa{};
      sa.cand = cand;
      sa.cnt = cnt;
      sa.cap = sched.cap;
      sa.M = rws;
      sa.k = (int)k;
      sa.P = sched.cap;
      sa.tkey = tkey;
      sa.tidx = tidx;
      sa.ovf = ovf;
      sa.metric = kMetricEuclidean;  // (the select's exact rule: the k-th entry itself)
      sa.qs = pq + r0;
      sa.cs = cs;
      sa.index_base = index_base;
      sa.out_idx = map ? oi : oi + r0 * k;
      sa.out_score = map ? os : os + r0 * k;
      int64_t seen = 0, chunk = map ? sched.cap - k : sched.s0;
      while (seen < n) {
        const int64_t cc = std::min<int64_t>(chunk, n - seen);
        a.col0 = (int)seen;
        a.ncol = (int)cc;
        {
          Timed t("gemm_bits_topk", s);
          HIP_TRY(launch_gemm_bits_topk(a, s));
        }
        seen += cc;
        if (seen < n) {
          Timed t("select_bits", s);
          HIP_TRY(launch_i8_select(sa, s));
        } else {
          Timed t("bits_finish", s);
          HIP_TRY(launch_bits_finish(sa, map ? map + r0 : nullptr, s));
        }
        if (!map) chunk = seen * sched.g;
      }
      if (!map) HIP_TRY(launch_i8_collect(ovf, rws, (int)r0, count, rows, s));
    }
    return PMM_OK;
  };
  if (int rc = scan(dq, ldq, qs, m, nullptr)) return rc;
  // rows that dropped candidates: again, in chunks that cannot overflow
  unsigned nov = 0;
  HIP_TRY(hipMemcpyAsync(&nov, count, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (nov) {
    uint8_t *gq = (uint8_t *)(w + r.off_gq);
    uint32_t *gqs = (uint32_t *)(w + r.off_gqs);
    {
      Timed t("bits_gather", s);
      HIP_TRY(launch_bits_gather(dq, ldq, rows, nov, gq, dp, qs, gqs, s));
    }
    if (int rc = scan(gq, dp, gqs, nov, rows)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
  }
  return PMM_OK;
}

// What every bit-row entry checks before it touches a device.
int validate_bits(int64_t m, int64_t n, int64_t w, int64_t k) {
  int rc = validate_sizes(m, n, w, k, true);
  if (rc) return rc;
  if (w > kBitsMaxW)
    return fail(PMM_ERR_UNSUPPORTED, "bit rows take w <= %d bytes (got %lld): split wider rows and add the distances",
                kBitsMaxW, (long long)w);
  return PMM_OK;
}

}  // namespace

// Device-resident corpus (pmm_corpus_*): padded f32 rows in HBM plus the
// norms / pre-filter factors of every metric, computed once at creation.
// With a device list set (pmm_set_devices) the rows are sharded over the
// devices at creation, one contiguous shard each.
// A Float64 corpus (pmm_corpus_create_f64; Polars' default float columns
// take the reference's f64 branch, src/matmul.rs:449-468) keeps its rows in
// f64 with the f64 norms of both metrics, sharded over a device list the same
// way (round 6).
// A bf16 corpus (pmm_corpus_create_bf16) keeps the rows rounded to bf16 at
// stride roundup(d, 128) -- what the bf16 kernels read -- and the f32 norms of
// the rounded rows in the f32 layout, both from one round_norms_bf16 pass.
// What the three kinds of handle store differs only by row_kind(dtype).
struct CorpusShard {
  int device = 0;
  int64_t lo = 0, n = 0;  // rows [lo, lo + n) of the corpus
  void *rows = nullptr;   // n x dp elements of the handle's row type
  void *norms = nullptr;  // the row type's norm arrays, n norms each (RowKind)
  template <typename T>
  const T *rows_as() const {
    return (const T *)rows;
  }
};
struct pmm_corpus {
  int64_t n = 0, d = 0, dp = 0;
  int dtype = PMM_DTYPE_F32;
  std::vector<CorpusShard> shards;
  // An f32 handle of one shard: the corpus' share of the cosine screen's
  // inputs (shard 0's rows), built under screen_mu by the
  // first pmm_topk_f32_corpus call whose shape asks for the screen and
  // published whole (release / acquire; a call reads the pointer once).
  // screen_never: the corpus has an unsafe row -- no image is kept and no
  // later call screens.
  mutable std::mutex screen_mu;
  mutable std::atomic<const ScreenImage *> screen{nullptr};
  mutable std::atomic<bool> screen_never{false};
  // A derived handle (pmm_corpus_subset_*): its row i is the
  // parent's row map[i], ascending (n entries on shard 0's device); the top-k
  // entries return map[i].  NULL: not derived.
  uint32_t *map = nullptr;
  // A partitioned handle (pmm_corpus_partition): the rows are
  // stored group by group, group g in rows [offsets[g], offsets[g + 1]), in
  // ascending parent order inside a group; `map` is then ascending only
  // inside a group, so the handle serves the grouped entries alone.
  // offsets: G + 1 entries on the host, d_offsets their copy on shard 0's
  // device.  Empty: not partitioned.
  std::vector<int64_t> offsets;
  int64_t *d_offsets = nullptr;
  bool partitioned() const { return !offsets.empty(); }
  // A multi-vector handle (pmm_corpus_create_f32_docs; DESIGN.md §4d
  // "Multi-vector rows"): document c is rows [doc_offsets[c], doc_offsets[c +
  // 1]), n_docs + 1 strictly ascending entries on the host, d_doc_offsets their
  // copy on shard 0's device.  Empty: no documents.  Only pmm_topk_f32_maxsim
  // reads them: every other entry sees the plain f32 handle of the rows.
  std::vector<int64_t> doc_offsets;
  int64_t *d_doc_offsets = nullptr;
};

static void free_screen_image(const ScreenImage *img) {
  if (!img) return;
  if (img->cb) (void)hipFree(img->cb);
  if (img->crel) (void)hipFree(img->crel);
  delete img;
}

// The norm array of shard x that `metric` reads (nullptr for dot); T is the
// row type's norm type.
template <typename T>
static const T *shard_norms(const pmm_corpus *h, const CorpusShard &x, int metric) {
  const int64_t off = row_kind(h->dtype).norm_offset(metric, x.n);
  return off < 0 ? nullptr : (const T *)x.norms + off;
}

// A ScreenImage with the buffers for n rows of d columns on the current
// device, when they fit in half of the free HBM; else, or when an allocation
// fails, nullptr with the HIP error cleared (the caller goes on without one).
static ScreenImage *alloc_screen_image(int64_t n, int64_t d) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || screen_image_bytes(n, d) > free_b / 2) {
    (void)hipGetLastError();
    return nullptr;
  }
  ScreenImage *ni = new ScreenImage();
  hipError_t e = hipMalloc(&ni->cb, (size_t)n * padded_dim(PMM_DTYPE_BF16, d) * 2);
  if (e == hipSuccess) e = hipMalloc(&ni->crel, (size_t)n * 8);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    free_screen_image(ni);
    return nullptr;
  }
  return ni;
}

// The handle's ScreenImage on the current device (shard 0's) and stream s,
// built and published on first use.  nullptr: the handle does not screen this
// call -- the image does not fit in half of the free HBM or an allocation
// failed (a later call tries again), or the corpus has an unsafe row (read
// back once, here: no later call tries).
static const ScreenImage *corpus_screen_image(const pmm_corpus *h, hipStream_t s) {
  const ScreenImage *img = h->screen.load(std::memory_order_acquire);
  if (img || h->screen_never.load(std::memory_order_acquire)) return img;
  std::lock_guard<std::mutex> lk(h->screen_mu);
  img = h->screen.load(std::memory_order_acquire);
  if (img || h->screen_never.load(std::memory_order_acquire)) return img;
  ScreenImage *ni = alloc_screen_image(h->n, h->d);
  if (!ni) return nullptr;
  unsigned *scal = nullptr;  // [0] max residual bound over the safe rows, [1] any unsafe row
  unsigned hs[2] = {0u, 0u};
  hipError_t e = hipMalloc(&scal, 256);
  if (e == hipSuccess) e = hipMemsetAsync(scal, 0, 8, s);
  if (e == hipSuccess) {
    // (the norms were computed at creation and stay)
    Timed t("corpus_image_build", s);
    e = launch_screen_prepare(h->shards[0].rows_as<float>(), h->n, h->d, h->dp, ni->cb, padded_dim(PMM_DTYPE_BF16, h->d),
                              nullptr, nullptr, ni->crel, (unsigned *)(ni->crel + h->n), scal, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hs, scal, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (scal) (void)hipFree(scal);
  if (e != hipSuccess || hs[1] != 0u) {
    free_screen_image(ni);
    if (e == hipSuccess) h->screen_never.store(true, std::memory_order_release);
    else (void)hipGetLastError();  // (not an error of the call: it runs unscreened)
    return nullptr;
  }
  memcpy(&ni->max_rel, &hs[0], 4);
  h->screen.store(ni, std::memory_order_release);
  return ni;
}

// A handle serves the one top-k entry of its row type: the others refuse it
// and name that entry.
static int wrong_handle(const pmm_corpus *h) {
  static const char *const kRows[] = {"f32", "f64", "bf16", "int8", "bit"};
  static const char *const kEntry[] = {"pmm_topk_f32_corpus", "pmm_topk_f64_corpus", "pmm_topk_bf16_corpus",
                                       "pmm_topk_i8_corpus", "pmm_topk_bits_corpus"};
  return fail(PMM_ERR_ARG, "the corpus handle holds %s rows: use %s", kRows[h->dtype], kEntry[h->dtype]);
}

// What every ungrouped search (top-k, range) answers on a partitioned handle.
static int partitioned_handle(const pmm_corpus *h) {
  return fail(PMM_ERR_ARG, "the corpus handle is partitioned (pmm_corpus_partition): its index map ascends only "
                           "inside a group, so an ungrouped search would break the tie order; use pmm_topk_%s_grouped",
              h->dtype == PMM_DTYPE_F64 ? "f64" : "f32");
}

// A derived handle's lists leave in the parent's numbering: one launch over
// the m x k device index buffer between the executor and the download.  A
// handle without a map launches nothing.
static int remap_lists(const pmm_corpus *h, uint32_t *idx, int64_t m, int64_t k, hipStream_t s) {
  if (!h->map) return PMM_OK;
  Timed t("remap_index", s);
  HIP_TRY(launch_remap_index(idx, m * k, h->map, h->n, s));
  return PMM_OK;
}

// What both subset creators refuse in a parent.
static int check_subset_parent(const pmm_corpus *p, pmm_corpus **out) {
  if (!out) return fail(PMM_ERR_ARG, "null argument");
  *out = nullptr;
  if (!p) return fail(PMM_ERR_ARG, "null corpus");
  if (p->partitioned())
    return fail(PMM_ERR_ARG, "the parent is a partitioned handle (pmm_corpus_partition): its rows are stored group by "
                             "group, so it has no subsets and no partitions; derive from its parent");
  if (p->map)
    return fail(PMM_ERR_ARG, "the parent is itself a derived handle: compose the selections and derive from its parent");
  if (p->shards.size() != 1)
    return fail(PMM_ERR_UNSUPPORTED, "a device-sharded corpus (%d shards) has no subsets: derive from a handle of one shard",
                (int)p->shards.size());
  if (p->dtype == PMM_DTYPE_I8)
    return fail(PMM_ERR_UNSUPPORTED, "an int8 corpus handle has no subsets and no partitions: pmm_topk_i8_corpus searches "
                                     "all of its rows");
  if (p->dtype == PMM_DTYPE_BITS)
    return fail(PMM_ERR_UNSUPPORTED, "a bit corpus handle has no subsets and no partitions: pmm_topk_bits_corpus searches "
                                     "all of its rows");
  return PMM_OK;
}

// The derived handle of parent p for the s ascending parent rows in `map`
// (device memory the handle takes over, freed here on failure), on the
// current device (p's) and stream st: the rows and the per-row norm arrays
// gathered in one launch, the screen image's rows, residuals and flags in one
// more when p has an image; `flag` is a device word for the gathered flags.
// Synchronises st before it returns.
static int subset_build(const pmm_corpus *p, uint32_t *map, int64_t s, unsigned *flag, hipStream_t st,
                        pmm_corpus **out, bool with_image = true) {
  const CorpusShard &px = p->shards[0];
  pmm_corpus *h = new pmm_corpus();
  h->n = s;
  h->d = p->d;
  h->dp = p->dp;
  h->dtype = p->dtype;
  h->map = map;
  h->shards.resize(1);
  CorpusShard &x = h->shards[0];
  x.device = px.device;
  x.lo = 0;
  x.n = s;
  const RowKind rk = row_kind(p->dtype);
  const size_t row_bytes = (size_t)p->dp * rk.elem;  // a multiple of 128
  hipError_t e = hipMalloc(&x.rows, (size_t)s * row_bytes);
  if (e == hipSuccess) e = hipMalloc(&x.norms, (size_t)s * rk.norm_arrays * rk.norm_elem);
  if (e != hipSuccess) {
    pmm_corpus_destroy(h);
    return fail(PMM_ERR_HIP, "subset allocation failed on device %d: %s", px.device, hipGetErrorString(e));
  }
  {
    Timed t("subset_gather_rows", st);
    e = launch_subset_gather(px.rows, map, s, (int)(row_bytes / 16), x.rows, px.norms, x.norms, rk.norm_arrays,
                             (int)rk.norm_elem, p->n, -1, nullptr, st);
  }
  // The parent's image, read once: its rows gathered too when they fit in
  // half of the free HBM (else, or when an allocation fails, the derived
  // handle starts without one and builds its own on its first screened call).
  // (with_image = false, a partitioned handle: no image is gathered)
  const ScreenImage *pimg =
      (with_image && p->dtype == PMM_DTYPE_F32) ? p->screen.load(std::memory_order_acquire) : nullptr;
  ScreenImage *ni = nullptr;
  unsigned hflag = 0u;
  if (e == hipSuccess && pimg && (ni = alloc_screen_image(s, p->d))) {
    e = hipMemsetAsync(flag, 0, 4, st);
    if (e == hipSuccess) {
      Timed t("subset_gather_image", st);
      e = launch_subset_gather(pimg->cb, map, s, (int)(padded_dim(PMM_DTYPE_BF16, p->d) * 2 / 16), ni->cb, pimg->crel,
                               ni->crel, 2, 4, p->n, 1, flag, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hflag, flag, 4, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    free_screen_image(ni);
    pmm_corpus_destroy(h);
    return fail(PMM_ERR_HIP, "subset gather failed: %s", hipGetErrorString(e));
  }
  if (ni && hflag != 0u) {
    // (a parent with an image has no unsafe row, so this does not happen
    // today; the rule is kept for a parent whose image carries flags)
    free_screen_image(ni);
    h->screen_never.store(true, std::memory_order_release);
  } else if (ni) {
    // the parent's bound holds over a superset of these rows: a larger bound
    // only widens the screen's slack, the screen stays exact
    ni->max_rel = pimg->max_rel;
    h->screen.store(ni, std::memory_order_release);
  }
  *out = h;
  return PMM_OK;
}

// Shard x of a handle under creation, filled from the corpus' host rows `c` on
// the current device (x's) and stream s, and waited for.  f32 and f64: the
// rows padded on their way up, then the norms every call would compute
// (src/metrics.rs:368-379), by the same kernels on the same padded rows --
// bit-identical to the per-call ones.  bf16: the f32 rows only pass through
// `stage` (x.n x d floats of the shard's own; the arena would keep them for
// the thread's lifetime), rounded with the norms of both metrics in one pass.
static int corpus_fill_shard(const pmm_corpus *h, const CorpusShard &x, const void *c, float *stage, hipStream_t s) {
  const int64_t d = h->d, dp = h->dp, n = x.n;
  const size_t elem = h->dtype == PMM_DTYPE_F64 ? 8 : (h->dtype == PMM_DTYPE_I8 || h->dtype == PMM_DTYPE_BITS) ? 1 : 4;  // of the HOST rows
  const void *src = (const char *)c + (size_t)x.lo * d * elem;
  hipError_t e1, e2;
  if (h->dtype == PMM_DTYPE_BF16) {
    float *nm = (float *)x.norms;
    {
      Timed t("h2d", s);
      e1 = hipMemcpyAsync(stage, src, (size_t)n * d * 4, hipMemcpyHostToDevice, s);
    }
    Timed t("round_norms_bf16", s);
    e2 = launch_round_norms_bf16(stage, n, d, d, (uint16_t *)x.rows, dp, nm, nm + n, nm + 2 * n, nm + 3 * n, s);
  } else {
    if (int rc = upload_padded(x.rows, src, n, d, dp, elem, s)) return rc;
    if (h->dtype == PMM_DTYPE_I8) {
      Timed t("norms_i8", s);
      e1 = launch_i8_norms(x.rows_as<int8_t>(), n, dp, (int)dp, (uint32_t *)x.norms, (float *)x.norms + n, s);
      e2 = hipSuccess;
    } else if (h->dtype == PMM_DTYPE_BITS) {
      Timed t("bits_popcount", s);
      e1 = launch_bits_popcount(x.rows_as<uint8_t>(), n, dp, (int)dp, (uint32_t *)x.norms, s);
      e2 = hipSuccess;
    } else if (h->dtype == PMM_DTYPE_F64) {
      double *nm = (double *)x.norms;
      e1 = launch_norms_f64(x.rows_as<double>(), n, d, dp, 0, nm, s);
      e2 = launch_norms_f64(x.rows_as<double>(), n, d, dp, 1, nm + n, s);
    } else {
      float *nm = (float *)x.norms;
      e1 = launch_norms_f32(x.rows_as<float>(), n, d, dp, 0, nm, nm + n, s);
      e2 = launch_norms_f32(x.rows_as<float>(), n, d, dp, 1, nm + 2 * n, nm + 3 * n, s);
    }
  }
  const hipError_t e3 = hipStreamSynchronize(s);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
    return fail(PMM_ERR_HIP, h->dtype == PMM_DTYPE_BF16 ? "corpus rounding failed" : "corpus norms failed");
  return PMM_OK;
}

// The creator behind pmm_corpus_create_f32 / _f64 / _bf16 (c: f32 host rows
// for bf16).  With a device list the rows are sharded over it: one contiguous
// shard per listed device, at most n.
static int corpus_create(int dtype, const void *c, int64_t n, int64_t d, pmm_corpus **out, bool one_device = false) {
  if (!out) return fail(PMM_ERR_ARG, "null argument");
  *out = nullptr;
  int rc = validate_sizes(0, n, d, 0, false);
  if (rc) return rc;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if (d == 0) return fail(PMM_ERR_ARG, "Zero-dimensional vectors");
  if (!c) return fail(PMM_ERR_ARG, "null argument");
  int dev;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, list_root()))) return rc;
  if (dtype == PMM_DTYPE_I8 && (rc = validate_i8(0, n, d, 0, kMetricDot))) return rc;  // (the dimension limit)
  if (dtype == PMM_DTYPE_BITS && (rc = validate_bits(0, n, d, 0))) return rc;          // (the width limit)
  std::vector<int> devs = devices_snapshot();
  // (an int8, bit or multi-vector handle is not sharded: it lives on the list's first device)
  if (devs.size() <= 1 || dtype == PMM_DTYPE_I8 || dtype == PMM_DTYPE_BITS || one_device) devs.assign(1, dev);
  const int G = (int)std::min<int64_t>((int64_t)devs.size(), n);
  const RowKind rk = row_kind(dtype);
  pmm_corpus *h = new pmm_corpus();
  h->n = n;
  h->d = d;
  h->dp = padded_dim(dtype, d);  // the stride rule of the row type's device entry
  h->dtype = dtype;
  h->shards.resize(G);
  for (int g = 0; g < G; g++) {
    CorpusShard &x = h->shards[g];
    x.device = devs[g];
    x.lo = shard_lo(n, G, g);
    x.n = shard_lo(n, G, g + 1) - x.lo;
  }
  for (int g = 0; g < G && rc == PMM_OK; g++) {
    CorpusShard &x = h->shards[g];
    hipStream_t s = nullptr;
    float *stage = nullptr;
    hipError_t e = hipSetDevice(x.device);
    if (e == hipSuccess) rc = thread_stream(x.device, &s);
    if (rc) break;
    if (e == hipSuccess) e = hipMalloc(&x.rows, (size_t)x.n * h->dp * rk.elem);
    if (e == hipSuccess) e = hipMalloc(&x.norms, (size_t)x.n * rk.norm_arrays * rk.norm_elem);
    if (e == hipSuccess && dtype == PMM_DTYPE_BF16) e = hipMalloc(&stage, (size_t)x.n * d * 4);
    if (e != hipSuccess)
      rc = fail(PMM_ERR_HIP, "corpus allocation failed on device %d: %s", x.device, hipGetErrorString(e));
    else
      rc = corpus_fill_shard(h, x, c, stage, s);
    if (stage) (void)hipFree(stage);
  }
  (void)hipSetDevice(dev);
  if (rc) {
    pmm_corpus_destroy(h);
    return rc;
  }
  *out = h;
  return PMM_OK;
}

// ---------------------------------------------------------------------------
// The frame of a host top-k call on one device, the same for every row type
// and for host rows and handles: the device (the handle's, else the device
// list's root or the thread's choice) and this thread's stream on it; one arena
// of [uploaded q | uploaded c | the entry's own regions | index list | score
// list | workspace]; the zero-padded upload of the operands that are host rows;
// the entry's executor; a derived handle's index remap; the download and the
// call's one synchronisation.  An entry supplies what differs:
//   plan(f, L) -> workspace bytes: decides the route on f.dev (f.s is set:
//     the f32 handle may build its screen image) and takes the entry's own
//     regions from L (bf16's staging rows, rounded rows and query norms);
//   run(f): fills those regions and calls the executor, which leaves the lists
//     in f.oi / f.os.
// ---------------------------------------------------------------------------
struct HostRows {  // rows x d host elements, uploaded at row stride dp (src nullptr: no operand of the frame's)
  const void *src = nullptr;
  int64_t rows = 0, d = 0, dp = 0;
  size_t elem = 0;
};
template <typename Score>
struct HostCall {
  int dev = 0;
  hipStream_t s = nullptr;
  char *b = nullptr;                // the arena
  char *q = nullptr, *c = nullptr;  // the uploaded operands
  uint32_t *oi = nullptr;
  Score *os = nullptr;
  char *w = nullptr;
  size_t ws_bytes = 0;
};
template <typename Score, typename PlanFn, typename RunFn>
static int host_topk(const pmm_corpus *h, const HostRows &qr, const HostRows &cr, int64_t m, int64_t k,
                     uint32_t *out_idx, Score *out_score, PlanFn plan, RunFn run) {
  HostCall<Score> f;
  DevScope scope;
  int rc = ensure_device(&f.dev, &scope, h ? h->shards[0].device : list_root());
  if (rc) return rc;
  if ((rc = thread_stream(f.dev, &f.s))) return rc;
  Layout L;
  const size_t off_q = L.take(qr.src ? (size_t)qr.rows * qr.dp * qr.elem : 0);
  const size_t off_c = L.take(cr.src ? (size_t)cr.rows * cr.dp * cr.elem : 0);
  f.ws_bytes = plan(f, L);
  const size_t off_i = L.take((size_t)m * k * 4), off_s = L.take((size_t)m * k * sizeof(Score));
  void *base;
  if ((rc = arena(f.dev, f.s, L.off + f.ws_bytes, &base))) return rc;
  f.b = (char *)base;
  f.q = f.b + off_q;
  f.c = f.b + off_c;
  f.oi = (uint32_t *)(f.b + off_i);
  f.os = (Score *)(f.b + off_s);
  f.w = f.b + L.off;
  if (qr.src && (rc = upload_padded(f.q, qr.src, qr.rows, qr.d, qr.dp, qr.elem, f.s))) return rc;
  if (cr.src && (rc = upload_padded(f.c, cr.src, cr.rows, cr.d, cr.dp, cr.elem, f.s))) return rc;
  if ((rc = run(f))) return rc;
  if (h && (rc = remap_lists(h, f.oi, m, k, f.s))) return rc;
  return download_lists(out_idx, out_score, f.oi, f.os, m, k, f.s);
}

// The call path of the four pmm_topk_*_corpus entries, Row the type of the
// queries and Score that of the scores.  A sharded handle goes to the sharded
// search on its resident shards; a handle of one shard through host_topk with
// the entry's plan and run.  The queries go up padded to the handle's stride;
// a bf16 handle's as they are (f32 staging rows, which its entry rounds).
template <typename Row, typename Score, typename PlanFn, typename RunFn>
static int corpus_topk(const pmm_corpus *h, int dtype, const Row *q, int64_t m, int64_t k, int metric,
                       uint32_t *out_idx, Score *out_score, PlanFn plan, RunFn run) {
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (h->partitioned()) return partitioned_handle(h);
  if (h->dtype != dtype) return wrong_handle(h);
  int rc = dtype == PMM_DTYPE_I8     ? validate_i8(m, h->n, h->d, k, metric)
           : dtype == PMM_DTYPE_BITS ? validate_bits(m, h->n, h->d, k)
                                     : validate_sizes(m, h->n, h->d, k, true);
  if (rc) return rc;
  if ((rc = check_metric(metric))) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if ((rc = need_buffers(q, out_idx, out_score))) return rc;
  if constexpr (!std::is_same<Row, int8_t>::value && !std::is_same<Row, uint8_t>::value) {  // (an int8 or bit handle has one shard)
    if (h->shards.size() > 1) {
      // (the f32 and bf16 shards run the fused top-k only; f64 has a path for every k)
      if (dtype != PMM_DTYPE_F64 && k > kFusedMaxK)
        return fail(PMM_ERR_UNSUPPORTED, "a device-sharded corpus supports k <= %d (got %lld)", kFusedMaxK,
                    (long long)k);
      std::vector<ShardSrc> sh(h->shards.size());
      for (size_t g = 0; g < sh.size(); g++) {
        const CorpusShard &x = h->shards[g];
        sh[g] = ShardSrc{x.device, x.lo, x.n, nullptr, x.rows, shard_norms<Score>(h, x, metric)};
      }
      return topk_sharded(dtype, q, m, h->d, k, metric, sh, out_idx, out_score);
    }
  }
  const HostRows qr{q, m, h->d, dtype == PMM_DTYPE_BF16 ? h->d : h->dp, sizeof(Row)};
  return host_topk(h, qr, HostRows{}, m, k, out_idx, out_score, plan, run);
}

// The opening of a list-valued entry (grouped, range and self, candidate
// search) on a handle of one shard: the shard's device, this thread's stream
// on it and the device's CU count.  run(body): the part of the entry that
// uploads from the frame's own vectors (or downloads into them) -- a failure
// in it waits for the stream before the frame, and those vectors, go.
struct ShardCall {
  int dev = 0, cus = 0;
  DevScope scope;
  hipStream_t s = nullptr;
  int open(const pmm_corpus *h) {
    if (int rc = ensure_device(&dev, &scope, h->shards[0].device)) return rc;
    if (int rc = thread_stream(dev, &s)) return rc;
    cus = g_dev[dev].cus;
    return PMM_OK;
  }
  template <typename Body>
  int run(Body body) {
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
  }
};

// ---------------------------------------------------------------------------
// Grouped search: every query row is searched inside its own
// group's segment of a partitioned handle.
// ---------------------------------------------------------------------------
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;
// Segments of at most this many rows go to the grouped kernel (one launch for
// all of them), larger ones to the per-pair loop over the existing executors.
// PMM_GROUPED_SEG_MAX overrides it per call.  The largest measured segment at
// which the kernel beats the loop (16 queries per group, d = 768: 1.78 against
// 8.03 ms at 64 groups of 16384 rows, 6.17 against 3.65 ms at 16 groups of
// 65536; tools/measure_grouped.py, profiles/grouped/README.md).
constexpr int64_t kGroupedSegMax = 16384;

// Stable counting sort of the row numbers 0 .. n-1 by label (host only, no
// device): perm = the kept rows group by group, ascending inside a group;
// offsets[g] .. offsets[g + 1] = group g's positions in perm.
static int partition_plan(const uint32_t *labels, int64_t n, int64_t G, uint32_t *perm, int64_t *offsets,
                          int64_t *kept) {
  if (n < 0 || G < 0 || n > (int64_t)UINT32_MAX - 1)
    return fail(PMM_ERR_ARG, "partition sizes out of range (n=%lld G=%lld)", (long long)n, (long long)G);
  if (!offsets || !kept || (n > 0 && (!labels || !perm))) return fail(PMM_ERR_ARG, "null argument");
  for (int64_t g = 0; g <= G; g++) offsets[g] = 0;
  for (int64_t i = 0; i < n; i++) {
    const uint32_t l = labels[i];
    if (l == kNoGroup) continue;
    if ((int64_t)l >= G)
      return fail(PMM_ERR_ARG, "labels[%lld] = %u is not a group (G=%lld) and not the none label 0xFFFFFFFF",
                  (long long)i, l, (long long)G);
    offsets[l + 1]++;
  }
  for (int64_t g = 0; g < G; g++) offsets[g + 1] += offsets[g];
  *kept = offsets[G];
  std::vector<int64_t> next(offsets, offsets + G);
  for (int64_t i = 0; i < n; i++)
    if (labels[i] != kNoGroup) perm[next[labels[i]]++] = (uint32_t)i;
  return PMM_OK;
}

// One (query range, segment range) pair of a grouped call: rows [q0, q0 + mq)
// of the label-grouped queries against partition rows [c0, c0 + ng).
struct GroupedPair {
  int64_t q0, mq, c0, ng;
  bool kernel;
};

template <typename Score>
static int topk_grouped(const pmm_corpus *h, const Score *q, int64_t m, const uint32_t *qlabels, int64_t k,
                        int metric, uint32_t *out_idx, Score *out_score, uint32_t *out_len) {
  constexpr bool f64 = std::is_same<Score, double>::value;
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (!h->partitioned())
    return fail(PMM_ERR_ARG, "the corpus handle is not partitioned: pmm_corpus_partition derives one");
  if (h->dtype == PMM_DTYPE_BF16)
    return fail(PMM_ERR_UNSUPPORTED, "a bf16 handle has no grouped entry: search it per label (pmm_corpus_subset_*)");
  if (h->dtype != (f64 ? PMM_DTYPE_F64 : PMM_DTYPE_F32))
    return fail(PMM_ERR_ARG, "the partitioned handle holds %s rows: use pmm_topk_%s_grouped", f64 ? "f32" : "f64",
                f64 ? "f32" : "f64");
  int rc = validate_sizes(m, h->n, h->d, 0, false);
  if (rc) return rc;
  if (k < 0 || k > INT32_MAX) return fail(PMM_ERR_ARG, "k must be in [0, 2^31) (got %lld)", (long long)k);
  if ((rc = check_metric(metric))) return rc;
  if (m == 0) return PMM_OK;
  if ((rc = need_buffers(q, qlabels, out_len))) return rc;
  if (k > 0 && (rc = need_buffers(out_idx, out_score))) return rc;
  const int64_t G = (int64_t)h->offsets.size() - 1, d = h->d, dp = h->dp;
  const std::vector<int64_t> &off = h->offsets;
  // The queries grouped by label on the host: a label with no corpus rows
  // counts as the none label (an empty list), so every kept query has a pair.
  std::vector<uint32_t> eff((size_t)m), qperm((size_t)m);
  for (int64_t i = 0; i < m; i++) {
    const uint32_t l = qlabels[i];
    if (l != kNoGroup && (int64_t)l >= G)
      return fail(PMM_ERR_ARG, "qlabels[%lld] = %u is not a group (G=%lld) and not the none label 0xFFFFFFFF",
                  (long long)i, l, (long long)G);
    eff[i] = (l == kNoGroup || off[l + 1] == off[l]) ? kNoGroup : l;
  }
  std::vector<int64_t> qoff((size_t)G + 1);
  int64_t mk = 0;
  if ((rc = partition_plan(eff.data(), m, G, qperm.data(), qoff.data(), &mk))) return rc;
  if (k == 0 || mk == 0) {  // nothing to search: empty lists, no device work
    for (int64_t i = 0; i < m; i++) out_len[i] = 0u;
    for (int64_t t = 0; t < m * k; t++) {
      out_idx[t] = kNoGroup;
      out_score[t] = (Score)0;
    }
    return PMM_OK;
  }
  // Dispatch (PMM_GROUPED, PMM_GROUPED_SEG_MAX: read per call).
  const char *ge = getenv("PMM_GROUPED");
  const bool force_kernel = ge && !strcmp(ge, "kernel"), force_loop = ge && !strcmp(ge, "loop");
  int64_t seg_max = kGroupedSegMax;
  if (const char *se = getenv("PMM_GROUPED_SEG_MAX")) seg_max = atoll(se);
  const bool kernel_ok = !f64 && k <= kGroupedMaxK && dp <= kGroupedMaxDp && !force_loop;
  std::vector<GroupedPair> pairs;
  std::vector<GroupedUnit> units;
  std::vector<uint32_t> glen((size_t)mk);
  for (int64_t g = 0; g < G; g++) {
    if (qoff[g + 1] == qoff[g]) continue;
    GroupedPair p{qoff[g], qoff[g + 1] - qoff[g], off[g], off[g + 1] - off[g], false};
    p.kernel = kernel_ok && (force_kernel || p.ng <= seg_max);
    pairs.push_back(p);
    for (int64_t i = 0; i < p.mq; i++) glen[p.q0 + i] = (uint32_t)std::min<int64_t>(k, p.ng);
    if (p.kernel)
      for (int64_t r0 = 0; r0 < p.mq; r0 += kGroupedRows)
        units.push_back(GroupedUnit{(uint32_t)p.c0, (uint32_t)p.ng, (uint32_t)(p.q0 + r0),
                                    (uint32_t)std::min<int64_t>(kGroupedRows, p.mq - r0)});
  }
  const CorpusShard &x = h->shards[0];
  ShardCall f;
  if ((rc = f.open(h))) return rc;
  const int dev = f.dev, cus = f.cus;
  const hipStream_t s = f.s;
  // The loop pairs' routes and the largest workspace and short-list staging among them.
  std::vector<TopkRoute> routes;
  size_t ws_need = 0, tmp_entries = 0;
  for (const GroupedPair &p : pairs) {
    if (p.kernel) continue;
    const int64_t kg = std::min<int64_t>(k, p.ng);
    if constexpr (f64) {
      ws_need = std::max(ws_need, f64_workspace_bytes(p.mq, p.ng, kg, f64_use_fused(p.mq, p.ng, kg)));
    } else {
      routes.push_back(route_topk(p.mq, p.ng, d, kg, metric, PMM_COMPUTE_F32, cus, false, false));
      ws_need = std::max(ws_need, routes.back().total);
    }
    if (kg < k) tmp_entries = std::max(tmp_entries, (size_t)(p.mq * kg));
  }
  constexpr size_t E = sizeof(Score);
  const size_t tab_words = (size_t)2 * mk + units.size() * 4;
  const size_t off_qu = 0, off_qg = al256((size_t)m * dp * E), off_qn = off_qg + al256((size_t)mk * dp * E);
  const size_t off_tab = off_qn + al256((size_t)mk * 4), off_gi = off_tab + al256(tab_words * 4);
  const size_t off_gs = off_gi + al256((size_t)mk * k * 4), off_oi = off_gs + al256((size_t)mk * k * E);
  const size_t off_os = off_oi + al256((size_t)m * k * 4), off_ol = off_os + al256((size_t)m * k * E);
  const size_t off_ti = off_ol + al256((size_t)m * 4), off_ts = off_ti + al256(tmp_entries * 4);
  const size_t off_w = off_ts + al256(tmp_entries * E);
  void *base;
  if ((rc = arena(dev, s, off_w + ws_need, &base))) return rc;
  char *b = (char *)base;
  const Score *qg = (const Score *)(b + off_qg);
  float *qn = (float *)(b + off_qn);
  uint32_t *tab = (uint32_t *)(b + off_tab);
  const uint32_t *d_qperm = tab, *d_glen = tab + mk;
  const GroupedUnit *d_units = (const GroupedUnit *)(tab + 2 * mk);
  uint32_t *gi = (uint32_t *)(b + off_gi), *oi = (uint32_t *)(b + off_oi), *ol = (uint32_t *)(b + off_ol);
  uint32_t *ti = (uint32_t *)(b + off_ti);
  Score *gs = (Score *)(b + off_gs), *os = (Score *)(b + off_os), *ts = (Score *)(b + off_ts);
  // the queries, once; the tables; the padding every list starts from
  if ((rc = upload_padded(b + off_qu, q, m, d, dp, E, s))) return rc;
  std::vector<uint32_t> htab(tab_words);
  memcpy(htab.data(), qperm.data(), (size_t)mk * 4);
  memcpy(htab.data() + mk, glen.data(), (size_t)mk * 4);
  if (!units.empty()) memcpy(htab.data() + 2 * mk, units.data(), units.size() * sizeof(GroupedUnit));
  // (from here on a failure waits for the stream: the uploads read this frame's vectors)
  return f.run([&]() -> int {
    {
      Timed t("h2d", s);
      HIP_TRY(hipMemcpyAsync(tab, htab.data(), tab_words * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(oi, 0xFF, (size_t)m * k * 4, s));
    HIP_TRY(hipMemsetAsync(os, 0, (size_t)m * k * E, s));
    HIP_TRY(hipMemsetAsync(ol, 0, (size_t)m * 4, s));
    {
      Timed t("grouped_gather_queries", s);
      HIP_TRY(launch_gather_rows(b + off_qu, (int64_t)(dp * E / 16), (const int *)d_qperm, (int)mk, (int)(dp * E / 16),
                                 b + off_qg, s));
    }
    if constexpr (!f64) {
      // (the kernel's query norms, and the sign-of-zero pass's; the loop's
      // executors compute their own, the same values)
      if (metric != kMetricDot && (!units.empty() || metric == kMetricCosine)) {
        Timed t("norms_f32", s);
        HIP_TRY(launch_norms_f32((const float *)qg, mk, d, dp, metric == kMetricEuclidean, qn, nullptr, s));
      }
    }
    // the loop path: the existing executor on each pair's slices, one after another
    size_t ri = 0;
    for (const GroupedPair &p : pairs) {
      if (p.kernel) continue;
      const int64_t kg = std::min<int64_t>(k, p.ng);
      uint32_t *di = kg == k ? gi + p.q0 * k : ti;
      Score *ds = kg == k ? gs + p.q0 * k : ts;
      if constexpr (f64) {
        const double *cn = shard_norms<double>(h, x, metric);
        if (int r2 = topk_f64_device_impl(qg + p.q0 * dp, dp, p.mq, x.rows_as<double>() + p.c0 * dp, dp, p.ng, d, kg,
                                          metric, (uint32_t)p.c0, di, ds, b + off_w, s,
                                          f64_use_fused(p.mq, p.ng, kg), cn ? cn + p.c0 : nullptr))
          return r2;
      } else {
        const float *cn = shard_norms<float>(h, x, metric);  // [norms n | pre-filter factors n]
        if (int r2 = topk_f32_device_impl(routes[ri++], qg + p.q0 * dp, dp, p.mq, x.rows_as<float>() + p.c0 * dp, dp,
                                          p.ng, d, kg, metric, (uint32_t)p.c0, di, ds, b + off_w, ws_need, s, dev,
                                          cn ? cn + p.c0 : nullptr, false, nullptr, cn ? cn + h->n + p.c0 : nullptr))
          return r2;
      }
      if (kg < k) {
        Timed t("grouped_pad", s);
        HIP_TRY(launch_grouped_pad(di, ds, (int)p.mq, (int)kg, (int)k, gi + p.q0 * k, gs + p.q0 * k, f64, s));
      }
    }
    if constexpr (!f64) {
      if (!units.empty()) {
        GroupedArgs a{};
        a.q = (const float *)qg;
        a.c = x.rows_as<float>();
        a.qn = qn;
        a.cn = shard_norms<float>(h, x, metric);
        a.ldq = dp;
        a.ldc = dp;
        a.dp = (int)dp;
        a.k = (int)k;
        a.units = d_units;
        a.out_idx = gi;
        a.out_score = (float *)gs;
        Timed t("grouped_topk_f32", s);
        HIP_TRY(launch_grouped_topk_f32(a, (int)units.size(), metric, s));
      }
      // the sign of zero scores, while the lists still number the partition's rows
      // (cosine and dot; the loop pairs' executors have restored theirs already)
      HIP_TRY(launch_zero_sign_f32((const float *)qg, dp, x.rows_as<float>(), dp, qn, shard_norms<float>(h, x, metric),
                                   (int)mk, h->n, (int)d, (int)k, metric, 0u, gi, (float *)gs, s));
    }
    {
      Timed t("grouped_scatter", s);
      HIP_TRY(launch_grouped_scatter(gi, gs, d_qperm, d_glen, mk, (int)k, h->map, (uint32_t)h->n, oi, os, ol, f64, s));
    }
    {
      Timed t("d2h", s);
      HIP_TRY(hipMemcpyAsync(out_len, ol, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    }
    return download_lists(out_idx, out_score, oi, os, m, k, s);
  });
}

// ---------------------------------------------------------------------------
// Probed search: every query row is searched inside the union
// of several groups' segments -- IVF with nprobe lists, a document visible to
// several tenants.  The plan turns (query row, probe list) into label-sorted
// slots; the grouped kernel's row-table variant (or the loop's executors)
// writes one exact list per slot; probe_merge_f32_kernel keeps each row's best
// k under the parent's row order.
// ---------------------------------------------------------------------------
// The plan (host only, no device).  Row i's labels are probe_labels[
// probe_offsets[i] .. probe_offsets[i + 1]); kNoGroup entries and labels of
// empty segments are skipped and a repeated label counts once.  The kept
// (row, label) slots leave stably sorted by label (ascending row inside a
// label): slot_row / slot_label; row i's slot numbers, ascending by label (and
// so ascending), are row_slots[row_offsets[i] .. row_offsets[i + 1]);
// out_len[i] = min(k, rows of the row's segments); *slots = row_offsets[m].
static int probe_plan(const int64_t *po, const uint32_t *pl, int64_t m, const int64_t *goff, int64_t G, int64_t k,
                      uint32_t *slot_row, uint32_t *slot_label, int64_t *row_offsets, uint32_t *row_slots,
                      uint32_t *out_len, int64_t *slots) {
  if (m < 0 || G < 0 || m > (int64_t)UINT32_MAX - 1 || G > (int64_t)UINT32_MAX - 1)
    return fail(PMM_ERR_ARG, "probe sizes out of range (m=%lld G=%lld)", (long long)m, (long long)G);
  if (k < 0 || k > INT32_MAX) return fail(PMM_ERR_ARG, "k must be in [0, 2^31) (got %lld)", (long long)k);
  if (!po || !goff || !row_offsets || !slots || (m > 0 && !out_len)) return fail(PMM_ERR_ARG, "null argument");
  if (po[0] != 0) return fail(PMM_ERR_ARG, "probe_offsets[0] must be 0 (got %lld)", (long long)po[0]);
  for (int64_t i = 0; i < m; i++)
    if (po[i + 1] < po[i])
      return fail(PMM_ERR_ARG, "probe_offsets must not decrease (row %lld: %lld after %lld)", (long long)i,
                  (long long)po[i + 1], (long long)po[i]);
  const int64_t cap = po[m];
  if (cap > 0 && (!pl || !slot_row || !slot_label || !row_slots)) return fail(PMM_ERR_ARG, "null argument");
  // pass one: every row's kept labels, ascending and distinct, packed into row_slots for now
  row_offsets[0] = 0;
  for (int64_t i = 0; i < m; i++) {
    uint32_t *kept = row_slots + row_offsets[i];
    int64_t nk = 0;
    for (int64_t e = po[i]; e < po[i + 1]; e++) {
      const uint32_t l = pl[e];
      if (l == kNoGroup) continue;
      if ((int64_t)l >= G)
        return fail(PMM_ERR_ARG,
                    "probe_labels[%lld] = %u (query row %lld) is not a group (G=%lld) and not the none label 0xFFFFFFFF",
                    (long long)e, l, (long long)i, (long long)G);
      if (goff[l + 1] > goff[l]) kept[nk++] = l;
    }
    std::sort(kept, kept + nk);
    nk = std::unique(kept, kept + nk) - kept;
    int64_t rows = 0;
    for (int64_t j = 0; j < nk; j++) rows += goff[kept[j] + 1] - goff[kept[j]];
    out_len[i] = (uint32_t)std::min(k, rows);
    row_offsets[i + 1] = row_offsets[i] + nk;
  }
  const int64_t S = row_offsets[m];
  *slots = S;
  if (S > 0 && k > 0 && S > ((int64_t)1 << 31) / k)
    return fail(PMM_ERR_UNSUPPORTED,
                "%lld (query row, group) lists of k=%lld entries pass 2^31 entries: split the call into fewer query rows",
                (long long)S, (long long)k);
  // pass two: the stable counting sort of the slots by label
  std::vector<int64_t> next((size_t)G + 1, 0);
  for (int64_t e = 0; e < S; e++) next[row_slots[e] + 1]++;
  for (int64_t g = 0; g < G; g++) next[g + 1] += next[g];
  for (int64_t i = 0; i < m; i++)
    for (int64_t e = row_offsets[i]; e < row_offsets[i + 1]; e++) {
      const uint32_t l = row_slots[e];
      const int64_t sl = next[l]++;
      slot_row[sl] = (uint32_t)i;
      slot_label[sl] = l;
      row_slots[e] = (uint32_t)sl;
    }
  return PMM_OK;
}

static int topk_probed(const pmm_corpus *h, const float *q, int64_t m, const int64_t *po, const uint32_t *pl,
                       int64_t k, int metric, uint32_t *out_idx, float *out_score, uint32_t *out_len) {
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (!h->partitioned())
    return fail(PMM_ERR_ARG, "the corpus handle is not partitioned: pmm_corpus_partition derives one");
  if (h->dtype != PMM_DTYPE_F32)
    return fail(PMM_ERR_UNSUPPORTED, "probed search runs on f32 handles: search a %s corpus per label and merge",
                h->dtype == PMM_DTYPE_BF16 ? "bf16" : "f64");
  int rc = validate_sizes(m, h->n, h->d, 0, false);
  if (rc) return rc;
  if (k < 0 || k > INT32_MAX) return fail(PMM_ERR_ARG, "k must be in [0, 2^31) (got %lld)", (long long)k);
  if (k > kGroupedMaxK)
    return fail(PMM_ERR_UNSUPPORTED, "probed search supports k <= %d (got %lld)", kGroupedMaxK, (long long)k);
  if ((rc = check_metric(metric))) return rc;
  if (m == 0) return PMM_OK;
  if ((rc = need_buffers(q, po, out_len))) return rc;
  if (k > 0 && (rc = need_buffers(out_idx, out_score))) return rc;
  const int64_t G = (int64_t)h->offsets.size() - 1, d = h->d, dp = h->dp;
  const std::vector<int64_t> &off = h->offsets;
  if (po[0] != 0 || po[m] < 0) return fail(PMM_ERR_ARG, "probe_offsets must start at 0 and not decrease");
  const size_t cap = (size_t)po[m];
  std::vector<uint32_t> slot_row(cap), slot_label(cap), row_slots(cap);
  std::vector<int64_t> roff((size_t)m + 1);
  int64_t S = 0;
  if ((rc = probe_plan(po, pl, m, off.data(), G, k, slot_row.data(), slot_label.data(), roff.data(),
                       row_slots.data(), out_len, &S)))
    return rc;
  if (k == 0 || S == 0) {  // nothing to search: empty lists, no device work
    for (int64_t t = 0; t < m * k; t++) {
      out_idx[t] = kNoGroup;
      out_score[t] = 0.0f;
    }
    return PMM_OK;
  }
  // Dispatch as the grouped entry's (PMM_GROUPED, PMM_GROUPED_SEG_MAX: read per call).
  const char *ge = getenv("PMM_GROUPED");
  const bool force_kernel = ge && !strcmp(ge, "kernel"), force_loop = ge && !strcmp(ge, "loop");
  int64_t seg_max = kGroupedSegMax;
  if (const char *se = getenv("PMM_GROUPED_SEG_MAX")) seg_max = atoll(se);
  const bool kernel_ok = dp <= kGroupedMaxDp && !force_loop;
  std::vector<GroupedPair> pairs;  // (q0, mq: a run of slots with one label)
  std::vector<GroupedUnit> units;
  for (int64_t s0 = 0; s0 < S;) {
    const uint32_t g = slot_label[s0];
    int64_t s1 = s0 + 1;
    while (s1 < S && slot_label[s1] == g) s1++;
    GroupedPair p{s0, s1 - s0, off[g], off[g + 1] - off[g], false};
    p.kernel = kernel_ok && (force_kernel || p.ng <= seg_max);
    pairs.push_back(p);
    if (p.kernel)
      for (int64_t r0 = 0; r0 < p.mq; r0 += kGroupedRows)
        units.push_back(GroupedUnit{(uint32_t)p.c0, (uint32_t)p.ng, (uint32_t)(p.q0 + r0),
                                    (uint32_t)std::min<int64_t>(kGroupedRows, p.mq - r0)});
    s0 = s1;
  }
  const CorpusShard &x = h->shards[0];
  ShardCall f;
  if ((rc = f.open(h))) return rc;
  const int dev = f.dev, cus = f.cus;
  const hipStream_t s = f.s;
  // The loop pairs' routes, the largest workspace, query slice and short-list staging among them.
  std::vector<TopkRoute> routes;
  size_t ws_need = 0, tmp_entries = 0, loop_rows = 0;
  for (const GroupedPair &p : pairs) {
    if (p.kernel) continue;
    const int64_t kg = std::min<int64_t>(k, p.ng);
    routes.push_back(route_topk(p.mq, p.ng, d, kg, metric, PMM_COMPUTE_F32, cus, false, false));
    ws_need = std::max(ws_need, routes.back().total);
    loop_rows = std::max(loop_rows, (size_t)p.mq);
    if (kg < k) tmp_entries = std::max(tmp_entries, (size_t)(p.mq * kg));
  }
  // The workspace (DESIGN.md §4d states this sum): no term in slots * dp.
  const size_t tab_words = units.size() * 4 + (size_t)2 * S + (size_t)m + 1;
  const size_t off_qu = 0, off_qn = al256((size_t)m * dp * 4), off_tab = off_qn + al256((size_t)m * 4);
  const size_t off_gi = off_tab + al256(tab_words * 4), off_gs = off_gi + al256((size_t)S * k * 4);
  const size_t off_oi = off_gs + al256((size_t)S * k * 4), off_os = off_oi + al256((size_t)m * k * 4);
  const size_t off_ol = off_os + al256((size_t)m * k * 4), off_ql = off_ol + al256((size_t)m * 4);
  const size_t off_ti = off_ql + al256(loop_rows * dp * 4), off_ts = off_ti + al256(tmp_entries * 4);
  const size_t off_w = off_ts + al256(tmp_entries * 4);
  void *base;
  if ((rc = arena(dev, s, off_w + ws_need, &base))) return rc;
  char *b = (char *)base;
  const float *qu = (const float *)(b + off_qu);
  float *qn = (float *)(b + off_qn), *ql = (float *)(b + off_ql);
  uint32_t *tab = (uint32_t *)(b + off_tab);
  const GroupedUnit *d_units = (const GroupedUnit *)tab;
  const uint32_t *d_slot_row = tab + units.size() * 4, *d_row_off = d_slot_row + S, *d_row_slots = d_row_off + m + 1;
  uint32_t *gi = (uint32_t *)(b + off_gi), *oi = (uint32_t *)(b + off_oi), *ol = (uint32_t *)(b + off_ol);
  uint32_t *ti = (uint32_t *)(b + off_ti);
  float *gs = (float *)(b + off_gs), *os = (float *)(b + off_os), *ts = (float *)(b + off_ts);
  if ((rc = upload_padded(b + off_qu, q, m, d, dp, 4, s))) return rc;
  std::vector<uint32_t> htab(tab_words);
  {
    uint32_t *t = htab.data();
    if (!units.empty()) memcpy(t, units.data(), units.size() * sizeof(GroupedUnit));
    t += units.size() * 4;
    memcpy(t, slot_row.data(), (size_t)S * 4);
    t += S;
    for (int64_t i = 0; i <= m; i++) t[i] = (uint32_t)roff[i];
    t += m + 1;
    memcpy(t, row_slots.data(), (size_t)S * 4);
  }
  const float *cn = shard_norms<float>(h, x, metric);  // [norms n | pre-filter factors n]
  // (from here on a failure waits for the stream: the upload reads this frame's vector)
  return f.run([&]() -> int {
    {
      Timed t("h2d", s);
      HIP_TRY(hipMemcpyAsync(tab, htab.data(), tab_words * 4, hipMemcpyHostToDevice, s));
    }
    // the query norms, once over the uploaded rows (the kernel's and the
    // sign-of-zero pass's; the loop's executors compute their own, the same values)
    if (metric != kMetricDot && (!units.empty() || metric == kMetricCosine)) {
      Timed t("norms_f32", s);
      HIP_TRY(launch_norms_f32(qu, m, d, dp, metric == kMetricEuclidean, qn, nullptr, s));
    }
    if (!units.empty()) {
      GroupedArgs a{};
      a.q = qu;
      a.c = x.rows_as<float>();
      a.qn = qn;
      a.cn = cn;
      a.ldq = dp;
      a.ldc = dp;
      a.dp = (int)dp;
      a.k = (int)k;
      a.units = d_units;
      a.out_idx = gi;
      a.out_score = gs;
      a.qrow = d_slot_row;
      Timed t("probed_topk_f32", s);
      HIP_TRY(launch_grouped_topk_f32(a, (int)units.size(), metric, s));
    }
    // the loop path: one pair's query rows gathered into a dense slice, the
    // existing executor on it, one pair after another
    size_t ri = 0;
    for (const GroupedPair &p : pairs) {
      if (p.kernel) continue;
      const int64_t kg = std::min<int64_t>(k, p.ng);
      uint32_t *di = kg == k ? gi + p.q0 * k : ti;
      float *ds = kg == k ? gs + p.q0 * k : ts;
      {
        Timed t("probed_gather_queries", s);
        HIP_TRY(launch_gather_rows(qu, (int64_t)(dp / 4), (const int *)(d_slot_row + p.q0), (int)p.mq, (int)(dp / 4),
                                   ql, s));
      }
      if (int r2 = topk_f32_device_impl(routes[ri++], ql, dp, p.mq, x.rows_as<float>() + p.c0 * dp, dp, p.ng, d, kg,
                                        metric, (uint32_t)p.c0, di, ds, b + off_w, ws_need, s, dev,
                                        cn ? cn + p.c0 : nullptr, false, nullptr, cn ? cn + h->n + p.c0 : nullptr))
        return r2;
      if (kg < k) {
        Timed t("grouped_pad", s);
        HIP_TRY(launch_grouped_pad(di, ds, (int)p.mq, (int)kg, (int)k, gi + p.q0 * k, gs + p.q0 * k, false, s));
      }
    }
    // the sign of zero scores, while the lists still number the partition's
    // rows: list s belongs to query row slot_row[s] (cosine and dot; the loop
    // pairs' executors have restored theirs already)
    HIP_TRY(launch_zero_sign_f32(qu, dp, x.rows_as<float>(), dp, qn, cn, (int)S, h->n, (int)d, (int)k, metric, 0u, gi,
                                 gs, s, d_slot_row));
    {
      ProbeMergeArgs a{};
      a.in_idx = gi;
      a.in_score = gs;
      a.row_off = d_row_off;
      a.row_slots = d_row_slots;
      a.map = h->map;
      a.n = (uint32_t)h->n;
      a.m = (int)m;
      a.k = (int)k;
      a.out_idx = oi;
      a.out_score = os;
      a.out_len = ol;
      Timed t("probe_merge", s);
      HIP_TRY(launch_probe_merge_f32(a, metric, s));
    }
    {
      Timed t("d2h", s);
      HIP_TRY(hipMemcpyAsync(out_len, ol, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    }
    return download_lists(out_idx, out_score, oi, os, m, k, s);
  });
}

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

const char *pmm_version(void) { return kVersion; }

const char *pmm_last_error(void) { return t_err.c_str(); }

int pmm_metric_from_str(const char *s, int *metric) {
  if (!s || !metric) return fail(PMM_ERR_ARG, "null argument");
  std::string l(s);
  for (auto &ch : l) ch = (char)tolower((unsigned char)ch);
  if (l == "cosine") *metric = PMM_METRIC_COSINE;
  else if (l == "dot") *metric = PMM_METRIC_DOT;
  else if (l == "euclidean" || l == "l2") *metric = PMM_METRIC_EUCLIDEAN;
  else return fail(PMM_ERR_ARG, "Unknown metric: '%s'. Supported: cosine, dot, euclidean", s);
  return PMM_OK;
}

int pmm_metric_higher_is_better(int metric) { return metric != PMM_METRIC_EUCLIDEAN; }

int pmm_device_count(int *count) {
  if (!count) return fail(PMM_ERR_ARG, "null argument");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *count = n;
  return PMM_OK;
}

int pmm_device_memory(size_t *free_bytes, size_t *total_bytes) {
  if (!free_bytes || !total_bytes) return fail(PMM_ERR_ARG, "null argument");
  int dev, rc;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, list_root()))) return rc;
  HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
  return PMM_OK;
}

int pmm_set_device(int device) {
  int n = 0;
  pmm_device_count(&n);
  if (device < 0 || device >= n) return fail(PMM_ERR_NODEVICE, "no HIP device %d (%d visible)", device, n);
  HIP_TRY(hipSetDevice(device));
  t_ctx.device = device;
  return PMM_OK;
}

int pmm_host_alloc(size_t bytes, void **out) {
  if (!out) return fail(PMM_ERR_ARG, "null argument");
  *out = nullptr;
  if (bytes == 0) return PMM_OK;
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocPortable));
  return PMM_OK;
}

int pmm_host_free(void *p) {
  if (p) HIP_TRY(hipHostFree(p));
  return PMM_OK;
}

int pmm_set_devices(const int *ids, int n) {
  if (n < 0 || (n > 0 && !ids)) return fail(PMM_ERR_ARG, "bad device list (n=%d)", n);
  int count = 0;
  pmm_device_count(&count);
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= count || ids[i] >= kMaxDevices)
      return fail(PMM_ERR_NODEVICE, "no HIP device %d (%d visible)", ids[i], count);
  for (int i = 0; i < n; i++)
    if (int rc = probe_device(ids[i])) return rc;
  std::lock_guard<std::mutex> lk(g_devs_mu);
  g_devs.assign(ids, ids + n);
  return PMM_OK;
}

int pmm_shard_plan(const int *devs, int G, int64_t m, int64_t n, int64_t d, int64_t k, int metric, int compute,
                   int host_rows, int *plan_of, int *plan_dev, uint64_t *plan_bytes, uint64_t *list_offsets,
                   int *n_plans) {
  if (!devs || G < 1 || !plan_of || !plan_dev || !plan_bytes || !list_offsets || !n_plans)
    return fail(PMM_ERR_ARG, "null argument or empty device list");
  if (m < 1 || n < G || d < 1 || k < 1 || k > kFusedMaxK)
    return fail(PMM_ERR_ARG, "bad sizes (m=%lld n=%lld G=%d d=%lld k=%lld)", (long long)m, (long long)n, G,
                (long long)d, (long long)k);
  static const float kHostTag = 0.0f;  // any non-null host pointer: rows are uploaded
  std::vector<ShardSrc> sh(G);
  for (int g = 0; g < G; g++) {
    const int64_t lo = shard_lo(n, G, g), hi = shard_lo(n, G, g + 1);
    sh[g] = ShardSrc{devs[g], lo, hi - lo, host_rows ? &kHostTag : nullptr, nullptr, nullptr};
  }
  ShardLayout L;
  plan_sharded(compute == PMM_COMPUTE_BF16 ? PMM_DTYPE_BF16 : PMM_DTYPE_F32, sh, m, d, k, metric, L);
  *n_plans = (int)L.dps.size();
  for (int j = 0; j < (int)L.dps.size(); j++) {
    plan_dev[j] = L.dps[j].dev;
    plan_bytes[j] = L.dps[j].total;
  }
  for (int g = 0; g < G; g++) {
    plan_of[g] = L.plan_of[g];
    list_offsets[g] = L.sl[g].off_li;
  }
  return PMM_OK;
}

int pmm_get_devices(int *ids, int cap, int *n) {
  if (!n || cap < 0 || (cap > 0 && !ids)) return fail(PMM_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(g_devs_mu);
  *n = (int)g_devs.size();
  for (int i = 0; i < (int)g_devs.size() && i < cap; i++) ids[i] = g_devs[i];
  return PMM_OK;
}

size_t pmm_topk_workspace_bytes(int64_t m, int64_t n, int64_t d, int64_t k, int metric,
                                int compute) {
  int dev = 0;
  const int cus = hipGetDevice(&dev) == hipSuccess ? device_cus(dev) : 256;
  return route_topk(m, n, d, k, metric, compute, cus, true, true).total;
}

int pmm_topk_merge_bytes(const void *workspace, int64_t m, int64_t n, int64_t d, int64_t k,
                         int metric, int compute, uint64_t *bytes) {
  if (!bytes) return fail(PMM_ERR_ARG, "null output");
  *bytes = 0;
  if (m <= 0 || k <= 0) return PMM_OK;
  if (k > kFusedMaxK)
    return fail(PMM_ERR_UNSUPPORTED, "no merge pass on the materialised path (k > %d)", kFusedMaxK);
  int dev;
  int rc = ensure_device(&dev);
  if (rc) return rc;
  // the counts sit at the offsets of the layout the call used: the route's
  // plan (at `base` behind the widened rows of a bf16 call past the bf16
  // kernels' limits)
  const TopkRoute r = route_topk(m, n, d, k, metric, compute, device_cus(dev), true, true);
  const Plan &p = r.p;
  const size_t base = r.base;
  // screened path: f32 bytes gathered per re-scored candidate
  const uint64_t row_bytes = r.kind == Route::kF32Screened ? (uint64_t)r.sp.dp * 4 : 0;
  // the merge reads every row's split counts and shared threshold, the
  // candidates the GEMM left, and writes the m x k (index, score) lists; the
  // screened path's exact finish also reads and rewrites every candidate the
  // screen kept and gathers its corpus row (and each query row once)
  std::vector<unsigned> cnt((size_t)m * p.segs);
  HIP_TRY(hipMemcpy(cnt.data(), (const char *)workspace + base + p.off_cnt, cnt.size() * 4,
                    hipMemcpyDeviceToHost));
  uint64_t cands = 0;
  for (unsigned c : cnt) cands += std::min<unsigned>(c, (unsigned)p.capg);
  *bytes = (uint64_t)m * p.segs * 4 + cands * 8 + (uint64_t)m * 8 + (uint64_t)m * k * 8;
  if (row_bytes) *bytes += cands * (16 + row_bytes) + (uint64_t)m * (row_bytes + 8 + p.segs * 4);
  return PMM_OK;
}

int pmm_topk_f32_device(const float *q, int64_t ldq, int64_t m, const float *c, int64_t ldc,
                        int64_t n, int64_t d, int64_t k, int metric, int compute,
                        uint32_t index_base, uint32_t *out_idx, float *out_score, void *workspace,
                        size_t workspace_bytes, void *stream) {
  // a corpus shard may hold fewer than k rows: the fused path pads with empty
  // slots (index 0xFFFFFFFF, score NaN), which the shard merge skips
  int rc = validate_sizes(m, n, d, k, true, k <= kFusedMaxK);
  if (rc) return rc;
  if ((rc = check_metric(metric))) return rc;
  if (compute == PMM_COMPUTE_BF16)
    return fail(PMM_ERR_UNSUPPORTED,
                "device f32 inputs with bf16 compute: convert to bf16 and call pmm_topk_bf16_device");
  if (compute != PMM_COMPUTE_F32)
    return fail(PMM_ERR_UNSUPPORTED, "unknown compute mode %d", compute);
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_F32, d);
  if (d == 0 || ldq % 4 != 0 || ldc % 4 != 0 || ldq < dp || ldc < dp || ((uintptr_t)q & 15) ||
      ((uintptr_t)c & 15))
    return fail(PMM_ERR_ARG,
                "device inputs need row strides >= roundup(d, 32) (zero-padded), multiples of 4, "
                "16-byte-aligned bases (d=%lld ldq=%lld ldc=%lld)",
                (long long)d, (long long)ldq, (long long)ldc);
  if ((rc = check_row_stride("ldq", ldq, 4)) || (rc = check_row_stride("ldc", ldc, 4))) return rc;
  int dev;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;  // NULL = the HIP default stream
  return topk_f32_device_impl(route_topk(m, n, d, k, metric, compute, g_dev[dev].cus, true, true), q, ldq, m, c, ldc,
                              n, d, k, metric, index_base, out_idx, out_score, workspace, workspace_bytes, s, dev);
}

int pmm_topk_f32_ex(const float *q, int64_t m, const float *c, int64_t n, int64_t d, int64_t k,
                    int metric, int compute, uint32_t *out_idx, float *out_score) {
  int rc = validate_sizes(m, n, d, k, true);
  if (rc) return rc;
  if ((rc = check_metric(metric))) return rc;
  if (compute != PMM_COMPUTE_F32 && compute != PMM_COMPUTE_BF16)
    return fail(PMM_ERR_UNSUPPORTED, "unknown compute mode %d", compute);
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if (d == 0) return fail(PMM_ERR_ARG, "Zero-dimensional vectors");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  {
    // a device list (pmm_set_devices): the corpus row-sharded over it, one
    // shard per listed device (at most n shards), results merged on the first
    const std::vector<int> devs = devices_snapshot();
    if (devs.size() > 1 && k <= kFusedMaxK)
      return topk_sharded(compute == PMM_COMPUTE_BF16 ? PMM_DTYPE_BF16 : PMM_DTYPE_F32, q, m, d, k, metric,
                          host_shards(devs, c, n, d, 4), out_idx, out_score);
  }
  TopkRoute route;
  auto plan_route = [&](const HostCall<float> &f) {
    route = route_topk(m, n, d, k, metric, compute, g_dev[f.dev].cus, true, true);
    return route.total;
  };
  if (compute == PMM_COMPUTE_BF16) {
    // f32 rows uploaded as they are, rounded to zero-padded bf16 rows on device
    const int64_t db = padded_dim(PMM_DTYPE_BF16, d);
    size_t off_qf = 0, off_cf = 0, off_qb = 0, off_cb = 0;
    return host_topk(
        nullptr, HostRows{}, HostRows{}, m, k, out_idx, out_score,
        [&](const HostCall<float> &f, Layout &L) {
          off_qf = L.take((size_t)m * d * 4), off_cf = L.take((size_t)n * d * 4);
          off_qb = L.take((size_t)m * db * 2), off_cb = L.take((size_t)n * db * 2);
          return plan_route(f);
        },
        [&](const HostCall<float> &f) -> int {
          uint16_t *qb = (uint16_t *)(f.b + off_qb), *cb = (uint16_t *)(f.b + off_cb);
          HIP_TRY(hipMemcpyAsync(f.b + off_qf, q, (size_t)m * d * 4, hipMemcpyHostToDevice, f.s));
          HIP_TRY(hipMemcpyAsync(f.b + off_cf, c, (size_t)n * d * 4, hipMemcpyHostToDevice, f.s));
          {
            Timed t("f32_to_bf16", f.s);  // (measured against round_norms_bf16, profiles/bf16_corpus)
            HIP_TRY(launch_f32_to_bf16((const float *)(f.b + off_qf), m, d, d, qb, db, f.s));
            HIP_TRY(launch_f32_to_bf16((const float *)(f.b + off_cf), n, d, d, cb, db, f.s));
          }
          return topk_bf16_device_impl(route, qb, db, m, cb, db, n, d, k, metric, 0u, f.oi, f.os, f.w, f.ws_bytes, f.s,
                                       f.dev);
        });
  }
  const int64_t dp = padded_dim(PMM_DTYPE_F32, d);
  {
    const char *ce = getenv("PMM_CHUNKED_UPLOAD");  // 0: one upload, then one launch
    if (k <= kFusedMaxK && (size_t)n * dp * 4 >= kChunkedMinBytes && n >= 64 * k && !(ce && atoi(ce) == 0))
      return topk_f32_host_chunked(q, m, c, n, d, k, metric, out_idx, out_score);
  }
  return host_topk(
      nullptr, HostRows{q, m, d, dp, 4}, HostRows{c, n, d, dp, 4}, m, k, out_idx, out_score,
      [&](const HostCall<float> &f, Layout &) { return plan_route(f); },
      [&](const HostCall<float> &f) {
        return topk_f32_device_impl(route, (const float *)f.q, dp, m, (const float *)f.c, dp, n, d, k, metric, 0u, f.oi,
                                    f.os, f.w, f.ws_bytes, f.s, f.dev);
      });
}

int pmm_topk_bf16_device(const uint16_t *q, int64_t ldq, int64_t m, const uint16_t *c,
                         int64_t ldc, int64_t n, int64_t d, int64_t k, int metric,
                         uint32_t index_base, uint32_t *out_idx, float *out_score,
                         void *workspace, size_t workspace_bytes, void *stream) {
  // (k > n only where the fused path pads short lists, as for f32)
  int rc = validate_sizes(m, n, d, k, true, k <= kFusedMaxK);
  if (rc) return rc;
  if ((rc = check_metric(metric))) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if (d == 0) return fail(PMM_ERR_ARG, "Zero-dimensional vectors");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_BF16, d);
  if (ldq % 8 != 0 || ldc % 8 != 0 || ldq < dp || ldc < dp || ((uintptr_t)q & 15) ||
      ((uintptr_t)c & 15))
    return fail(PMM_ERR_ARG,
                "bf16 device inputs need row strides >= roundup(d, 128) (zero-padded), multiples "
                "of 8, 16-byte-aligned bases (d=%lld ldq=%lld ldc=%lld)",
                (long long)d, (long long)ldq, (long long)ldc);
  if ((rc = check_row_stride("ldq", ldq, 2)) || (rc = check_row_stride("ldc", ldc, 2))) return rc;
  int dev;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;  // NULL = the HIP default stream
  return topk_bf16_device_impl(route_topk(m, n, d, k, metric, PMM_COMPUTE_BF16, g_dev[dev].cus, true, true), q, ldq, m,
                               c, ldc, n, d, k, metric, index_base, out_idx, out_score, workspace, workspace_bytes,
                               s, dev);
}

int pmm_topk_f32(const float *q, int64_t m, const float *c, int64_t n, int64_t d, int64_t k,
                 int metric, uint32_t *out_idx, float *out_score) {
  return pmm_topk_f32_ex(q, m, c, n, d, k, metric, PMM_COMPUTE_F32, out_idx, out_score);
}

int pmm_topk_f64(const double *q, int64_t m, const double *c, int64_t n, int64_t d, int64_t k,
                 int metric, uint32_t *out_idx, double *out_score) {
  int rc = validate_sizes(m, n, d, k, true);
  if (rc) return rc;
  if ((rc = check_metric(metric))) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if (d == 0) return fail(PMM_ERR_ARG, "Zero-dimensional vectors");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  {
    // a device list (pmm_set_devices): the corpus row-sharded over it, as the f32 path does
    const std::vector<int> devs = devices_snapshot();
    if (devs.size() > 1 && n > 1)
      return topk_sharded(PMM_DTYPE_F64, q, m, d, k, metric, host_shards(devs, c, n, d, 8), out_idx, out_score);
  }
  const int64_t dp = padded_dim(PMM_DTYPE_F64, d);
  const bool fused = f64_use_fused(m, n, k);
  return host_topk(
      nullptr, HostRows{q, m, d, dp, 8}, HostRows{c, n, d, dp, 8}, m, k, out_idx, out_score,
      [&](const HostCall<double> &, Layout &) { return f64_workspace_bytes(m, n, k, fused); },
      [&](const HostCall<double> &f) {
        return topk_f64_device_impl((const double *)f.q, dp, m, (const double *)f.c, dp, n, d, k, metric, 0u, f.oi, f.os,
                                    f.w, f.s, fused);
      });
}

int pmm_topk_f64_device(const double *q, int64_t ldq, int64_t m, const double *c, int64_t ldc, int64_t n,
                        int64_t d, int64_t k, int metric, uint32_t index_base, uint32_t *out_idx,
                        double *out_score, void *stream) {
  int rc = validate_sizes(m, n, d, k, true);
  if (rc) return rc;
  if ((rc = check_metric(metric))) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_F64, d);
  // (f64_tile stages the rows with 16-byte loads: every row must start 16-byte aligned)
  if (d == 0 || ldq < dp || ldc < dp || ldq % 2 != 0 || ldc % 2 != 0 || ((uintptr_t)q & 15) || ((uintptr_t)c & 15))
    return fail(PMM_ERR_ARG,
                "device f64 inputs need row strides >= roundup(d, 16) (zero-padded), multiples of 2, and "
                "16-byte-aligned bases (d=%lld ldq=%lld ldc=%lld)",
                (long long)d, (long long)ldq, (long long)ldc);
  int dev;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;
  void *w;
  const bool fused = f64_use_fused(m, n, k);
  if ((rc = arena(dev, s, f64_workspace_bytes(m, n, k, fused), &w))) return rc;
  rc = topk_f64_device_impl(q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score, (char *)w, s, fused);
  if (rc) return rc;
  return arena_record(dev, s);
}

int pmm_matmul_f32(const float *q, int64_t m, const float *c, int64_t n, int64_t d, float *out) {
  int rc = validate_sizes(m, n, d, 0, false);
  if (rc) return rc;
  if (m == 0 || n == 0) return PMM_OK;
  if ((rc = need_buffers(q, c, out))) return rc;
  int dev;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, list_root()))) return rc;
  hipStream_t s;
  if ((rc = thread_stream(dev, &s))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_F32, std::max<int64_t>(d, 1));
  const int64_t rows_chunk =
      std::max<int64_t>(1, std::min<int64_t>(m, (int64_t)(materialise_budget() / ((size_t)n * 4))));
  size_t off_q = 0, off_c = al256((size_t)m * dp * 4), off_o = off_c + al256((size_t)n * dp * 4);
  size_t off_cnt = off_o + al256((size_t)rows_chunk * n * 4);
  void *base;
  if ((rc = arena(dev, s, off_cnt + 256, &base))) return rc;
  char *b = (char *)base;
  if ((rc = upload_padded(b + off_q, q, m, d, dp, 4, s))) return rc;
  if ((rc = upload_padded(b + off_c, c, n, d, dp, 4, s))) return rc;
  const float *dq = (const float *)(b + off_q), *dc = (const float *)(b + off_c);
  float *dout = (float *)(b + off_o);
  HostPin pin(out, (size_t)m * n * 4);
  for (int64_t r0 = 0; r0 < m; r0 += rows_chunk) {
    const int64_t rows = std::min<int64_t>(rows_chunk, m - r0);
    rc = gemm_store_f32(dq + r0 * dp, dp, rows, dc, dp, n, dp, kMetricDot, 0, nullptr, nullptr,
                        dout, n, (unsigned *)(b + off_cnt), g_dev[dev].cus, s);
    if (rc) return rc;
    // (a padded dimension's +0 products turn a -0.0 sum into +0.0: the sign of
    // a zero element from the chain over exactly d elements)
    if (d < dp)
      HIP_TRY(launch_zero_sign_f32(dq + r0 * dp, dp, dc, dp, nullptr, nullptr, (int)rows, n, (int)d, (int)n,
                                   kMetricDot, 0u, nullptr, dout, s));
    HIP_TRY(hipMemcpyAsync(out + r0 * n, dout, (size_t)rows * n * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return PMM_OK;
}

int pmm_matmul_f64(const double *q, int64_t m, const double *c, int64_t n, int64_t d,
                   double *out) {
  int rc = validate_sizes(m, n, d, 0, false);
  if (rc) return rc;
  if (m == 0 || n == 0) return PMM_OK;
  if ((rc = need_buffers(q, c, out))) return rc;
  int dev;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, list_root()))) return rc;
  hipStream_t s;
  if ((rc = thread_stream(dev, &s))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_F64, std::max<int64_t>(d, 1));
  const int64_t rows_chunk =
      std::max<int64_t>(1, std::min<int64_t>(m, (int64_t)(materialise_budget() / ((size_t)n * 8))));
  size_t off_q = 0, off_c = al256((size_t)m * dp * 8), off_o = off_c + al256((size_t)n * dp * 8);
  void *base;
  if ((rc = arena(dev, s, off_o + al256((size_t)rows_chunk * n * 8), &base))) return rc;
  char *b = (char *)base;
  if ((rc = upload_padded(b + off_q, q, m, d, dp, 8, s))) return rc;
  if ((rc = upload_padded(b + off_c, c, n, d, dp, 8, s))) return rc;
  const double *dq = (const double *)(b + off_q), *dc = (const double *)(b + off_c);
  double *dout = (double *)(b + off_o);
  HostPin pin(out, (size_t)m * n * 8);
  for (int64_t r0 = 0; r0 < m; r0 += rows_chunk) {
    const int64_t rows = std::min<int64_t>(rows_chunk, m - r0);
    {
      Timed t("gemm_f64_matmul", s);
      HIP_TRY(launch_gemm_f64_store(dq + r0 * dp, dp, dc, dp, nullptr, nullptr, (int)rows, (int)n,
                                    (int)dp, kMetricDot, 0, dout, n, s));
    }
    if (d < dp)  // (as in pmm_matmul_f32)
      HIP_TRY(launch_zero_sign_f64(dq + r0 * dp, dp, dc, dp, nullptr, nullptr, (int)rows, n, (int)d, (int)n,
                                   kMetricDot, 0u, nullptr, dout, s));
    HIP_TRY(hipMemcpyAsync(out + r0 * n, dout, (size_t)rows * n * 8, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return PMM_OK;
}

int pmm_norms_f32_device(const float *a, int64_t ld, int64_t rows, int64_t d, int squared,
                         float *out, void *stream) {
  if (rows < 0 || d < 0 || ld < d) return fail(PMM_ERR_ARG, "bad norm sizes (rows=%lld d=%lld ld=%lld)",
                                                (long long)rows, (long long)d, (long long)ld);
  if (rows == 0) return PMM_OK;
  int dev, rc;
  if ((rc = ensure_device(&dev))) return rc;
  HIP_TRY(launch_norms_f32(a, rows, d, ld, squared ? 1 : 0, out, nullptr, (hipStream_t)stream));
  return PMM_OK;
}

int pmm_norms_f64_device(const double *a, int64_t ld, int64_t rows, int64_t d, int squared,
                         double *out, void *stream) {
  if (rows < 0 || d < 0 || ld < d) return fail(PMM_ERR_ARG, "bad norm sizes (rows=%lld d=%lld ld=%lld)",
                                                (long long)rows, (long long)d, (long long)ld);
  if (rows == 0) return PMM_OK;
  int dev, rc;
  if ((rc = ensure_device(&dev))) return rc;
  HIP_TRY(launch_norms_f64(a, rows, d, ld, squared ? 1 : 0, out, (hipStream_t)stream));
  return PMM_OK;
}

int pmm_merge_topk_device(const uint32_t *idx, const float *score, int64_t m, int64_t lists,
                          int64_t k_in, int64_t k_out, int metric, uint32_t *out_idx,
                          float *out_score, void *stream) {
  return pmm_merge_topk_strided_device(idx, score, m, lists, k_in, lists * k_in, k_in, k_out, metric,
                                       out_idx, out_score, stream);
}

static int merge_strided(const uint32_t *idx, const float *score, int64_t m, int64_t lists, int64_t k_in,
                         int64_t row_stride, int64_t list_stride, int64_t k_out, int metric, uint32_t *out_idx,
                         float *out_score, void *stream, bool sorted);

int pmm_merge_topk_strided_device(const uint32_t *idx, const float *score, int64_t m,
                                  int64_t lists, int64_t k_in, int64_t row_stride,
                                  int64_t list_stride, int64_t k_out, int metric,
                                  uint32_t *out_idx, float *out_score, void *stream) {
  return merge_strided(idx, score, m, lists, k_in, row_stride, list_stride, k_out, metric, out_idx, out_score,
                       stream, false);
}

int pmm_merge_sorted_topk_strided_device(const uint32_t *idx, const float *score, int64_t m,
                                         int64_t lists, int64_t k_in, int64_t row_stride,
                                         int64_t list_stride, int64_t k_out, int metric,
                                         uint32_t *out_idx, float *out_score, void *stream) {
  return merge_strided(idx, score, m, lists, k_in, row_stride, list_stride, k_out, metric, out_idx, out_score,
                       stream, true);
}

static int merge_strided(const uint32_t *idx, const float *score, int64_t m, int64_t lists, int64_t k_in,
                         int64_t row_stride, int64_t list_stride, int64_t k_out, int metric, uint32_t *out_idx,
                         float *out_score, void *stream, bool sorted) {
  int rc;
  if ((rc = check_metric(metric))) return rc;
  if (m < 0 || lists < 1 || k_in < 0 || k_out < 0 || k_out > lists * k_in || row_stride < 0 ||
      list_stride < 0)
    return fail(PMM_ERR_ARG, "bad merge sizes (m=%lld lists=%lld k_in=%lld k_out=%lld)",
                (long long)m, (long long)lists, (long long)k_in, (long long)k_out);
  if (k_out > kFusedMaxK) return fail(PMM_ERR_UNSUPPORTED, "merge k_out > %d", kFusedMaxK);
  if (m == 0 || k_out == 0) return PMM_OK;
  int dev;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;  // NULL = the HIP default stream
  const MergeArgs ma = merge_lists_args(idx, score, m, lists, k_in, row_stride, list_stride, k_out, metric, sorted,
                                        out_idx, out_score);
  Timed t("merge_shards", s);
  HIP_TRY(launch_merge(ma, 1, s));
  return PMM_OK;
}

int pmm_corpus_create_f32(const float *c, int64_t n, int64_t d, pmm_corpus **out) {
  return corpus_create(PMM_DTYPE_F32, c, n, d, out);
}

int pmm_corpus_destroy(pmm_corpus *h) {
  if (!h) return PMM_OK;
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (auto &x : h->shards) {
    if (!x.rows && !x.norms && !h->map) continue;
    (void)hipSetDevice(x.device);
    (void)hipDeviceSynchronize();
    if (x.rows) (void)hipFree(x.rows);
    if (x.norms) (void)hipFree(x.norms);
    if (&x == &h->shards[0]) {
      free_screen_image(h->screen.exchange(nullptr, std::memory_order_acq_rel));
      if (h->map) (void)hipFree(h->map);
      if (h->d_offsets) (void)hipFree(h->d_offsets);
      if (h->d_doc_offsets) (void)hipFree(h->d_doc_offsets);
    }
  }
  (void)hipSetDevice(cur);
  delete h;
  return PMM_OK;
}

int pmm_corpus_bytes(const pmm_corpus *h, size_t *bytes) {
  if (!h || !bytes) return fail(PMM_ERR_ARG, "null argument");
  const RowKind rk = row_kind(h->dtype);
  size_t b = 0;
  for (const auto &x : h->shards) b += (size_t)x.n * (h->dp * rk.elem + rk.norm_arrays * rk.norm_elem);
  if (h->screen.load(std::memory_order_acquire)) b += screen_image_bytes(h->n, h->d);
  if (h->map) b += (size_t)h->n * 4;
  if (h->d_offsets) b += h->offsets.size() * 8;
  if (h->d_doc_offsets) b += h->doc_offsets.size() * 8;
  *bytes = b;
  return PMM_OK;
}

int pmm_corpus_info(const pmm_corpus *h, int64_t *n, int64_t *d, int *device) {
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (n) *n = h->n;
  if (d) *d = h->d;
  if (device) *device = h->shards.empty() ? -1 : h->shards[0].device;
  return PMM_OK;
}

int pmm_corpus_shards(const pmm_corpus *h, int *shards) {
  if (!h || !shards) return fail(PMM_ERR_ARG, "null argument");
  *shards = (int)h->shards.size();
  return PMM_OK;
}

int pmm_corpus_dtype(const pmm_corpus *h, int *dtype) {
  if (!h || !dtype) return fail(PMM_ERR_ARG, "null argument");
  *dtype = h->dtype;
  return PMM_OK;
}

int pmm_corpus_subset_ids(const pmm_corpus *p, const uint32_t *ids, int64_t s, pmm_corpus **out) {
  int rc = check_subset_parent(p, out);
  if (rc) return rc;
  if (!ids) return fail(PMM_ERR_ARG, "null argument");
  if (s < 1 || s > p->n)
    return fail(PMM_ERR_ARG, "a subset holds 1 <= s <= n rows (s=%lld n=%lld)", (long long)s, (long long)p->n);
  for (int64_t i = 0; i < s; i++) {
    if ((int64_t)ids[i] >= p->n)
      return fail(PMM_ERR_ARG, "ids[%lld] = %u is not a row of the corpus (n=%lld)", (long long)i, ids[i],
                  (long long)p->n);
    if (i > 0 && ids[i] <= ids[i - 1])
      return fail(PMM_ERR_ARG, "ids must be strictly ascending: ids[%lld] = %u follows %u", (long long)i, ids[i],
                  ids[i - 1]);
  }
  int dev;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, p->shards[0].device))) return rc;
  hipStream_t st;
  if ((rc = thread_stream(dev, &st))) return rc;
  void *flag;
  if ((rc = arena(dev, st, 256, &flag))) return rc;
  uint32_t *map = nullptr;
  hipError_t e = hipMalloc(&map, (size_t)s * 4);
  if (e != hipSuccess)
    return fail(PMM_ERR_HIP, "subset allocation failed on device %d: %s", dev, hipGetErrorString(e));
  {
    Timed t("h2d", st);
    e = hipMemcpyAsync(map, ids, (size_t)s * 4, hipMemcpyHostToDevice, st);
  }
  if (e != hipSuccess) {
    (void)hipFree(map);
    return fail(PMM_ERR_HIP, "subset upload failed: %s", hipGetErrorString(e));
  }
  return subset_build(p, map, s, (unsigned *)flag, st, out);
}

int pmm_corpus_subset_mask(const pmm_corpus *p, const uint8_t *bitmap, int64_t bit_offset, pmm_corpus **out) {
  int rc = check_subset_parent(p, out);
  if (rc) return rc;
  if (!bitmap) return fail(PMM_ERR_ARG, "null argument");
  if (bit_offset < 0) return fail(PMM_ERR_ARG, "bit_offset must be >= 0 (got %lld)", (long long)bit_offset);
  const int64_t n = p->n;
  int dev;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, p->shards[0].device))) return rc;
  hipStream_t st;
  if ((rc = thread_stream(dev, &st))) return rc;
  // The bitmap from the byte that holds the first row's bit, as 64-bit words
  // with one zero word behind (a word's rows straddle two when the offset is
  // no multiple of 8), the per-block counts and their exclusive sums.
  const int shift = (int)(bit_offset & 7);
  const size_t in_bytes = (size_t)((shift + n + 7) / 8);
  const int64_t nwords = cdiv(n, 64) + 1, nblk = cdiv(n, kMaskBlockRows);
  const size_t off_w = 256, off_cnt = off_w + al256((size_t)nwords * 8);
  const size_t off_base = off_cnt + al256((size_t)nblk * 4), total = off_base + al256((size_t)(nblk + 1) * 4);
  void *base;
  if ((rc = arena(dev, st, total, &base))) return rc;
  char *b = (char *)base;  // [0, 256): subset_build's flag word
  const unsigned long long *words = (const unsigned long long *)(b + off_w);
  uint32_t *counts = (uint32_t *)(b + off_cnt), *bases = (uint32_t *)(b + off_base);
  uint32_t hs = 0;
  HIP_TRY(hipMemsetAsync(b + off_w, 0, (size_t)nwords * 8, st));
  {
    Timed t("h2d", st);
    HIP_TRY(hipMemcpyAsync(b + off_w, bitmap + (bit_offset >> 3), in_bytes, hipMemcpyHostToDevice, st));
  }
  {
    Timed t("subset_mask_count", st);
    HIP_TRY(launch_mask_count(words, shift, n, counts, st));
    HIP_TRY(launch_mask_scan(counts, nblk, bases, st));
  }
  // the one read-back: the allocations below are sized by the count
  HIP_TRY(hipMemcpyAsync(&hs, bases + nblk, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t s = (int64_t)hs;
  if (s == 0) return fail(PMM_ERR_ARG, "empty selection: no bit of the mask's %lld is set", (long long)n);
  uint32_t *map = nullptr;
  hipError_t e = hipMalloc(&map, (size_t)s * 4);
  if (e != hipSuccess)
    return fail(PMM_ERR_HIP, "subset allocation failed on device %d: %s", dev, hipGetErrorString(e));
  {
    Timed t("subset_mask_write", st);
    e = launch_mask_write(words, shift, n, bases, map, st);
  }
  if (e != hipSuccess) {
    (void)hipFree(map);
    return fail(PMM_ERR_HIP, "subset compaction failed: %s", hipGetErrorString(e));
  }
  return subset_build(p, map, s, (unsigned *)b, st, out);
}

int pmm_corpus_index_map(const pmm_corpus *h, uint32_t *ids, int64_t cap, int64_t *s) {
  if (!h || !s) return fail(PMM_ERR_ARG, "null argument");
  *s = h->map ? h->n : 0;
  const int64_t take = std::min<int64_t>(cap, *s);
  if (take <= 0) return PMM_OK;
  if (!ids) return fail(PMM_ERR_ARG, "null argument");
  int dev, rc;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, h->shards[0].device))) return rc;
  HIP_TRY(hipMemcpy(ids, h->map, (size_t)take * 4, hipMemcpyDeviceToHost));
  return PMM_OK;
}

int pmm_partition_plan(const uint32_t *labels, int64_t n, int64_t G, uint32_t *perm, int64_t *offsets,
                       int64_t *kept) {
  return partition_plan(labels, n, G, perm, offsets, kept);
}

int pmm_corpus_partition(const pmm_corpus *p, const uint32_t *labels, int64_t G, pmm_corpus **out) {
  int rc = check_subset_parent(p, out);
  if (rc) return rc;
  if (!labels) return fail(PMM_ERR_ARG, "null argument");
  if (G < 1) return fail(PMM_ERR_ARG, "a partition has G >= 1 groups (got %lld)", (long long)G);
  std::vector<uint32_t> perm((size_t)p->n);
  std::vector<int64_t> off((size_t)G + 1);
  int64_t kept = 0;
  if ((rc = partition_plan(labels, p->n, G, perm.data(), off.data(), &kept))) return rc;
  if (kept == 0)
    return fail(PMM_ERR_ARG, "empty partition: every one of the %lld rows carries the none label", (long long)p->n);
  int dev;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, p->shards[0].device))) return rc;
  hipStream_t st;
  if ((rc = thread_stream(dev, &st))) return rc;
  void *flag;
  if ((rc = arena(dev, st, 256, &flag))) return rc;
  uint32_t *map = nullptr;
  int64_t *doff = nullptr;
  hipError_t e = hipMalloc(&map, (size_t)kept * 4);
  if (e == hipSuccess) e = hipMalloc(&doff, off.size() * 8);
  if (e != hipSuccess) {
    if (map) (void)hipFree(map);
    return fail(PMM_ERR_HIP, "partition allocation failed on device %d: %s", dev, hipGetErrorString(e));
  }
  {
    Timed t("h2d", st);
    e = hipMemcpyAsync(map, perm.data(), (size_t)kept * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(doff, off.data(), off.size() * 8, hipMemcpyHostToDevice, st);
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(map);
    (void)hipFree(doff);
    return fail(PMM_ERR_HIP, "partition upload failed: %s", hipGetErrorString(e));
  }
  // (subset_build waits for the stream: the uploads above read this frame's vectors)
  if ((rc = subset_build(p, map, kept, (unsigned *)flag, st, out, false))) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(doff);
    return rc;
  }
  pmm_corpus *h = *out;
  h->offsets = std::move(off);
  h->d_offsets = doff;
  h->screen_never.store(true, std::memory_order_release);
  return PMM_OK;
}

int pmm_corpus_groups(const pmm_corpus *h, int64_t *G, int64_t *offsets, int64_t cap) {
  if (!h || !G) return fail(PMM_ERR_ARG, "null argument");
  *G = h->partitioned() ? (int64_t)h->offsets.size() - 1 : 0;
  const int64_t take = h->partitioned() ? std::min<int64_t>(cap, (int64_t)h->offsets.size()) : 0;
  if (take <= 0) return PMM_OK;
  if (!offsets) return fail(PMM_ERR_ARG, "null argument");
  memcpy(offsets, h->offsets.data(), (size_t)take * 8);
  return PMM_OK;
}

int pmm_topk_f32_grouped(const pmm_corpus *h, const float *q, int64_t m, const uint32_t *qlabels, int64_t k,
                         int metric, uint32_t *out_idx, float *out_score, uint32_t *out_len) {
  return topk_grouped<float>(h, q, m, qlabels, k, metric, out_idx, out_score, out_len);
}

int pmm_topk_f64_grouped(const pmm_corpus *h, const double *q, int64_t m, const uint32_t *qlabels, int64_t k,
                         int metric, uint32_t *out_idx, double *out_score, uint32_t *out_len) {
  return topk_grouped<double>(h, q, m, qlabels, k, metric, out_idx, out_score, out_len);
}

int pmm_probe_plan(const int64_t *probe_offsets, const uint32_t *probe_labels, int64_t m,
                   const int64_t *group_offsets, int64_t G, int64_t k, uint32_t *slot_row, uint32_t *slot_label,
                   int64_t *row_offsets, uint32_t *row_slots, uint32_t *out_len, int64_t *slots) {
  return probe_plan(probe_offsets, probe_labels, m, group_offsets, G, k, slot_row, slot_label, row_offsets, row_slots,
                    out_len, slots);
}

int pmm_topk_f32_probed(const pmm_corpus *h, const float *q, int64_t m, const int64_t *probe_offsets,
                        const uint32_t *probe_labels, int64_t k, int metric, uint32_t *out_idx, float *out_score,
                        uint32_t *out_len) {
  return topk_probed(h, q, m, probe_offsets, probe_labels, k, metric, out_idx, out_score, out_len);
}

int pmm_corpus_create_f64(const double *c, int64_t n, int64_t d, pmm_corpus **out) {
  return corpus_create(PMM_DTYPE_F64, c, n, d, out);
}

int pmm_topk_f64_corpus(const pmm_corpus *h, const double *q, int64_t m, int64_t k, int metric,
                        uint32_t *out_idx, double *out_score) {
  bool fused = false;
  return corpus_topk(
      h, PMM_DTYPE_F64, q, m, k, metric, out_idx, out_score,
      [&](const HostCall<double> &, Layout &) {
        fused = f64_use_fused(m, h->n, k);
        return f64_workspace_bytes(m, h->n, k, fused);
      },
      [&](const HostCall<double> &f) {
        const CorpusShard &x = h->shards[0];
        return topk_f64_device_impl((const double *)f.q, h->dp, m, x.rows_as<double>(), h->dp, h->n, h->d, k, metric, 0u,
                                    f.oi, f.os, f.w, f.s, fused, shard_norms<double>(h, x, metric));
      });
}

// The route of m query rows on an f32 handle of one shard: the screened route
// when the shape asks for it (screen_wanted, as the device entry's) and the
// handle has, or can now build, its ScreenImage (*img); else the f32 kernel on
// the cached norms, as for every other metric.
static TopkRoute f32_handle_route(const pmm_corpus *h, int64_t m, int64_t k, int metric,
                                  const HostCall<float> &f, const ScreenImage **img) {
  TopkRoute route = route_topk(m, h->n, h->d, k, metric, PMM_COMPUTE_F32, g_dev[f.dev].cus, true, true, true);
  *img = route.kind == Route::kF32Screened ? corpus_screen_image(h, f.s) : nullptr;
  if (!*img) route = route_topk(m, h->n, h->d, k, metric, PMM_COMPUTE_F32, g_dev[f.dev].cus, false, false);
  return route;
}

int pmm_topk_f32_corpus(const pmm_corpus *h, const float *q, int64_t m, int64_t k, int metric,
                        uint32_t *out_idx, float *out_score) {
  TopkRoute route;
  const ScreenImage *img = nullptr;
  return corpus_topk(
      h, PMM_DTYPE_F32, q, m, k, metric, out_idx, out_score,
      [&](const HostCall<float> &f, Layout &) {
        route = f32_handle_route(h, m, k, metric, f, &img);
        return route.total;
      },
      [&](const HostCall<float> &f) {
        const CorpusShard &x = h->shards[0];
        return topk_f32_device_impl(route, (const float *)f.q, h->dp, m, x.rows_as<float>(), h->dp, h->n, h->d, k, metric,
                                    0u, f.oi, f.os, f.w, f.ws_bytes, f.s, f.dev, shard_norms<float>(h, x, metric), false,
                                    img);
      });
}

// Range search.  The tile variant of the emit pass: the ones
// the range mode is instantiated for, PMM_GEMM_VARIANT (per call) choosing
// among them, else choose_variant's size rule between 128 x 128 and 256 x 256.
static int range_variant_by_size(int64_t m, int64_t n, int cus) {
  return cdiv(m, 256) * cdiv(n, 256) < 4 * (int64_t)cus ? 0 : 3;
}
static int range_variant(int64_t m, int64_t n, int cus) {
  const char *ev = getenv("PMM_GEMM_VARIANT");
  const int env = ev ? atoi(ev) : -1;
  if (env >= 0 && gemm_f32_range_variant(env)) return env;
  return range_variant_by_size(m, n, cus);
}

// The longest segment the in-LDS sort takes: kRangeSortMax, or a lower
// PMM_RANGE_SORT_MAX (per call; at least the wave tier's 128) so that a test
// reaches the any-k route with a small corpus.
static int64_t range_sort_max() {
  const char *e = getenv("PMM_RANGE_SORT_MAX");
  const int64_t v = e ? atoll(e) : 0;
  return (v >= kRangeWaveMax && v < kRangeSortMax) ? v : kRangeSortMax;
}

// What the range and self entries (`what`) refuse in a handle.
static int range_handle(const pmm_corpus *h, const char *what) {
  if (h->partitioned()) return partitioned_handle(h);
  if (h->dtype == PMM_DTYPE_I8 || h->dtype == PMM_DTYPE_BITS)
    return fail(PMM_ERR_UNSUPPORTED, "%s takes an f32 handle: %s handle has no %s", what,
                h->dtype == PMM_DTYPE_I8 ? "an int8" : "a bit", what);
  if (h->dtype != PMM_DTYPE_F32) {
    static const char *const kRows[] = {"f32", "f64", "bf16"};
    return fail(PMM_ERR_ARG, "%s takes an f32 handle: this one holds %s rows", what, kRows[h->dtype]);
  }
  if (h->shards.size() != 1)
    return fail(PMM_ERR_UNSUPPORTED, "a device-sharded corpus (%d shards) has no %s: use a handle of one shard",
                (int)h->shards.size(), what);
  return PMM_OK;
}

static int range_search(const pmm_corpus *h, bool self, const float *q, int64_t m, float threshold, int metric,
                        int64_t cap, int64_t *out_offsets, uint32_t *out_idx, float *out_score, int64_t *total);

int pmm_range_f32_corpus(const pmm_corpus *h, const float *q, int64_t m, float threshold, int metric, int64_t cap,
                         int64_t *out_offsets, uint32_t *out_idx, float *out_score, int64_t *total) {
  return range_search(h, false, q, m, threshold, metric, cap, out_offsets, out_idx, out_score, total);
}

int pmm_range_f32_self(const pmm_corpus *h, float threshold, int metric, int64_t cap, int64_t *out_offsets,
                       uint32_t *out_idx, float *out_score, int64_t *total) {
  return range_search(h, true, nullptr, 0, threshold, metric, cap, out_offsets, out_idx, out_score, total);
}

int pmm_topk_f32_self(const pmm_corpus *h, int64_t k, int metric, uint32_t *out_idx, float *out_score) {
  // every argument check before the handle is read or a device touched
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (!out_idx || !out_score) return fail(PMM_ERR_ARG, "null argument");
  if (k < 1) return fail(PMM_ERR_ARG, "k must be >= 1 (got %lld)", (long long)k);
  int rc = check_metric(metric);
  if (rc) return rc;
  if ((rc = range_handle(h, "self search"))) return rc;
  const int64_t n = h->n;
  if (k >= n)
    return fail(PMM_ERR_ARG, "k (%lld) must be <= n - 1 (n = %lld): a row has n - 1 neighbours, clip k first",
                (long long)k, (long long)n);
  if ((rc = validate_sizes(n, n, h->d, k + 1, true))) return rc;
  // The handle's route for k + 1 with its own rows as the (device-resident)
  // queries, into lists of the entry's own; the drop-self pass writes the
  // frame's k-lists from them, ahead of a derived handle's remap, so a row's
  // own id is its position.
  TopkRoute route;
  const ScreenImage *img = nullptr;
  size_t off_i1 = 0, off_s1 = 0;
  return host_topk(
      h, HostRows{}, HostRows{}, n, k, out_idx, out_score,
      [&](const HostCall<float> &f, Layout &L) {
        off_i1 = L.take((size_t)n * (k + 1) * 4), off_s1 = L.take((size_t)n * (k + 1) * 4);
        route = f32_handle_route(h, n, k + 1, metric, f, &img);
        return route.total;
      },
      [&](const HostCall<float> &f) -> int {
        const CorpusShard &x = h->shards[0];
        uint32_t *i1 = (uint32_t *)(f.b + off_i1);
        float *s1 = (float *)(f.b + off_s1);
        if (int rc2 = topk_f32_device_impl(route, x.rows_as<float>(), h->dp, n, x.rows_as<float>(), h->dp, n, h->d, k + 1,
                                           metric, 0u, i1, s1, f.w, f.ws_bytes, f.s, f.dev,
                                           shard_norms<float>(h, x, metric), false, img))
          return rc2;
        Timed t("drop_self", f.s);
        HIP_TRY(launch_drop_self(i1, s1, n, k, f.oi, f.os, f.s));
        return PMM_OK;
      });
}

int pmm_range_self_plan(int64_t n, int cus, int variant_in, int *variant, int64_t *block_tile_visits,
                        int64_t *block_tile_full) {
  if (!variant || !block_tile_visits || !block_tile_full) return fail(PMM_ERR_ARG, "null argument");
  if (n < 0 || n > INT32_MAX || cus < 1 || (variant_in != -1 && !gemm_f32_range_variant(variant_in)))
    return fail(PMM_ERR_ARG, "bad self plan arguments (n=%lld cus=%d variant=%d: the variant is 0, 3 or -1)",
                (long long)n, cus, variant_in);
  const int v = variant_in >= 0 ? variant_in : range_variant_by_size(n, n, cus);
  const int bm = gemm_f32_bm(v), bn = gemm_f32_bn(v);
  const int64_t QB = cdiv(n, bm), T = cdiv(n, bn);
  int64_t visits = 0;
  for (int64_t b = 0; b < QB; b++) visits += T - self_first_tile((int)n, (int)(b * bm), bn, (int)T);
  *variant = v;
  *block_tile_visits = visits;
  *block_tile_full = QB * T;
  return PMM_OK;
}

// The sort plan of ragged key lists (range, self and candidate search;
// DESIGN.md §4d "Piece planner and sort driver"), from the m + 1 host bounds
// of the segments.  A segment of up to smax keys is one piece; a longer one is
// cut into pieces of smax (the last one shorter), each sorted on its own, and
// its best min(cap, count) keys are merged to merged keys from `dst` on.
struct SortPlan {
  std::vector<int64_t> po;     // the piece bounds
  std::vector<int> mid;        // the pieces of more than kRangeWaveMax keys: the block sort's
  int64_t mid_max = 0;         // the longest of them
  std::vector<CandPiece> cut;  // one per piece of a cut segment
  int64_t merged = 0;          // the merged keys of all cut segments
};
static void plan_pieces(const int64_t *offsets, int64_t m, int64_t smax, int64_t cap, SortPlan &p) {
  p.po.assign(1, 0);
  for (int64_t i = 0; i < m; i++) {
    const int64_t o = offsets[i], c = offsets[i + 1] - o;
    const int64_t T = c > smax ? cdiv(c, smax) : 1, first = (int64_t)p.po.size() - 1;
    if (T > 1) {
      const int64_t kout = std::min(cap, c);
      for (int64_t t = 0; t < T; t++)
        p.cut.push_back(CandPiece{(uint32_t)(first + t), (uint32_t)first, (uint32_t)T, (uint32_t)kout, p.merged});
      p.merged += kout;
    }
    for (int64_t t = 0; t < T; t++) {
      const int64_t len = std::min(smax, c - t * smax);
      if (len > kRangeWaveMax) {
        p.mid.push_back((int)(first + t));
        p.mid_max = std::max(p.mid_max, len);
      }
      p.po.push_back(o + t * smax + len);
    }
  }
}

// The sort of every segment of `keys` by a plan: the plan's tables to their
// device places (d_po, d_cut: used only with a cut segment -- without one the
// pieces are the m rows and the device offsets d_offs their bounds), the wave
// and block sorts over the pieces, and the cut segments' merge into dst.  The
// uploads read the plan: the caller runs this inside ShardCall::run.
static int sort_segments(unsigned long long *keys, const int64_t *d_offs, int64_t m, const SortPlan &p, int64_t *d_po,
                         int *d_mid, CandPiece *d_cut, unsigned long long *dst, hipStream_t s) {
  const bool cut = !p.cut.empty();
  if (cut) {
    HIP_TRY(hipMemcpyAsync(d_po, p.po.data(), p.po.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_cut, p.cut.data(), p.cut.size() * sizeof(CandPiece), hipMemcpyHostToDevice, s));
  }
  const int64_t *bounds = cut ? d_po : d_offs;
  {
    Timed t("range_sort_wave", s);
    HIP_TRY(launch_range_sort_wave(keys, bounds, cut ? (int)(p.po.size() - 1) : (int)m, s));
  }
  if (!p.mid.empty()) {
    HIP_TRY(hipMemcpyAsync(d_mid, p.mid.data(), p.mid.size() * 4, hipMemcpyHostToDevice, s));
    Timed t("range_sort_block", s);
    HIP_TRY(launch_range_sort_block(keys, bounds, d_mid, (int)p.mid.size(), next_pow2((int)p.mid_max), s));
  }
  if (cut) {
    Timed t("cand_merge", s);
    HIP_TRY(launch_cand_merge(keys, bounds, d_cut, (int)p.cut.size(), dst, s));
  }
  return PMM_OK;
}

int pmm_sort_plan(const int64_t *offsets, int64_t m, int64_t smax, int64_t cap, int64_t *piece_offsets, int *mid,
                  pmm_sort_piece *cut, int64_t *counts) {
  static_assert(sizeof(pmm_sort_piece) == sizeof(CandPiece), "pmm.h states CandPiece's layout");
  if (!offsets || !piece_offsets || !mid || !cut || !counts) return fail(PMM_ERR_ARG, "null argument");
  bool ok = m >= 0 && smax >= kRangeWaveMax && smax <= kRangeSortMax && cap >= 1 && offsets[0] == 0;
  for (int64_t i = 0; ok && i < m; i++) ok = offsets[i + 1] >= offsets[i];
  if (!ok)
    return fail(PMM_ERR_ARG, "bad sort plan arguments (m=%lld smax=%lld cap=%lld: smax in [%d, %d], cap >= 1, "
                             "offsets ascending from 0)", (long long)m, (long long)smax, (long long)cap, kRangeWaveMax,
                kRangeSortMax);
  SortPlan p;
  plan_pieces(offsets, m, smax, cap, p);
  std::copy(p.po.begin(), p.po.end(), piece_offsets);
  std::copy(p.mid.begin(), p.mid.end(), mid);
  memcpy(cut, p.cut.data(), p.cut.size() * sizeof(CandPiece));
  const int64_t n[5] = {(int64_t)p.po.size() - 1, (int64_t)p.mid.size(), p.mid_max, (int64_t)p.cut.size(), p.merged};
  std::copy(n, n + 5, counts);
  return PMM_OK;
}

// What both range entries check before the handle is read or a device touched
// (the self form has no q and no m).
static int range_args(const pmm_corpus *h, bool self, const float *q, int64_t m, float threshold, int metric,
                      int64_t cap, const int64_t *out_offsets, const uint32_t *out_idx, const float *out_score,
                      const int64_t *total) {
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if ((!self && !q) || !out_offsets || !total) return fail(PMM_ERR_ARG, "null argument");
  if (!self && (m < 0 || cap < 0))
    return fail(PMM_ERR_ARG, "negative size (m=%lld cap=%lld)", (long long)m, (long long)cap);
  if (cap < 0) return fail(PMM_ERR_ARG, "negative size (cap=%lld)", (long long)cap);
  if (cap > 0 && (!out_idx || !out_score))
    return fail(PMM_ERR_ARG, "null argument: cap > 0 needs out_idx and out_score (cap = 0 is the count-only form)");
  if (int rc = check_metric(metric)) return rc;
  if (threshold != threshold) return fail(PMM_ERR_ARG, "the range threshold is NaN");
  return PMM_OK;
}

// The body of both range entries.  The self form: the handle's rows are the
// m = n query rows and its norms their norms, nothing is uploaded, the emit
// pass runs the triangular schedule (launch_gemm_f32_self) and a row records
// only its hits at positions above it.
static int range_search(const pmm_corpus *h, bool self, const float *q, int64_t m, float threshold, int metric,
                        int64_t cap, int64_t *out_offsets, uint32_t *out_idx, float *out_score, int64_t *total) {
  int rc = range_args(h, self, q, m, threshold, metric, cap, out_offsets, out_idx, out_score, total);
  if (rc) return rc;
  if ((rc = range_handle(h, self ? "self search" : "range search"))) return rc;
  if (self) m = h->n;
  if ((rc = validate_sizes(m, h->n, h->d, 0, false))) return rc;
  *total = 0;
  out_offsets[0] = 0;
  if (m == 0) return PMM_OK;
  if (self && m == 1) {  // (one row has no pair)
    out_offsets[1] = 0;
    return PMM_OK;
  }

  const CorpusShard &x = h->shards[0];
  ShardCall f;
  if ((rc = f.open(h))) return rc;
  const hipStream_t s = f.s;
  const int64_t n = h->n, d = h->d, dp = h->dp;
  Plan p;
  p.variant = range_variant(m, n, f.cus);
  const int bn = gemm_f32_bn(p.variant);
  plan_units(m, n, gemm_f32_bm(p.variant), bn, f.cus, 0.5, 1 << 20, p);
  // the record arena never needs more than m x n records (self: the pairs)
  const uint64_t rcap = (uint64_t)std::min<int64_t>(cap, self ? n * (n - 1) / 2 : m * n);
  // self: a row past the in-LDS sort is cut into pieces (below); of tot <= rcap
  // keys, at most rcap / 128 pieces more than rows and rcap / 64 cut pieces
  const size_t max_pieces = self ? (size_t)m + rcap / kRangeWaveMax + 1 : 0;
  const size_t max_cut = self ? rcap / (kRangeWaveMax / 2) + 1 : 0;

  // arena: queries | [work counter, cursor | hit counts | bin cursors] (one
  // fill) | query norms | offsets | row list | survivor queues | records (key,
  // row) | binned keys; the decoded lists reuse the record keys' bytes
  // (self: no queries and no query norms; a piece list for the row list, and
  // the piece bounds and cut pieces at the end)
  Layout L;
  const size_t off_q = L.take(self ? 0 : (size_t)m * dp * 4);
  const size_t off_ctl = L.take(256);
  const size_t off_hits = L.take((size_t)m * 4);
  const size_t off_cur = L.take((size_t)m * 4);
  const size_t off_qn = L.take(self ? 0 : (size_t)m * 4);
  const size_t off_offs = L.take((size_t)(m + 1) * 8);
  const size_t off_rows = L.take((self ? max_pieces : (size_t)m) * 4);
  const size_t off_wq = L.take((size_t)p.grid * gemm_f32_nw(p.variant) * 32 * bn * 8);
  const size_t off_rkey = L.take((size_t)rcap * 8);
  const size_t off_rrow = L.take((size_t)rcap * 4);
  const size_t off_keys = L.take((size_t)rcap * 8);
  const size_t off_po = L.take((max_pieces + 1) * 8);
  const size_t off_cut = L.take(max_cut * sizeof(CandPiece));
  void *base;
  if ((rc = arena(f.dev, s, L.off, &base))) return rc;
  char *b = (char *)base;
  const float *dq = self ? x.rows_as<float>() : (const float *)(b + off_q);
  if (!self && (rc = upload_padded(b + off_q, q, m, d, dp, 4, s))) return rc;
  HIP_TRY(hipMemsetAsync(b + off_ctl, 0, off_qn - off_ctl, s));
  const float *qn = self ? shard_norms<float>(h, x, metric) : (const float *)(b + off_qn);
  if (!self && metric != kMetricDot) {
    Timed t("norms_f32", s);
    HIP_TRY(launch_norms_f32(dq, m, d, dp, metric == kMetricEuclidean, (float *)(b + off_qn), nullptr, s));
  }
  // the threshold's composite: okey32 of its ranking value (-0 folds onto +0,
  // so both zeros compare alike), index part 0 -- at or above it is a hit
  const float rank = metric == kMetricEuclidean ? -threshold : threshold;
  uint32_t tu;
  memcpy(&tu, &rank, 4);
  if ((tu << 1) == 0u) tu = 0u;
  const uint32_t tkey = (tu & 0x80000000u) ? ~tu : (tu | 0x80000000u);

  GemmF32Args a{};
  a.q = dq;
  a.c = x.rows_as<float>();
  a.qn = qn;
  a.cn = shard_norms<float>(h, x, metric);
  a.cpre = a.cn ? a.cn + n : nullptr;
  a.ldq = dp;
  a.ldc = dp;
  a.M = (int)m;
  a.N = (int)n;
  a.D = (int)dp;
  a.metric = metric;
  a.QB = p.QB;
  a.S = p.S;
  a.tps = p.tps;
  a.ntiles = p.T;
  a.units = p.units;
  a.counter = (unsigned *)(b + off_ctl);
  a.wq = (unsigned long long *)(b + off_wq);
  a.rthr = (unsigned long long)tkey << 32;
  a.rcur = (unsigned long long *)(b + off_ctl + 8);
  a.rhits = (unsigned *)(b + off_hits);
  a.rkey = (unsigned long long *)(b + off_rkey);
  a.rrow = (uint32_t *)(b + off_rrow);
  a.rcap = rcap;
  if (self) {
    Timed t("gemm_f32_self", s);
    HIP_TRY(launch_gemm_f32_self(a, p.variant, p.grid, s));
  } else {
    Timed t("gemm_f32_range", s);
    HIP_TRY(launch_gemm_f32_range(a, p.variant, p.grid, s));
  }
  // (from here on a failure waits for the stream: the copies read and write this frame's vectors)
  std::vector<uint32_t> hits((size_t)m);
  unsigned long long cursor = 0;
  SortPlan plan;
  std::vector<int> longr;  // the rows the handle's ordinary top-k serves at the end
  rc = f.run([&]() -> int {
    // the count: the rows' hits and the cursor, the call's one wait before the lists
    {
      Timed t("d2h", s);
      HIP_TRY(hipMemcpyAsync(hits.data(), a.rhits, (size_t)m * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(&cursor, a.rcur, 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t i = 0; i < m; i++) out_offsets[i + 1] = out_offsets[i] + (int64_t)hits[(size_t)i];
    const int64_t tot = out_offsets[m];
    if ((unsigned long long)tot != cursor)
      return fail(PMM_ERR_HIP, "range search: the rows' counts (%lld) and the record cursor (%llu) disagree",
                  (long long)tot, cursor);
    *total = tot;
    if (tot > cap || tot == 0) return PMM_OK;

    // Rows by sort tier: up to 128 keys in a wave, up to smax in a workgroup's
    // LDS.  A longer row goes to the handle's ordinary top-k at the end; self,
    // whose pairs j > i that top-k does not know, cuts it into pieces instead
    // (plan_pieces, cap = the row's count), merges the row's whole order into
    // the record keys' bytes, free since the bin pass, and copies it back.
    const int64_t smax = range_sort_max();
    if (self) {
      plan_pieces(out_offsets, m, smax, INT64_MAX, plan);
      if (plan.po.size() > max_pieces + 1 || plan.cut.size() > max_cut || plan.po.size() - 1 > (size_t)INT32_MAX)
        return fail(PMM_ERR_HIP, "self search: %zu pieces, %zu of cut rows, past the arena's tables",
                    plan.po.size() - 1, plan.cut.size());
    } else {
      for (int64_t i = 0; i < m; i++) {
        const int64_t c = (int64_t)hits[(size_t)i];
        if (c > smax) longr.push_back((int)i);
        else if (c > kRangeWaveMax) {
          plan.mid.push_back((int)i);
          plan.mid_max = std::max(plan.mid_max, c);
        }
      }
    }
    int64_t *d_offs = (int64_t *)(b + off_offs);
    unsigned long long *keys = (unsigned long long *)(b + off_keys);
    HIP_TRY(hipMemcpyAsync(d_offs, out_offsets, (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
    {
      Timed t("range_bin", s);
      HIP_TRY(launch_range_bin(a.rkey, a.rrow, tot, d_offs, (unsigned *)(b + off_cur), keys, s));
    }
    if (int rc2 = sort_segments(keys, d_offs, m, plan, (int64_t *)(b + off_po), (int *)(b + off_rows),
                                (CandPiece *)(b + off_cut), a.rkey, s))
      return rc2;
    for (const CandPiece &c : plan.cut)  // a cut row's merged order, back to its segment
      if (c.self == c.first)
        HIP_TRY(hipMemcpyAsync(keys + plan.po[c.first], a.rkey + c.dst, (size_t)c.kout * 8, hipMemcpyDeviceToDevice,
                               s));
    RangeDecodeArgs da{};
    da.keys = keys;
    da.total = tot;
    da.offsets = d_offs;
    da.m = (int)m;
    da.metric = metric;
    da.d = (int)d;
    da.map = h->map;
    da.q = dq;
    da.c = a.c;
    da.qn = qn;
    da.cn = a.cn;
    da.ldq = dp;
    da.ldc = dp;
    da.out_idx = (uint32_t *)(b + off_rkey);  // (the records are binned, a cut row merged: their bytes are free)
    da.out_score = (float *)(b + off_rkey + (size_t)tot * 4);
    {
      Timed t("range_decode", s);
      HIP_TRY(launch_range_decode(da, s));
    }
    {
      Timed t("d2h", s);
      HIP_TRY(hipMemcpyAsync(out_idx, da.out_idx, (size_t)tot * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_score, da.out_score, (size_t)tot * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return PMM_OK;
  });
  if (rc) return rc;

  // Segments past the in-LDS sort: the row's list is the first count entries
  // of its top-k list with k = count (the defining property), so those rows go
  // through pmm_topk_f32_corpus, a batch of at most 2^26 list entries at a time.
  for (size_t i0 = 0; i0 < longr.size();) {
    size_t i1 = i0;
    int64_t kmax = 0;
    while (i1 < longr.size()) {
      const int64_t k2 = std::max<int64_t>(kmax, hits[(size_t)longr[i1]]);
      if (i1 > i0 && (int64_t)(i1 - i0 + 1) * k2 > (int64_t(1) << 26)) break;
      kmax = k2;
      i1++;
    }
    const size_t r = i1 - i0;
    std::vector<float> qb(r * (size_t)d);
    for (size_t j = 0; j < r; j++) memcpy(&qb[j * (size_t)d], q + (size_t)longr[i0 + j] * d, (size_t)d * 4);
    std::vector<uint32_t> ti(r * (size_t)kmax);
    std::vector<float> ts(r * (size_t)kmax);
    if ((rc = pmm_topk_f32_corpus(h, qb.data(), (int64_t)r, kmax, metric, ti.data(), ts.data()))) return rc;
    for (size_t j = 0; j < r; j++) {
      const int row = longr[i0 + j];
      const size_t c = hits[(size_t)row];
      memcpy(out_idx + out_offsets[row], &ti[j * (size_t)kmax], c * 4);
      memcpy(out_score + out_offsets[row], &ts[j * (size_t)kmax], c * 4);
    }
    i0 = i1;
  }
  return PMM_OK;
}

// Duplicate groups (DESIGN.md §4d "Duplicate groups"): the connected
// components of the self range search's pairs.  The self path of range_search
// with the components pass in place of the emit pass: a hit unites its two
// rows where it is found, so the arena holds n parents and n labels whatever
// the number of hits, and there is no second run, bin, sort or decode.
int pmm_components_f32_self(const pmm_corpus *h, float threshold, int metric, uint32_t *out_labels,
                            int64_t *components, int64_t *pairs) {
  // every argument check before the handle is read or a device touched
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (!components || !pairs) return fail(PMM_ERR_ARG, "null argument");
  int rc = check_metric(metric);
  if (rc) return rc;
  if (threshold != threshold) return fail(PMM_ERR_ARG, "the range threshold is NaN");
  if ((rc = range_handle(h, "self search"))) return rc;
  const int64_t n = h->n, dp = h->dp;
  if ((rc = validate_sizes(n, n, h->d, 0, false))) return rc;
  if (n > 0 && !out_labels) return fail(PMM_ERR_ARG, "null argument");
  *components = 0;
  *pairs = 0;
  if (n == 0) return PMM_OK;

  if (n == 1 && !h->map) {  // (one row has no pair: its own number, no device touched)
    out_labels[0] = 0u;
    *components = 1;
    return PMM_OK;
  }
  const CorpusShard &x = h->shards[0];
  ShardCall f;
  if ((rc = f.open(h))) return rc;
  const hipStream_t s = f.s;
  if (n == 1) {  // (derived: the row's parent number is on the device; a copy, no launch)
    rc = f.run([&]() -> int {
      HIP_TRY(hipMemcpyAsync(out_labels, h->map, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      return PMM_OK;
    });
    if (rc) return rc;
    *components = 1;
    return PMM_OK;
  }
  Plan p;
  p.variant = range_variant(n, n, f.cus);
  const int bn = gemm_f32_bn(p.variant);
  plan_units(n, n, gemm_f32_bm(p.variant), bn, f.cus, 0.5, 1 << 20, p);

  // arena: [work counter, cursor] | parent | labels | survivor queues --
  // nothing in it depends on the number of hits
  Layout L;
  const size_t off_ctl = L.take(256);
  const size_t off_parent = L.take((size_t)n * 4);
  const size_t off_labels = L.take((size_t)n * 4);
  const size_t off_wq = L.take((size_t)p.grid * gemm_f32_nw(p.variant) * 32 * bn * 8);
  void *base;
  if ((rc = arena(f.dev, s, L.off, &base))) return rc;
  char *b = (char *)base;
  HIP_TRY(hipMemsetAsync(b + off_ctl, 0, 256, s));
  uint32_t *parent = (uint32_t *)(b + off_parent), *labels = (uint32_t *)(b + off_labels);
  HIP_TRY(launch_components_init(parent, n, s));
  // the threshold's composite, as range_search states it
  const float rank = metric == kMetricEuclidean ? -threshold : threshold;
  uint32_t tu;
  memcpy(&tu, &rank, 4);
  if ((tu << 1) == 0u) tu = 0u;
  const uint32_t tkey = (tu & 0x80000000u) ? ~tu : (tu | 0x80000000u);

  GemmF32Args a{};
  a.q = x.rows_as<float>();
  a.c = a.q;
  a.qn = shard_norms<float>(h, x, metric);
  a.cn = a.qn;
  a.cpre = a.cn ? a.cn + n : nullptr;
  a.ldq = dp;
  a.ldc = dp;
  a.M = (int)n;
  a.N = (int)n;
  a.D = (int)dp;
  a.metric = metric;
  a.QB = p.QB;
  a.S = p.S;
  a.tps = p.tps;
  a.ntiles = p.T;
  a.units = p.units;
  a.counter = (unsigned *)(b + off_ctl);
  a.wq = (unsigned long long *)(b + off_wq);
  a.rthr = (unsigned long long)tkey << 32;
  a.rcur = (unsigned long long *)(b + off_ctl + 8);
  a.parent = parent;
  {
    Timed t("gemm_f32_components", s);
    HIP_TRY(launch_gemm_f32_components(a, p.variant, p.grid, s));
  }
  {
    Timed t("components_label", s);
    HIP_TRY(launch_components_label(parent, h->map, n, labels, s));
  }
  // the call's one wait: the labels and the cursor together
  unsigned long long cursor = 0;
  rc = f.run([&]() -> int {
    {
      Timed t("d2h", s);
      HIP_TRY(hipMemcpyAsync(out_labels, labels, (size_t)n * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(&cursor, a.rcur, 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return PMM_OK;
  });
  if (rc) return rc;
  // The count leans on two facts, both stated here and nowhere else: unite
  // always links the higher root under the lower, so a component's root is its
  // smallest position; and a derived handle's map ascends, so labels keep the
  // positions' order.  Then a root's label is above every label at a lower
  // position, and a member's label (its root's) is not: the roots are the
  // positions where the running maximum of the labels rises.
  int64_t roots = 1;
  uint32_t top = out_labels[0];
  for (int64_t i = 1; i < n; i++)
    if (out_labels[i] > top) {
      top = out_labels[i];
      roots++;
    }
  *components = roots;
  *pairs = (int64_t)cursor;
  return PMM_OK;
}

// Candidate search (DESIGN.md §4d "Candidate lists"): score every (row,
// candidate) pair into the CSR key layout of the range search, sort each
// row's segment with its kernels, cut at k and decode into the [m][k] planes.
int pmm_topk_f32_candidates(const pmm_corpus *h, const float *q, int64_t m, const int64_t *cand_offsets,
                            const uint32_t *cand_ids, int64_t k, int metric, uint32_t *out_idx, float *out_score,
                            uint32_t *out_len) {
  // every argument check before the handle is read or a device touched
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (m < 0) return fail(PMM_ERR_ARG, "negative size (m=%lld)", (long long)m);
  if (k < 1) return fail(PMM_ERR_ARG, "k must be >= 1 (got %lld)", (long long)k);
  int rc = check_metric(metric);
  if (rc) return rc;
  if (h->dtype != PMM_DTYPE_F32) {
    static const char *const kRows[] = {"f32", "f64", "bf16", "int8", "bit"};
    return fail(PMM_ERR_ARG, "candidate search takes an f32 handle: this one holds %s rows", kRows[h->dtype]);
  }
  if (h->partitioned())
    return fail(PMM_ERR_ARG, "candidate search takes a plain f32 handle: this one is partitioned "
                             "(pmm_corpus_partition); list the candidates in its parent's row numbers and search the parent");
  if (h->map)
    return fail(PMM_ERR_ARG, "candidate search takes a plain f32 handle: this one is derived (pmm_corpus_subset_*); "
                             "list the candidates in its parent's row numbers and search the parent");
  if (h->shards.size() != 1)
    return fail(PMM_ERR_UNSUPPORTED,
                "a device-sharded corpus (%d shards) has no candidate search: use a handle of one shard",
                (int)h->shards.size());
  if ((rc = validate_sizes(m, h->n, h->d, 0, false))) return rc;
  if (m == 0) return PMM_OK;
  if (!q || !cand_offsets || !out_idx || !out_score || !out_len) return fail(PMM_ERR_ARG, "null argument");
  const int64_t n = h->n, d = h->d, dp = h->dp;
  if (cand_offsets[0] != 0)
    return fail(PMM_ERR_ARG, "cand_offsets must start at 0 (cand_offsets[0] = %lld)", (long long)cand_offsets[0]);
  for (int64_t i = 0; i < m; i++) {
    const int64_t c = cand_offsets[i + 1] - cand_offsets[i];
    if (c < 0)
      return fail(PMM_ERR_ARG, "cand_offsets must not descend: cand_offsets[%lld] = %lld follows %lld",
                  (long long)(i + 1), (long long)cand_offsets[i + 1], (long long)cand_offsets[i]);
    if (c > n)
      return fail(PMM_ERR_ARG, "row %lld lists %lld candidates, the corpus has %lld rows: its ids cannot be strictly "
                               "ascending", (long long)i, (long long)c, (long long)n);
  }
  const int64_t total = cand_offsets[m];
  if (total > 0 && !cand_ids) return fail(PMM_ERR_ARG, "null argument");
  if (m > (int64_t(1) << 40) / k)
    return fail(PMM_ERR_ARG, "m * k out of range (m=%lld k=%lld): clip k to the longest list first", (long long)m,
                (long long)k);

  // Host tables.  Units of the score pass: a row's candidates 256 at a time.
  // The sort plan (plan_pieces, cap = k): a cut row's best min(k, count) keys
  // are merged into a second key array behind the first, where its key source
  // then points.
  const int64_t smax = range_sort_max();
  SortPlan plan;
  plan_pieces(cand_offsets, m, smax, k, plan);
  std::vector<CandUnit> units;
  std::vector<int64_t> src(cand_offsets, cand_offsets + m);
  size_t ci = 0;  // (plan.cut holds the cut rows' pieces in row order)
  for (int64_t i = 0; i < m; i++) {
    const int64_t c = cand_offsets[i + 1] - cand_offsets[i];
    for (int64_t u = 0; u < c; u += kCandUnit) units.push_back(CandUnit{(uint32_t)i, (uint32_t)u});
    if (c > smax) {
      src[(size_t)i] = total + plan.cut[ci].dst;
      ci += plan.cut[ci].T;
    }
  }
  const int64_t npieces = (int64_t)plan.po.size() - 1;
  if ((int64_t)units.size() > INT32_MAX || npieces > INT32_MAX)
    return fail(PMM_ERR_ARG, "too many candidates for one call (%lld): split the query rows", (long long)total);

  const CorpusShard &x = h->shards[0];
  ShardCall f;
  if ((rc = f.open(h))) return rc;
  const hipStream_t s = f.s;
  // arena: queries | query norms | flag | offsets | ids | units | piece bounds
  // | piece list | cut pieces | key sources | keys, merged keys | the planes
  Layout L;
  const size_t off_q = L.take((size_t)m * dp * 4);
  const size_t off_qn = L.take((size_t)m * 4);
  const size_t off_flag = L.take(4);
  const size_t off_offs = L.take((size_t)(m + 1) * 8);
  const size_t off_ids = L.take((size_t)total * 4);
  const size_t off_units = L.take(units.size() * sizeof(CandUnit));
  const size_t off_po = L.take(plan.cut.empty() ? 0 : (size_t)(npieces + 1) * 8);
  const size_t off_mid = L.take(plan.mid.size() * 4);
  const size_t off_cut = L.take(plan.cut.size() * sizeof(CandPiece));
  const size_t off_src = L.take((size_t)m * 8);
  const size_t off_keys = L.take((size_t)(total + plan.merged) * 8);
  const size_t off_oi = L.take((size_t)m * k * 4);
  const size_t off_os = L.take((size_t)m * k * 4);
  const size_t off_len = L.take((size_t)m * 4);
  void *base;
  if ((rc = arena(f.dev, s, L.off, &base))) return rc;
  char *b = (char *)base;
  const float *dq = (const float *)(b + off_q);
  if ((rc = upload_padded(b + off_q, q, m, d, dp, 4, s))) return rc;
  // (from here on a failure waits for the stream: the copies read and write this frame's vectors)
  unsigned flag = 0u;
  rc = f.run([&]() -> int {
    HIP_TRY(hipMemsetAsync(b + off_flag, 0, 4, s));
    int64_t *d_offs = (int64_t *)(b + off_offs);
    {
      Timed t("h2d", s);
      HIP_TRY(hipMemcpyAsync(d_offs, cand_offsets, (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(b + off_src, src.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
      if (total > 0) {
        HIP_TRY(hipMemcpyAsync(b + off_ids, cand_ids, (size_t)total * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b + off_units, units.data(), units.size() * sizeof(CandUnit), hipMemcpyHostToDevice,
                               s));
      }
    }
    float *qn = (float *)(b + off_qn);
    if (metric != kMetricDot) {
      Timed t("norms_f32", s);
      HIP_TRY(launch_norms_f32(dq, m, d, dp, metric == kMetricEuclidean, qn, nullptr, s));
    }
    unsigned long long *keys = (unsigned long long *)(b + off_keys);
    CandScoreArgs sa{};
    sa.q = dq;
    sa.c = x.rows_as<float>();
    sa.qn = qn;
    sa.cn = shard_norms<float>(h, x, metric);
    sa.offsets = d_offs;
    sa.ids = (const uint32_t *)(b + off_ids);
    sa.unit = (const CandUnit *)(b + off_units);
    sa.units = (int)units.size();
    sa.ldq = dp;
    sa.ldc = dp;
    sa.n = (uint32_t)n;
    sa.d = (int)d;
    sa.metric = metric;
    sa.keys = keys;
    sa.flag = (unsigned *)(b + off_flag);
    {
      Timed t("cand_score", s);
      HIP_TRY(launch_cand_score(sa, s));
    }
    if (total > 0)
      if (int rc2 = sort_segments(keys, d_offs, m, plan, (int64_t *)(b + off_po), (int *)(b + off_mid),
                                  (CandPiece *)(b + off_cut), keys + total, s))
        return rc2;
    CandDecodeArgs da{};
    da.keys = keys;
    da.src = (const int64_t *)(b + off_src);
    da.offsets = d_offs;
    da.m = (int)m;
    da.metric = metric;
    da.d = (int)d;
    da.k = k;
    da.q = dq;
    da.c = sa.c;
    da.qn = qn;
    da.cn = sa.cn;
    da.ldq = dp;
    da.ldc = dp;
    da.out_idx = (uint32_t *)(b + off_oi);
    da.out_score = (float *)(b + off_os);
    da.out_len = (uint32_t *)(b + off_len);
    {
      Timed t("cand_decode", s);
      HIP_TRY(launch_cand_decode(da, s));
    }
    {
      Timed t("d2h", s);
      HIP_TRY(hipMemcpyAsync(out_idx, da.out_idx, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_score, da.out_score, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_len, da.out_len, (size_t)m * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(&flag, sa.flag, 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return PMM_OK;
  });
  if (rc) return rc;
  if (flag & 2u)
    return fail(PMM_ERR_ARG, "a candidate id is not a row of the corpus (n=%lld)", (long long)n);
  if (flag & 1u)
    return fail(PMM_ERR_ARG, "candidate ids must be strictly ascending within a row (a row repeats or descends)");
  return PMM_OK;
}

// ---- multi-vector rows (DESIGN.md §4d "Multi-vector rows") ----

int pmm_corpus_create_f32_docs(const float *tokens, int64_t n_tokens, int64_t d, const int64_t *doc_offsets,
                               int64_t n_docs, pmm_corpus **out) {
  if (!out) return fail(PMM_ERR_ARG, "null argument");
  *out = nullptr;
  if (!tokens || !doc_offsets) return fail(PMM_ERR_ARG, "null argument");
  if (n_docs < 1 || n_tokens < 1)
    return fail(PMM_ERR_ARG, "a multi-vector corpus needs a document and a token (n_docs=%lld n_tokens=%lld)",
                (long long)n_docs, (long long)n_tokens);
  // every bound before any device call
  if (doc_offsets[0] != 0)
    return fail(PMM_ERR_ARG, "doc_offsets must start at 0 (doc_offsets[0] = %lld)", (long long)doc_offsets[0]);
  for (int64_t c = 0; c < n_docs; c++)
    if (doc_offsets[c + 1] <= doc_offsets[c])
      return fail(PMM_ERR_ARG, "doc_offsets must ascend strictly (no empty document): doc_offsets[%lld] = %lld follows %lld",
                  (long long)(c + 1), (long long)doc_offsets[c + 1], (long long)doc_offsets[c]);
  if (doc_offsets[n_docs] != n_tokens)
    return fail(PMM_ERR_ARG, "doc_offsets must end at n_tokens (doc_offsets[%lld] = %lld, n_tokens = %lld)",
                (long long)n_docs, (long long)doc_offsets[n_docs], (long long)n_tokens);
  pmm_corpus *h = nullptr;
  int rc = corpus_create(PMM_DTYPE_F32, tokens, n_tokens, d, &h, true);
  if (rc) return rc;
  h->doc_offsets.assign(doc_offsets, doc_offsets + n_docs + 1);
  int dev;
  DevScope scope;
  rc = ensure_device(&dev, &scope, h->shards[0].device);
  if (!rc) {
    hipError_t e = hipMalloc(&h->d_doc_offsets, (size_t)(n_docs + 1) * 8);
    if (e == hipSuccess)
      e = hipMemcpy(h->d_doc_offsets, h->doc_offsets.data(), (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(PMM_ERR_HIP, "document offsets failed on device %d: %s", dev, hipGetErrorString(e));
  }
  if (rc) {
    pmm_corpus_destroy(h);
    return rc;
  }
  *out = h;
  return PMM_OK;
}

int pmm_corpus_docs(const pmm_corpus *h, int64_t *n_docs, int64_t *doc_offsets_out, int64_t cap) {
  if (!h || !n_docs) return fail(PMM_ERR_ARG, "null argument");
  const int64_t nd = h->doc_offsets.empty() ? 0 : (int64_t)h->doc_offsets.size() - 1;
  *n_docs = nd;
  if (nd > 0 && doc_offsets_out && cap >= nd + 1)
    std::copy(h->doc_offsets.begin(), h->doc_offsets.end(), doc_offsets_out);
  return PMM_OK;
}

// Late-interaction search: candidate search's frame with the MaxSim scorer.
// Every (row, listed document) pair is scored into the CSR key layout of the
// lists, each row's segment sorted by the shared driver, cut at k and decoded.
int pmm_topk_f32_maxsim(const pmm_corpus *h, const float *q_tokens, const int64_t *q_offsets, int64_t m,
                        const int64_t *cand_offsets, const uint32_t *cand_docs, int64_t k, int metric,
                        uint32_t *out_idx, float *out_score, uint32_t *out_len) {
  // every argument check before the handle is read or a device touched
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (m < 0) return fail(PMM_ERR_ARG, "negative size (m=%lld)", (long long)m);
  if (k < 1) return fail(PMM_ERR_ARG, "k must be >= 1 (got %lld)", (long long)k);
  int rc = check_metric(metric);
  if (rc) return rc;
  if (metric == kMetricEuclidean)
    return fail(PMM_ERR_ARG, "MaxSim takes cosine or dot: a maximum over euclidean distances is not a similarity");
  if (h->dtype != PMM_DTYPE_F32) {
    static const char *const kRows[] = {"f32", "f64", "bf16", "int8", "bit"};
    return fail(PMM_ERR_ARG, "MaxSim search takes an f32 multi-vector handle: this one holds %s rows", kRows[h->dtype]);
  }
  if (h->partitioned())
    return fail(PMM_ERR_ARG, "MaxSim search takes a multi-vector handle (pmm_corpus_create_f32_docs): this one is "
                             "partitioned (pmm_corpus_partition) and carries no documents; search its parent");
  if (h->map)
    return fail(PMM_ERR_ARG, "MaxSim search takes a multi-vector handle (pmm_corpus_create_f32_docs): this one is "
                             "derived (pmm_corpus_subset_*) and carries no documents; search its parent");
  if (h->doc_offsets.empty())
    return fail(PMM_ERR_ARG, "MaxSim search takes a multi-vector handle: this one has no documents "
                             "(pmm_corpus_create_f32_docs makes one)");
  if (h->shards.size() != 1)
    return fail(PMM_ERR_UNSUPPORTED,
                "a device-sharded corpus (%d shards) has no MaxSim search: use a handle of one shard",
                (int)h->shards.size());
  if (m > INT32_MAX) return fail(PMM_ERR_ARG, "size out of range (m=%lld)", (long long)m);
  if (m == 0) return PMM_OK;
  if (!q_offsets || !cand_offsets || !out_idx || !out_score || !out_len) return fail(PMM_ERR_ARG, "null argument");
  const int64_t nd = (int64_t)h->doc_offsets.size() - 1, d = h->d, dp = h->dp;
  if (q_offsets[0] != 0)
    return fail(PMM_ERR_ARG, "q_offsets must start at 0 (q_offsets[0] = %lld)", (long long)q_offsets[0]);
  if (cand_offsets[0] != 0)
    return fail(PMM_ERR_ARG, "cand_offsets must start at 0 (cand_offsets[0] = %lld)", (long long)cand_offsets[0]);
  for (int64_t i = 0; i < m; i++) {
    if (q_offsets[i + 1] < q_offsets[i])
      return fail(PMM_ERR_ARG, "q_offsets must not descend: q_offsets[%lld] = %lld follows %lld", (long long)(i + 1),
                  (long long)q_offsets[i + 1], (long long)q_offsets[i]);
    const int64_t c = cand_offsets[i + 1] - cand_offsets[i];
    if (c < 0)
      return fail(PMM_ERR_ARG, "cand_offsets must not descend: cand_offsets[%lld] = %lld follows %lld",
                  (long long)(i + 1), (long long)cand_offsets[i + 1], (long long)cand_offsets[i]);
    if (c > nd)
      return fail(PMM_ERR_ARG, "row %lld lists %lld documents, the corpus has %lld: its ids cannot be strictly "
                               "ascending", (long long)i, (long long)c, (long long)nd);
  }
  const int64_t tq = q_offsets[m], total = cand_offsets[m];
  if (tq > INT32_MAX) return fail(PMM_ERR_ARG, "too many query tokens for one call (%lld): split the query rows", (long long)tq);
  if ((tq > 0 && !q_tokens) || (total > 0 && !cand_docs)) return fail(PMM_ERR_ARG, "null argument");
  if (m > (int64_t(1) << 40) / k)
    return fail(PMM_ERR_ARG, "m * k out of range (m=%lld k=%lld): clip k to the longest list first", (long long)m,
                (long long)k);
  if (dp > kMaxsimMaxDp)
    return fail(PMM_ERR_UNSUPPORTED, "MaxSim search serves a padded dimension up to %d (d = %lld pads to %lld)",
                kMaxsimMaxDp, (long long)d, (long long)dp);
  static_assert(kMaxsimMaxDp == PMM_MAXSIM_MAX_DP, "pmm.h states the kernel's limit");

  // Host tables.  Units of the score pass: a row's documents kMaxsimRun at a
  // time.  The sort plan (plan_pieces, cap = k) as candidate search's: a cut
  // row's best min(k, count) keys are merged into a second key array behind
  // the first, where its key source then points.
  const int64_t smax = range_sort_max();
  SortPlan plan;
  plan_pieces(cand_offsets, m, smax, k, plan);
  std::vector<CandUnit> units;
  std::vector<int64_t> src(cand_offsets, cand_offsets + m);
  size_t ci = 0;  // (plan.cut holds the cut rows' pieces in row order)
  for (int64_t i = 0; i < m; i++) {
    const int64_t c = cand_offsets[i + 1] - cand_offsets[i];
    for (int64_t u = 0; u < c; u += kMaxsimRun) units.push_back(CandUnit{(uint32_t)i, (uint32_t)u});
    if (c > smax) {
      src[(size_t)i] = total + plan.cut[ci].dst;
      ci += plan.cut[ci].T;
    }
  }
  const int64_t npieces = (int64_t)plan.po.size() - 1;
  if ((int64_t)units.size() > INT32_MAX || npieces > INT32_MAX)
    return fail(PMM_ERR_ARG, "too many listed documents for one call (%lld): split the query rows", (long long)total);

  const CorpusShard &x = h->shards[0];
  ShardCall f;
  if ((rc = f.open(h))) return rc;
  const hipStream_t s = f.s;
  // arena: query tokens | their norms | flag | token bounds | list bounds | ids
  // | units | piece bounds | piece list | cut pieces | key sources | keys,
  // merged keys | the planes
  Layout L;
  const size_t off_q = L.take((size_t)tq * dp * 4);
  const size_t off_qn = L.take((size_t)tq * 4);
  const size_t off_flag = L.take(4);
  const size_t off_qo = L.take((size_t)(m + 1) * 8);
  const size_t off_offs = L.take((size_t)(m + 1) * 8);
  const size_t off_ids = L.take((size_t)total * 4);
  const size_t off_units = L.take(units.size() * sizeof(CandUnit));
  const size_t off_po = L.take(plan.cut.empty() ? 0 : (size_t)(npieces + 1) * 8);
  const size_t off_mid = L.take(plan.mid.size() * 4);
  const size_t off_cut = L.take(plan.cut.size() * sizeof(CandPiece));
  const size_t off_src = L.take((size_t)m * 8);
  const size_t off_keys = L.take((size_t)(total + plan.merged) * 8);
  const size_t off_oi = L.take((size_t)m * k * 4);
  const size_t off_os = L.take((size_t)m * k * 4);
  const size_t off_len = L.take((size_t)m * 4);
  void *base;
  if ((rc = arena(f.dev, s, L.off, &base))) return rc;
  char *b = (char *)base;
  const float *dq = (const float *)(b + off_q);
  if ((rc = upload_padded(b + off_q, q_tokens, tq, d, dp, 4, s))) return rc;
  // (from here on a failure waits for the stream: the copies read and write this frame's vectors)
  unsigned flag = 0u;
  rc = f.run([&]() -> int {
    HIP_TRY(hipMemsetAsync(b + off_flag, 0, 4, s));
    int64_t *d_offs = (int64_t *)(b + off_offs);
    {
      Timed t("h2d", s);
      HIP_TRY(hipMemcpyAsync(b + off_qo, q_offsets, (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(d_offs, cand_offsets, (size_t)(m + 1) * 8, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(b + off_src, src.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
      if (total > 0) {
        HIP_TRY(hipMemcpyAsync(b + off_ids, cand_docs, (size_t)total * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b + off_units, units.data(), units.size() * sizeof(CandUnit), hipMemcpyHostToDevice,
                               s));
      }
    }
    float *qn = (float *)(b + off_qn);
    if (metric == kMetricCosine && tq > 0) {
      Timed t("norms_f32", s);
      HIP_TRY(launch_norms_f32(dq, tq, d, dp, 0, qn, nullptr, s));
    }
    unsigned long long *keys = (unsigned long long *)(b + off_keys);
    MaxsimScoreArgs sa{};
    sa.q = dq;
    sa.c = x.rows_as<float>();
    sa.qn = qn;
    sa.cn = shard_norms<float>(h, x, metric);
    sa.q_offsets = (const int64_t *)(b + off_qo);
    sa.doc_offsets = h->d_doc_offsets;
    sa.offsets = d_offs;
    sa.ids = (const uint32_t *)(b + off_ids);
    sa.unit = (const CandUnit *)(b + off_units);
    sa.units = (int)units.size();
    sa.ldq = dp;
    sa.ldc = dp;
    sa.n_docs = (uint32_t)nd;
    sa.dp = (int)dp;
    sa.metric = metric;
    sa.keys = keys;
    sa.flag = (unsigned *)(b + off_flag);
    {
      Timed t("maxsim_score", s);
      HIP_TRY(launch_maxsim_score(sa, s));
    }
    if (total > 0)
      if (int rc2 = sort_segments(keys, d_offs, m, plan, (int64_t *)(b + off_po), (int *)(b + off_mid),
                                  (CandPiece *)(b + off_cut), keys + total, s))
        return rc2;
    MaxsimDecodeArgs da{};
    da.keys = keys;
    da.src = (const int64_t *)(b + off_src);
    da.offsets = d_offs;
    da.q_offsets = sa.q_offsets;
    da.m = (int)m;
    da.k = k;
    da.out_idx = (uint32_t *)(b + off_oi);
    da.out_score = (float *)(b + off_os);
    da.out_len = (uint32_t *)(b + off_len);
    {
      Timed t("maxsim_decode", s);
      HIP_TRY(launch_maxsim_decode(da, s));
    }
    {
      Timed t("d2h", s);
      HIP_TRY(hipMemcpyAsync(out_idx, da.out_idx, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_score, da.out_score, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_len, da.out_len, (size_t)m * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(&flag, sa.flag, 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return PMM_OK;
  });
  if (rc) return rc;
  if (flag & 2u) return fail(PMM_ERR_ARG, "a listed id is not a document of the corpus (n_docs=%lld)", (long long)nd);
  if (flag & 1u)
    return fail(PMM_ERR_ARG, "document ids must be strictly ascending within a row (a row repeats or descends)");
  return PMM_OK;
}

// ---- k-means (DESIGN.md §4d "k-means") ----

// Lloyd's iteration on the handle's resident rows: the assignment is the f32
// executor's top-1 with the rows as the queries and the centroids as the
// corpus, the update the ordered f64 gather-sum of pmm_kmeans.hip.  One arena
// for the whole call; one read-back of the changed flag per iteration.
int pmm_kmeans_f32_corpus(const pmm_corpus *h, int64_t K, const float *init, int metric, int64_t max_iter,
                          float *out_centroids, uint32_t *out_labels, float *out_score, int64_t *out_updates,
                          int *out_converged) {
  // every argument check before the handle is read or a device touched
  if (!h) return fail(PMM_ERR_ARG, "null corpus");
  if (!init || !out_centroids || !out_labels || !out_updates || !out_converged)
    return fail(PMM_ERR_ARG, "null argument");
  if (K < 1) return fail(PMM_ERR_ARG, "k-means needs a cluster: K must be >= 1 (got %lld)", (long long)K);
  if (K >= (int64_t(1) << 32)) return fail(PMM_ERR_ARG, "K out of range (%lld): labels are 32 bits wide", (long long)K);
  if (max_iter < 0) return fail(PMM_ERR_ARG, "max_iter must be >= 0 (got %lld)", (long long)max_iter);
  int rc = check_metric(metric);
  if (rc) return rc;
  if (metric == kMetricDot)
    return fail(PMM_ERR_ARG, "k-means takes euclidean or cosine: a mean does not maximise a dot product");
  if (h->partitioned())
    return fail(PMM_ERR_ARG, "k-means takes a plain f32 handle: this one is partitioned (pmm_corpus_partition); "
                             "cluster its parent");
  if (h->dtype != PMM_DTYPE_F32) {
    static const char *const kRows[] = {"f32", "f64", "bf16", "int8", "bit"};
    return fail(PMM_ERR_ARG, "k-means takes an f32 handle: this one holds %s rows", kRows[h->dtype]);
  }
  if (h->shards.size() != 1)
    return fail(PMM_ERR_UNSUPPORTED, "a device-sharded corpus (%d shards) has no k-means: use a handle of one shard",
                (int)h->shards.size());
  const int64_t n = h->n, d = h->d, dp = h->dp;
  if (K > n) return fail(PMM_ERR_ARG, "K (%lld) must be <= n (%lld): more clusters than rows", (long long)K, (long long)n);
  if ((rc = validate_sizes(n, K, d, 1, true))) return rc;
  static_assert(kKmeansPiece == PMM_KMEANS_PIECE, "pmm.h states the piece length");
  const int64_t maxp = kmeans_max_pieces(n, K), units = kmeans_sort_units(n);
  if (maxp * cdiv(dp, 256) > (int64_t)INT32_MAX * 4 || K * cdiv(dp, 256) > INT32_MAX)
    return fail(PMM_ERR_UNSUPPORTED, "too many clusters for one k-means call (K=%lld at d=%lld)", (long long)K,
                (long long)d);

  const CorpusShard &x = h->shards[0];
  ShardCall f;
  if ((rc = f.open(h))) return rc;
  const hipStream_t s = f.s;
  const TopkRoute route = route_topk(n, K, d, 1, metric, PMM_COMPUTE_F32, f.cus, false, false);
  // arena: centroids | their norms and pre-filter factors | top-1 lists | labels
  // | scores | flag | sort keys and rows (two each) | histograms | their scan |
  // bounds | piece bases | piece sums | piece counts | the route's workspace
  Layout L;
  const size_t off_c = L.take((size_t)K * dp * 4);
  const size_t off_cn = L.take((size_t)K * 2 * 4);
  const size_t off_oi = L.take((size_t)n * 4), off_os = L.take((size_t)n * 4);
  const size_t off_lab = L.take((size_t)n * 4), off_sc = L.take((size_t)n * 4);
  const size_t off_flag = L.take(4);
  size_t off_key[2], off_val[2];
  for (int j = 0; j < 2; j++) off_key[j] = L.take((size_t)n * 4), off_val[j] = L.take((size_t)n * 4);
  const size_t off_hist = L.take((size_t)units * 256 * 4), off_base = L.take((size_t)units * 256 * 4);
  const size_t off_bounds = L.take((size_t)(K + 1) * 4), off_pbase = L.take((size_t)(K + 1) * 4);
  const size_t off_psum = L.take((size_t)maxp * dp * 8), off_pcount = L.take((size_t)maxp * 4);
  void *base;
  if ((rc = arena(f.dev, s, L.off + route.total, &base))) return rc;
  char *b = (char *)base;
  float *C = (float *)(b + off_c), *cnrm = (float *)(b + off_cn);
  if ((rc = upload_padded(C, init, K, d, dp, 4, s))) return rc;
  uint32_t *oi = (uint32_t *)(b + off_oi), *labels = (uint32_t *)(b + off_lab);
  float *os = (float *)(b + off_os), *scores = (float *)(b + off_sc);
  unsigned *flag = (unsigned *)(b + off_flag);
  KmeansOrder oa{};
  oa.labels = labels;
  oa.n = n;
  oa.K = (uint32_t)K;
  for (int j = 0; j < 2; j++) oa.key[j] = (uint32_t *)(b + off_key[j]), oa.val[j] = (uint32_t *)(b + off_val[j]);
  oa.hist = (uint32_t *)(b + off_hist);
  oa.base = (uint32_t *)(b + off_base);
  oa.bounds = (uint32_t *)(b + off_bounds);
  oa.pbase = (uint32_t *)(b + off_pbase);
  KmeansUpdateArgs ua{};
  ua.x = x.rows_as<float>();
  ua.ldx = dp;
  ua.cn = metric == kMetricCosine ? shard_norms<float>(h, x, kMetricCosine) : nullptr;
  ua.rows = kmeans_sorted_rows(oa);
  ua.bounds = oa.bounds;
  ua.pbase = oa.pbase;
  ua.K = (uint32_t)K;
  ua.d = (int)d;
  ua.dp = (int)dp;
  ua.max_pieces = maxp;
  ua.psum = (double *)(b + off_psum);
  ua.pcount = (uint32_t *)(b + off_pcount);
  ua.C = C;
  int64_t updates = 0;
  bool converged = false;
  // (a failure waits for the stream: the read-back writes this frame's flag)
  rc = f.run([&]() -> int {
    for (;;) {
      {
        // the centroids' norms and pre-filter factors, by the kernel that made the handle's
        Timed t("norms_f32", s);
        HIP_TRY(launch_norms_f32(C, K, d, dp, metric == kMetricEuclidean, cnrm, cnrm + K, s));
      }
      if (int rc2 = topk_f32_device_impl(route, x.rows_as<float>(), dp, n, C, dp, K, d, 1, metric, 0u, oi, os,
                                         b + L.off, route.total, s, f.dev, cnrm))
        return rc2;
      HIP_TRY(hipMemsetAsync(flag, 0, 4, s));
      {
        Timed t("kmeans_labels", s);
        HIP_TRY(launch_kmeans_labels(oi, os, n, (uint32_t)K, labels, scores, updates > 0, flag, s));
      }
      if (updates > 0) {
        // the iteration's one read-back and wait
        unsigned changed = 0u;
        HIP_TRY(hipMemcpyAsync(&changed, flag, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!changed) {
          converged = true;
          break;
        }
      }
      if (updates == max_iter) break;
      {
        Timed t("kmeans_order", s);
        HIP_TRY(launch_kmeans_order(oa, s));
      }
      {
        Timed t("kmeans_update", s);
        HIP_TRY(launch_kmeans_update(ua, s));
      }
      {
        Timed t("kmeans_finish", s);
        HIP_TRY(launch_kmeans_finish(ua, s));
      }
      updates++;
    }
    Timed t("d2h", s);
    HIP_TRY(hipMemcpy2DAsync(out_centroids, (size_t)d * 4, C, (size_t)dp * 4, (size_t)d * 4, (size_t)K,
                             hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_labels, labels, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_score) HIP_TRY(hipMemcpyAsync(out_score, scores, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    return PMM_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  *out_updates = updates;
  *out_converged = converged ? 1 : 0;
  return PMM_OK;
}

int pmm_screen_prepare_device(const float *a, int64_t ld, int64_t rows, int64_t d, uint16_t *out, int64_t ldo,
                              float *norm, float *inv_norm, float *rel, uint32_t *unsafe, uint32_t *scalars,
                              void *stream) {
  if (rows < 0 || d < 0 || ld < d || ldo < d || ldo % 8 != 0)
    return fail(PMM_ERR_ARG, "bad screen sizes (rows=%lld d=%lld ld=%lld ldo=%lld: ld >= d, ldo >= d a multiple of 8)",
                (long long)rows, (long long)d, (long long)ld, (long long)ldo);
  if (rows == 0) return PMM_OK;
  if (!a || !out) return fail(PMM_ERR_ARG, "null argument");
  if ((uintptr_t)out & 15) return fail(PMM_ERR_ARG, "the bf16 output needs a 16-byte-aligned base");
  int dev, rc;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;  // NULL = the HIP default stream
  Timed t("screen_prepare", s);
  HIP_TRY(launch_screen_prepare(a, rows, d, ld, out, ldo, norm, inv_norm, rel, unsafe, scalars, s));
  return PMM_OK;
}

int pmm_round_bf16_device(const float *a, int64_t ld, int64_t rows, int64_t d, uint16_t *out, int64_t ldo,
                          float *norm, float *inv_norm, float *sq, float *sq_factor, void *stream) {
  if (rows < 0 || d < 0 || ld < d || ldo < d || ldo % 8 != 0)
    return fail(PMM_ERR_ARG, "bad rounding sizes (rows=%lld d=%lld ld=%lld ldo=%lld: ld >= d, ldo >= d a multiple of 8)",
                (long long)rows, (long long)d, (long long)ld, (long long)ldo);
  if (rows == 0) return PMM_OK;
  if (!a || !out) return fail(PMM_ERR_ARG, "null argument");
  if ((uintptr_t)out & 15) return fail(PMM_ERR_ARG, "the bf16 output needs a 16-byte-aligned base");
  int dev, rc;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;  // NULL = the HIP default stream
  Timed t("round_norms_bf16", s);
  HIP_TRY(launch_round_norms_bf16(a, rows, d, ld, out, ldo, norm, inv_norm, sq, sq_factor, s));
  return PMM_OK;
}

int pmm_corpus_create_bf16(const float *c, int64_t n, int64_t d, pmm_corpus **out) {
  return corpus_create(PMM_DTYPE_BF16, c, n, d, out);
}

int pmm_topk_bf16_corpus(const pmm_corpus *h, const float *q, int64_t m, int64_t k, int metric, uint32_t *out_idx,
                         float *out_score) {
  TopkRoute route;
  size_t off_qb = 0, off_qn = 0;
  return corpus_topk(
      h, PMM_DTYPE_BF16, q, m, k, metric, out_idx, out_score,
      [&](const HostCall<float> &f, Layout &L) {
        // the rounded rows, and the query norms outside the route's workspace
        // (topk_bf16_native zeroes its top)
        off_qb = L.take((size_t)m * h->dp * 2), off_qn = L.take((size_t)m * 4);
        // the route pmm_topk_f32_ex's bf16 branch asks for, so the same kernels run
        route = route_topk(m, h->n, h->d, k, metric, PMM_COMPUTE_BF16, g_dev[f.dev].cus, true, true);
        return route.total;
      },
      [&](const HostCall<float> &f) -> int {
        const CorpusShard &x = h->shards[0];
        const int64_t d = h->d, db = h->dp;
        uint16_t *qb = (uint16_t *)(f.b + off_qb);
        // the native route reads the metric's query norms; the widened one computes
        // its own from the widened rows
        float *qn = (metric != kMetricDot && route.kind == Route::kBf16Native) ? (float *)(f.b + off_qn) : nullptr;
        {
          Timed t("round_norms_bf16", f.s);
          HIP_TRY(launch_round_norms_bf16((const float *)f.q, m, d, d, qb, db, metric == kMetricCosine ? qn : nullptr,
                                          nullptr, metric == kMetricEuclidean ? qn : nullptr, nullptr, f.s));
        }
        return topk_bf16_device_impl(route, qb, db, m, x.rows_as<uint16_t>(), db, h->n, d, k, metric, 0u, f.oi, f.os, f.w,
                                     f.ws_bytes, f.s, f.dev, qn, shard_norms<float>(h, x, metric));
      });
}

// ---- int8 rows (DESIGN.md §4d "Int8 rows") ----

size_t pmm_topk_i8_workspace_bytes(int64_t m, int64_t n, int64_t d, int64_t k, int metric) {
  (void)metric;  // (every metric keeps the same buffers)
  if (m <= 0 || n <= 0 || d <= 0 || k <= 0 || d >= kI8DimLimit) return 0;
  return route_i8(m, n, d, k).total;
}

int pmm_topk_i8_device(const int8_t *q, int64_t ldq, int64_t m, const int8_t *c, int64_t ldc, int64_t n, int64_t d,
                       int64_t k, int metric, uint32_t index_base, uint32_t *out_idx, double *out_score,
                       void *workspace, size_t workspace_bytes, void *stream) {
  int rc = validate_i8(m, n, d, k, metric);
  if (rc) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_I8, d);
  if (d == 0 || ldq < dp || ldc < dp || (ldq & 15) || (ldc & 15) || ((uintptr_t)q & 15) || ((uintptr_t)c & 15))
    return fail(PMM_ERR_ARG,
                "device int8 inputs need row strides >= roundup(d, 64) that are multiples of 16 (zero-padded) and "
                "16-byte-aligned bases (d=%lld ldq=%lld ldc=%lld)",
                (long long)d, (long long)ldq, (long long)ldc);
  int dev;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const I8Route route = route_i8(m, n, d, k);
  void *w = workspace;
  if (w) {
    if (workspace_bytes < route.total || ((uintptr_t)w & 255))
      return fail(PMM_ERR_ARG, "the int8 workspace needs %zu bytes at a 256-byte-aligned address (got %zu at %p): "
                               "size it with pmm_topk_i8_workspace_bytes", route.total, workspace_bytes, w);
  } else if ((rc = arena(dev, s, route.total, &w))) {
    return rc;
  }
  rc = topk_i8_device_impl(route, q, ldq, m, c, ldc, n, d, k, metric, index_base, out_idx, out_score, (char *)w, s);
  if (rc) return rc;
  return workspace ? PMM_OK : arena_record(dev, s);
}

int pmm_topk_i8(const int8_t *q, int64_t m, const int8_t *c, int64_t n, int64_t d, int64_t k, int metric,
                uint32_t *out_idx, double *out_score) {
  int rc = validate_i8(m, n, d, k, metric);
  if (rc) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if (d == 0) return fail(PMM_ERR_ARG, "Zero-dimensional vectors");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  // (a device list does not shard int8 rows: the call runs on its first device)
  const int64_t dp = padded_dim(PMM_DTYPE_I8, d);
  const I8Route route = route_i8(m, n, d, k);
  return host_topk(
      nullptr, HostRows{q, m, d, dp, 1}, HostRows{c, n, d, dp, 1}, m, k, out_idx, out_score,
      [&](const HostCall<double> &, Layout &) { return route.total; },
      [&](const HostCall<double> &f) {
        return topk_i8_device_impl(route, (const int8_t *)f.q, dp, m, (const int8_t *)f.c, dp, n, d, k, metric, 0u, f.oi,
                                   f.os, f.w, f.s);
      });
}

int pmm_corpus_create_i8(const int8_t *c, int64_t n, int64_t d, pmm_corpus **out) {
  return corpus_create(PMM_DTYPE_I8, c, n, d, out);
}

int pmm_topk_i8_corpus(const pmm_corpus *h, const int8_t *q, int64_t m, int64_t k, int metric, uint32_t *out_idx,
                       double *out_score) {
  I8Route route;
  return corpus_topk(
      h, PMM_DTYPE_I8, q, m, k, metric, out_idx, out_score,
      [&](const HostCall<double> &, Layout &) {
        route = route_i8(m, h->n, h->d, k);
        return route.total;
      },
      [&](const HostCall<double> &f) {
        const CorpusShard &x = h->shards[0];
        return topk_i8_device_impl(route, (const int8_t *)f.q, h->dp, m, x.rows_as<int8_t>(), h->dp, h->n, h->d, k, metric,
                                   0u, f.oi, f.os, f.w, f.s, (const uint32_t *)x.norms, (const float *)x.norms + h->n);
      });
}

// ---- bit rows (DESIGN.md §4d "Bit rows") ----

int pmm_pack_sign_device(const float *x, int64_t ldx, int64_t rows, int64_t d, uint8_t *out, int64_t ld_out,
                         void *stream) {
  if (rows < 0 || d < 0 || rows > INT32_MAX || d > INT32_MAX - 64)
    return fail(PMM_ERR_ARG, "size out of range (rows=%lld d=%lld)", (long long)rows, (long long)d);
  if (rows == 0) return PMM_OK;
  if (d == 0) return fail(PMM_ERR_ARG, "Zero-dimensional vectors");
  if (int rc = need_buffers(x, out)) return rc;
  const int64_t w8 = cdiv(d, 64) * 8;  // the bytes written per row: whole 8-byte words
  if (ldx < d || ld_out < w8 || (ld_out & 7) || ((uintptr_t)x & 3) || ((uintptr_t)out & 7))
    return fail(PMM_ERR_ARG,
                "sign packing needs ldx >= d at a 4-byte-aligned address and ld_out >= roundup(ceil(d / 8), 8), a "
                "multiple of 8, at an 8-byte-aligned address (d=%lld ldx=%lld ld_out=%lld)",
                (long long)d, (long long)ldx, (long long)ld_out);
  int dev;
  if (int rc = ensure_device(&dev)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Timed t("pack_sign", s);
  HIP_TRY(launch_pack_sign(x, ldx, rows, (int)d, out, ld_out, nullptr, s));
  return PMM_OK;
}

size_t pmm_topk_bits_workspace_bytes(int64_t m, int64_t n, int64_t w, int64_t k) {
  if (m <= 0 || n <= 0 || w <= 0 || k <= 0 || w > kBitsMaxW) return 0;
  return route_bits(m, n, w, k).total;
}

int pmm_topk_bits_device(const uint8_t *q, int64_t ldq, int64_t m, const uint8_t *c, int64_t ldc, int64_t n, int64_t w,
                         int64_t k, uint32_t index_base, uint32_t *out_idx, double *out_score, void *workspace,
                         size_t workspace_bytes, void *stream) {
  int rc = validate_bits(m, n, w, k);
  if (rc) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  const int64_t dp = padded_dim(PMM_DTYPE_BITS, w);
  if (w == 0 || ldq < dp || ldc < dp || (ldq & 15) || (ldc & 15) || ((uintptr_t)q & 15) || ((uintptr_t)c & 15))
    return fail(PMM_ERR_ARG,
                "device bit rows need row strides >= roundup(w, 16) that are multiples of 16 (zero-padded) and "
                "16-byte-aligned bases (w=%lld ldq=%lld ldc=%lld)",
                (long long)w, (long long)ldq, (long long)ldc);
  int dev;
  if ((rc = ensure_device(&dev))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const BitsRoute route = route_bits(m, n, w, k);
  void *ws = workspace;
  if (ws) {
    if (workspace_bytes < route.total || ((uintptr_t)ws & 255))
      return fail(PMM_ERR_ARG, "the bit-row workspace needs %zu bytes at a 256-byte-aligned address (got %zu at %p): "
                               "size it with pmm_topk_bits_workspace_bytes", route.total, workspace_bytes, ws);
  } else if ((rc = arena(dev, s, route.total, &ws))) {
    return rc;
  }
  rc = topk_bits_device_impl(route, q, ldq, m, c, ldc, n, w, k, index_base, out_idx, out_score, (char *)ws, s);
  if (rc) return rc;
  return workspace ? PMM_OK : arena_record(dev, s);
}

int pmm_topk_bits(const uint8_t *q, int64_t m, const uint8_t *c, int64_t n, int64_t w, int64_t k, uint32_t *out_idx,
                  double *out_score) {
  int rc = validate_bits(m, n, w, k);
  if (rc) return rc;
  if (m == 0 || k == 0) return PMM_OK;
  if (n == 0) return fail(PMM_ERR_ARG, "Empty series");
  if (w == 0) return fail(PMM_ERR_ARG, "Zero-dimensional vectors");
  if ((rc = need_buffers(q, c, out_idx, out_score))) return rc;
  // (a device list does not shard bit rows: the call runs on its first device)
  const int64_t dp = padded_dim(PMM_DTYPE_BITS, w);
  const BitsRoute route = route_bits(m, n, w, k);
  return host_topk(
      nullptr, HostRows{q, m, w, dp, 1}, HostRows{c, n, w, dp, 1}, m, k, out_idx, out_score,
      [&](const HostCall<double> &, Layout &) { return route.total; },
      [&](const HostCall<double> &f) {
        return topk_bits_device_impl(route, (const uint8_t *)f.q, dp, m, (const uint8_t *)f.c, dp, n, w, k, 0u, f.oi,
                                     f.os, f.w, f.s);
      });
}

int pmm_corpus_create_bits(const uint8_t *c, int64_t n, int64_t w, pmm_corpus **out) {
  return corpus_create(PMM_DTYPE_BITS, c, n, w, out);
}

// The sign bits of a resident f32 handle's rows, packed on the device from the
// handle's own rows (no upload) with the popcounts from the same pass.  A
// derived parent's index map is copied, so the lists keep the numbering of
// the parent's parent.
int pmm_corpus_sign_bits(const pmm_corpus *p, pmm_corpus **out) {
  if (!out) return fail(PMM_ERR_ARG, "null argument");
  *out = nullptr;
  if (!p) return fail(PMM_ERR_ARG, "null corpus");
  if (p->partitioned())
    return fail(PMM_ERR_ARG, "the parent is a partitioned handle (pmm_corpus_partition): its rows are stored group by "
                             "group; take the sign bits of its parent");
  if (p->dtype != PMM_DTYPE_F32) {
    static const char *const kRows[] = {"f32", "f64", "bf16", "int8", "bit"};
    return fail(PMM_ERR_ARG, "sign bits are taken from an f32 handle: this one holds %s rows", kRows[p->dtype]);
  }
  if (p->shards.size() != 1)
    return fail(PMM_ERR_UNSUPPORTED, "a device-sharded corpus (%d shards) has no sign-bit handle: derive from a handle "
                                     "of one shard", (int)p->shards.size());
  const int64_t w = cdiv(p->d, 8);
  int rc = validate_bits(0, p->n, w, 0);
  if (rc) return rc;
  const CorpusShard &px = p->shards[0];
  int dev;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, px.device))) return rc;
  hipStream_t s;
  if ((rc = thread_stream(dev, &s))) return rc;
  pmm_corpus *h = new pmm_corpus();
  h->n = p->n;
  h->d = w;
  h->dp = padded_dim(PMM_DTYPE_BITS, w);
  h->dtype = PMM_DTYPE_BITS;
  h->shards.resize(1);
  CorpusShard &x = h->shards[0];
  x.device = px.device;
  x.lo = 0;
  x.n = p->n;
  hipError_t e = hipMalloc(&x.rows, (size_t)x.n * h->dp);
  if (e == hipSuccess) e = hipMalloc(&x.norms, (size_t)x.n * 4);
  if (e == hipSuccess && p->map) e = hipMalloc(&h->map, (size_t)x.n * 4);
  if (e != hipSuccess) {
    pmm_corpus_destroy(h);
    return fail(PMM_ERR_HIP, "sign-bit allocation failed on device %d: %s", px.device, hipGetErrorString(e));
  }
  // (the kernel writes roundup(w, 8) bytes of a row; the stride is roundup(w, 16))
  if (h->dp != cdiv(w, 8) * 8) e = hipMemsetAsync(x.rows, 0, (size_t)x.n * h->dp, s);
  if (e == hipSuccess) {
    Timed t("pack_sign", s);
    e = launch_pack_sign(px.rows_as<float>(), p->dp, p->n, (int)p->d, (uint8_t *)x.rows, h->dp, (uint32_t *)x.norms, s);
  }
  if (e == hipSuccess && p->map) e = hipMemcpyAsync(h->map, p->map, (size_t)x.n * 4, hipMemcpyDeviceToDevice, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    pmm_corpus_destroy(h);
    return fail(PMM_ERR_HIP, "sign packing failed: %s", hipGetErrorString(e));
  }
  *out = h;
  return PMM_OK;
}

int pmm_corpus_bits_rows(const pmm_corpus *h, uint8_t *out) {
  if (!h || !out) return fail(PMM_ERR_ARG, "null argument");
  if (h->dtype != PMM_DTYPE_BITS) return wrong_handle(h);
  int dev, rc;
  DevScope scope;
  if ((rc = ensure_device(&dev, &scope, h->shards[0].device))) return rc;
  // (hipMemcpy2D waits for the copy; the handle's rows were complete at creation)
  HIP_TRY(hipMemcpy2D(out, (size_t)h->d, h->shards[0].rows, (size_t)h->dp, (size_t)h->d, (size_t)h->n,
                      hipMemcpyDeviceToHost));
  return PMM_OK;
}

int pmm_topk_bits_corpus(const pmm_corpus *h, const uint8_t *q, int64_t m, int64_t k, uint32_t *out_idx,
                         double *out_score) {
  BitsRoute route;
  return corpus_topk(
      h, PMM_DTYPE_BITS, q, m, k, kMetricEuclidean, out_idx, out_score,
      [&](const HostCall<double> &, Layout &) {
        route = route_bits(m, h->n, h->d, k);
        return route.total;
      },
      [&](const HostCall<double> &f) {
        const CorpusShard &x = h->shards[0];
        return topk_bits_device_impl(route, (const uint8_t *)f.q, h->dp, m, x.rows_as<uint8_t>(), h->dp, h->n, h->d, k, 0u,
                                     f.oi, f.os, f.w, f.s, (const uint32_t *)x.norms);
      });
}

int pmm_timing_enable(int enable) {
  t_ctx.timing = enable != 0;
  return PMM_OK;
}

int pmm_timing_reset(void) {
  for (auto &r : t_ctx.recs) {
    (void)hipEventSynchronize(r.b);
    if ((int)t_ctx.free_events.size() <= r.dev) t_ctx.free_events.resize(r.dev + 1);
    t_ctx.free_events[r.dev].push_back(r.a);
    t_ctx.free_events[r.dev].push_back(r.b);
  }
  t_ctx.recs.clear();
  return PMM_OK;
}

int pmm_timing_read(const char *kernel, double *total_ms, int64_t *launches) {
  double tot = 0.0;
  int64_t cnt = 0;
  for (auto &r : t_ctx.recs) {
    if (kernel && !strstr(r.name, kernel)) continue;
    HIP_TRY(hipEventSynchronize(r.b));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
    tot += ms;
    cnt++;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = cnt;
  return PMM_OK;
}

}  // extern "C"
