// Host-side state of the library, no kernels: the last-error string, the option table with its per-stream overrides, the tile-scheduler
// block pairs of the persistent GEMM grids, check_launch, and the alpro_hip_* entry points that serve them.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.hpp"

namespace alpro {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {
const char* const kOptNames[OPT_COUNT] = {"gemm_tile", "gemm_grid", "gemm_tune", "tn_splits", "tn_kind", "gemm_tail", "attn_bwd", "attn_order", "gemm_kind", "cu_budget", "ln_grid", "gemm_sched", "gemm_epi"};
const char* const kOptEnv[OPT_COUNT] = {"ALPRO_GEMM_TILE", "ALPRO_GEMM_GRID", "ALPRO_GEMM_TUNE", "ALPRO_TN_SPLITS", "ALPRO_TN_KIND", "ALPRO_GEMM_TAIL", "ALPRO_ATTN_BWD", "ALPRO_ATTN_ORDER", "ALPRO_GEMM_KIND", "ALPRO_CU_BUDGET", "ALPRO_LN_GRID", "ALPRO_GEMM_SCHED", "ALPRO_GEMM_EPI"};
int g_opts[OPT_COUNT];
// Values that once selected ablations (gemm_tune >= 3, tn_kind 1, attn_bwd 3 / 4: measurement variants that have been removed) are
// refused, from alpro_hip_set_option, alpro_hip_set_stream_option and the environment alike.
bool option_allowed(int which, int value) {
  if (which == OPT_GEMM_TUNE) return value >= 0 && value <= 2;
  if (which == OPT_TN_KIND) return value == 0 || value == 2;   // 0: one group, 2: two-group schedule
  if (which == OPT_ATTN_BWD) return value >= 0 && value <= 2;   // 0 two-phase, 1 best per shape, 2 key-owned
  return value >= 0;
}
struct OptInit {
  OptInit() {
    for (int i = 0; i < OPT_COUNT; ++i) {
      const char* e = getenv(kOptEnv[i]);
      const int dflt = (i == OPT_GEMM_TUNE || i == OPT_GEMM_TAIL || i == OPT_ATTN_BWD || i == OPT_GEMM_KIND || i == OPT_GEMM_SCHED || i == OPT_GEMM_EPI) ? 1
                       : i == OPT_TN_KIND ? 2   // (round 5: the two-group schedule of the weight-gradient kernel, -1.2 % on its 29.7 ms in the step: profiles/r5_tn_kind_ab.txt)
                                          : 0;
      g_opts[i] = e ? atoi(e) : dflt;
      if (!option_allowed(i, g_opts[i])) {
        fprintf(stderr, "libalpro_hip: %s=%d selected an ablation that has been removed (ignored)\n", kOptEnv[i], g_opts[i]);
        g_opts[i] = dflt;
      }
    }
  }
} g_opt_init;
}  // namespace

int get_option(int which) { return __atomic_load_n(&g_opts[which], __ATOMIC_RELAXED); }

// ---- per-stream option overrides (round 5) ---------------------------------------------------------------------------------------
// A handful of (stream, option) -> value entries behind a spin lock: set by the owner of a stream (alpro_amd.optim while its gradient
// exchange is in flight), read once per launch that consults the option.  An empty table (the normal case) costs one relaxed load.
namespace {
struct StreamOpt { hipStream_t st; int which, value; };
constexpr int kMaxStreamOpts = 32;
StreamOpt g_sopts[kMaxStreamOpts];
int g_nsopts = 0;
int g_sopt_lock = 0;
struct SpinGuard {
  SpinGuard() { while (__atomic_exchange_n(&g_sopt_lock, 1, __ATOMIC_ACQUIRE)) {} }
  ~SpinGuard() { __atomic_store_n(&g_sopt_lock, 0, __ATOMIC_RELEASE); }
};
}  // namespace

int get_stream_option(int which, hipStream_t st) {
  if (__atomic_load_n(&g_nsopts, __ATOMIC_RELAXED) == 0) return -1;
  SpinGuard g;
  for (int i = 0; i < g_nsopts; ++i)
    if (g_sopts[i].st == st && g_sopts[i].which == which) return g_sopts[i].value;
  return -1;
}

// ---- tile-scheduler blocks (common.hpp) ---------------------------------------------------------------------------------------------
// Who owns the memory.  Each (device, stream) that launches the persistent 8-phase GEMM needs one PAIR of counter blocks (2 x 1056 bytes).
//   * A caller that wants the library to allocate nothing registers its own: alpro_hip_set_sched_workspace(stream, ptr, bytes).
//   * Otherwise the first such launch on a device makes ONE hipMalloc of kSchedSlots pairs (135 KB) for that device -- the only allocation
//     this library ever makes -- and the stream's pair is cleared by a hipMemsetAsync ON THAT STREAM (ordered before the launch; no device-wide
//     synchronisation, round 6).
// A slot belongs to its (device, stream) until alpro_hip_release_stream(stream): a destroyed stream's handle value may be handed out again
// by the runtime, so owners of short-lived streams release them (the re-created stream then starts from a cleared pair instead of
// inheriting one).  With all kSchedSlots slots taken a further stream runs the static walk (same results, no CU-theft tolerance).
namespace {
constexpr int kSchedSlots = 64;
struct SchedSlot {
  int dev;
  hipStream_t st;
  uint32_t* pair;   // 2 x SCHED_BLOCK_U32 dwords
  unsigned n;       // launches committed on this pair: launch n works on block n & 1 and zeroes the other
  int lock;
  bool used, caller_owned;
};
SchedSlot g_sched[kSchedSlots];
int g_sched_table_lock = 0;
uint32_t* g_sched_pool[64];   // per device: kSchedSlots pairs (slot i's pair is pool + i * pair size)
constexpr size_t kPairBytes = (size_t)2 * SCHED_BLOCK_U32 * sizeof(uint32_t);
struct TableGuard {
  TableGuard() { while (__atomic_exchange_n(&g_sched_table_lock, 1, __ATOMIC_ACQUIRE)) {} }
  ~TableGuard() { __atomic_store_n(&g_sched_table_lock, 0, __ATOMIC_RELEASE); }
};
SchedSlot* find_slot(int dev, hipStream_t st) {
  for (int i = 0; i < kSchedSlots; ++i)
    if (g_sched[i].used && g_sched[i].dev == dev && g_sched[i].st == st) return &g_sched[i];
  return nullptr;
}
// a free slot for (dev, st) on `pair` (nullptr: the device pool's), cleared on the stream; nullptr when the table is full / the pool cannot be made
SchedSlot* make_slot(int dev, hipStream_t st, uint32_t* pair) {
  int at = -1;
  for (int i = 0; i < kSchedSlots && at < 0; ++i)
    if (!g_sched[i].used) at = i;
  if (at < 0) return nullptr;
  const bool own = pair != nullptr;
  if (!own) {
    if (!g_sched_pool[dev]) {
      void* pmem = nullptr;
      if (hipMalloc(&pmem, kSchedSlots * kPairBytes) == hipSuccess) g_sched_pool[dev] = (uint32_t*)pmem;
      else (void)hipGetLastError();
    }
    if (!g_sched_pool[dev]) return nullptr;
    pair = g_sched_pool[dev] + (size_t)at * 2 * SCHED_BLOCK_U32;
  }
  if (hipMemsetAsync(pair, 0, kPairBytes, st) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  SchedSlot* s = &g_sched[at];
  s->dev = dev;
  s->st = st;
  s->pair = pair;
  s->n = 0;
  s->lock = 0;
  s->caller_owned = own;
  s->used = true;
  return s;
}
}  // namespace

SchedLaunch::SchedLaunch(hipStream_t st, bool enabled) {
  if (!enabled) return;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {   // a captured launch is replayed with the SAME block: static walk
    (void)hipGetLastError();
    return;
  }
  SchedSlot* s = nullptr;
  {
    TableGuard g;
    s = find_slot(dev, st);
    if (!s) s = make_slot(dev, st, nullptr);
  }
  if (!s) return;
  while (__atomic_exchange_n(&s->lock, 1, __ATOMIC_ACQUIRE)) {}
  slot = s;
  cur = s->pair + (size_t)(s->n & 1u) * SCHED_BLOCK_U32;
  prev = s->pair + (size_t)((s->n + 1u) & 1u) * SCHED_BLOCK_U32;
}

// The pair's parity moves on only when the launch was accepted: a launch that failed at enqueue never ran, so `cur` is still
// clear and `prev` still holds the previous launch's counts -- exactly what the next attempt expects.
void SchedLaunch::commit(bool launched) {
  if (slot && launched) ++((SchedSlot*)slot)->n;
}

SchedLaunch::~SchedLaunch() {
  if (slot) __atomic_store_n(&((SchedSlot*)slot)->lock, 0, __ATOMIC_RELEASE);
}

int sched_set_workspace(hipStream_t st, void* ptr, size_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { set_error("alpro_hip_set_sched_workspace: no current device"); return ALPRO_ERR_INVALID; }
  TableGuard g;
  SchedSlot* s = find_slot(dev, st);
  if (s) {   // (the stream's launches so far are ordered before the clear make_slot() issues on it)
    while (__atomic_exchange_n(&s->lock, 1, __ATOMIC_ACQUIRE)) {}
    s->used = false;
    __atomic_store_n(&s->lock, 0, __ATOMIC_RELEASE);
  }
  if (!ptr) return ALPRO_OK;
  if (bytes < kPairBytes || ((uintptr_t)ptr % 16) != 0) { set_error("alpro_hip_set_sched_workspace: needs %zu bytes, 16-byte aligned (got %zu)", kPairBytes, bytes); return ALPRO_ERR_INVALID; }
  if (!make_slot(dev, st, (uint32_t*)ptr)) { set_error("alpro_hip_set_sched_workspace: all %d (device, stream) slots are taken: release a stream first", kSchedSlots); return ALPRO_ERR_INVALID; }
  return ALPRO_OK;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return ALPRO_ERR_LAUNCH;
  }
  return ALPRO_OK;
}

}  // namespace alpro

using namespace alpro;

extern "C" const char* alpro_hip_last_error(void) { return g_err; }
extern "C" int alpro_hip_abi_version(void) { return ALPRO_HIP_ABI_VERSION; }
extern "C" int alpro_hip_set_option(const char* name, int value) {
  using namespace alpro;
  for (int i = 0; name && i < OPT_COUNT; ++i)
    if (!strcmp(name, kOptNames[i])) {
      if (!option_allowed(i, value)) {
        set_error("alpro_hip_set_option: %s=%d selected an ablation that has been removed; it is not a valid value", name, value);
        return ALPRO_ERR_INVALID;
      }
      __atomic_store_n(&g_opts[i], value, __ATOMIC_RELAXED);
      return ALPRO_OK;
    }
  set_error("alpro_hip_set_option: unknown option '%s'", name ? name : "(null)");
  return ALPRO_ERR_INVALID;
}

extern "C" int alpro_hip_set_stream_option(void* stream, const char* name, int value) {
  using namespace alpro;
  int which = -1;
  for (int i = 0; name && i < OPT_COUNT; ++i)
    if (!strcmp(name, kOptNames[i])) which = i;
  if (which < 0) {
    set_error("alpro_hip_set_stream_option: unknown option '%s'", name ? name : "(null)");
    return ALPRO_ERR_INVALID;
  }
  if (value >= 0 && !option_allowed(which, value)) {
    set_error("alpro_hip_set_stream_option: %s=%d selected an ablation that has been removed; it is not a valid value", name, value);
    return ALPRO_ERR_INVALID;
  }
  SpinGuard g;
  int at = -1;
  for (int i = 0; i < g_nsopts; ++i)
    if (g_sopts[i].st == (hipStream_t)stream && g_sopts[i].which == which) at = i;
  if (value < 0) {   // clear the override
    if (at >= 0) {
      g_sopts[at] = g_sopts[g_nsopts - 1];
      __atomic_store_n(&g_nsopts, g_nsopts - 1, __ATOMIC_RELAXED);
    }
    return ALPRO_OK;
  }
  if (at < 0) {
    if (g_nsopts == kMaxStreamOpts) {
      set_error("alpro_hip_set_stream_option: more than %d (stream, option) overrides", kMaxStreamOpts);
      return ALPRO_ERR_INVALID;
    }
    at = g_nsopts;
    g_sopts[at].st = (hipStream_t)stream;
    g_sopts[at].which = which;
    g_sopts[at].value = value;
    __atomic_store_n(&g_nsopts, g_nsopts + 1, __ATOMIC_RELAXED);
  }
  g_sopts[at].value = value;
  return ALPRO_OK;
}

extern "C" size_t alpro_hip_sched_workspace_bytes(void) { return (size_t)2 * alpro::SCHED_BLOCK_U32 * sizeof(uint32_t); }

extern "C" int alpro_hip_set_sched_workspace(void* stream, void* ptr, size_t bytes) { return alpro::sched_set_workspace((hipStream_t)stream, ptr, bytes); }

extern "C" int alpro_hip_release_stream(void* stream) {
  using namespace alpro;
  {   // every per-stream option override of that stream
    SpinGuard g;
    for (int i = 0; i < g_nsopts;) {
      if (g_sopts[i].st == (hipStream_t)stream) {
        g_sopts[i] = g_sopts[g_nsopts - 1];
        __atomic_store_n(&g_nsopts, g_nsopts - 1, __ATOMIC_RELAXED);
      } else {
        ++i;
      }
    }
  }
  return sched_set_workspace((hipStream_t)stream, nullptr, 0);   // ... and its tile-scheduler slot (a caller-owned workspace is simply forgotten)
}
