// msha_group_digests_device: digests grouped by value on the GPU (include/mirsha.h
// "Digests grouped by value on the GPU"; group.hip, group.hpp). Six kernels on the
// caller's stream and nothing else: no memset, no library stream, no host wait. The
// workspace is the context's (call_workspace.hpp GroupState, laid out by group.hpp Layout)
// and follows the workspace rule stated there. The host checks what it can see;
// everything the kernels find is in the caller's arrays, and the device error word is not
// used.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>

#include "../../include/mirsha.h"
#include "call_workspace.hpp"
#include "group.hpp"

static_assert(sizeof(msha_group_result) == 5 * sizeof(uint64_t), "k_group_fill writes the result as five words");

namespace {

const char* const kEntry = "msha_group_digests_device";
using Layout = msha::group::Layout;

// env_int for a 64-bit value (decimal, or hex with 0x), read at each call.
bool env_u64(const char* name, uint64_t* v) {
  const char* e = getenv(name);
  if (!e || !*e) return false;
  *v = std::strtoull(e, nullptr, 0);
  return true;
}

}  // namespace

extern "C" {

int msha_group_digests_device(msha_ctx* ctx, const uint8_t* d_digests, uint64_t n, const uint32_t* d_scope,
                              uint32_t* d_first, uint32_t* d_group, uint32_t* d_members, uint32_t* d_group_first,
                              uint32_t* d_group_count, uint64_t group_cap, msha_group_result* d_result, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (n > msha::group::kMaxSlots) return msha::bad_arg(ctx, kEntry, "n must be at most 2^30");
  if (n == 0) return MSHA_OK;
  if (!d_digests || !d_first || !d_group || !d_result) return msha::bad_arg(ctx, kEntry, "null pointer argument");
  if (group_cap > 0 && (!d_group_first || !d_group_count))
    return msha::bad_arg(ctx, kEntry, "d_group_first or d_group_count is null with group_cap > 0");
  if (reinterpret_cast<uintptr_t>(d_digests) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_digests must be 16-byte aligned");

  return msha::guard(ctx, [&] {
    // a capturing stream allows no allocation: know that before the context's first
    // device call would make one (the error word) or the workspace would grow
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    msha::GroupState& gs = msha::ctx_group_state(ctx);
    const Layout lay(n);
    if (capturing && !msha::ctx_first_device_ready(ctx)) msha::CallWorkspace::refuse(kEntry);
    gs.ws.refuse_growth(kEntry, lay.bytes, capturing);
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, kEntry, stream, capturing, &d);

    uint8_t* ws = gs.ws.acquire(kEntry, lay.bytes, lay.bytes / 4, capturing, st);
    msha::GroupArgs a;
    a.digests = d_digests;
    a.n = n;
    a.scope = d_scope;
    a.first = d_first;
    a.group = d_group;
    a.members = d_members;
    a.group_first = d_group_first;
    a.group_count = d_group_count;
    a.group_cap = group_cap;
    a.result = reinterpret_cast<uint64_t*>(d_result);
    a.head = reinterpret_cast<uint64_t*>(ws + lay.head);
    a.table = reinterpret_cast<uint32_t*>(ws + lay.table);
    a.pos = reinterpret_cast<uint32_t*>(ws + lay.pos);
    a.count = reinterpret_cast<uint32_t*>(ws + lay.count);
    a.id = reinterpret_cast<uint32_t*>(ws + lay.id);
    a.totals = reinterpret_cast<uint32_t*>(ws + lay.totals);
    a.capacity = lay.cap;
    // MSHA_GROUP_SEED and MSHA_GROUP_FORCE_HOME (diagnostics, tests/test_gpu_group.py):
    // another seed, and one home position for every key. No output depends on either.
    a.seed = gs.seed;
    (void)env_u64("MSHA_GROUP_SEED", &a.seed);
    uint64_t at = 0;
    if (env_u64("MSHA_GROUP_FORCE_HOME", &at)) {
      a.force_home = 1;
      a.force_at = (uint32_t)(at % lay.cap);
    }
    // MSHA_GROUP_STOP_AFTER=k (diagnostic, tools/group_bench.py): the first k kernels
    // alone, so that each kernel's share can be timed; the outputs are then incomplete.
    const int stop = msha::env_int("MSHA_GROUP_STOP_AFTER", 0);
    const uint32_t kernels = stop >= 1 && stop < (int)msha::group::kLaunches ? (uint32_t)stop : msha::group::kLaunches;

    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    msha::launch_check(msha::launch_group_init(a, st), "k_group_init launch");
    if (kernels > 1) msha::launch_check(msha::launch_group_insert(a, st), "k_group_insert launch");
    if (kernels > 2) msha::launch_check(msha::launch_group_resolve(a, st), "k_group_resolve launch");
    if (kernels > 3) msha::launch_check(msha::launch_group_scan(a, st), "k_group_scan launch");
    if (kernels > 4) msha::launch_check(msha::launch_group_rank(a, st), "k_group_rank launch");
    if (kernels > 5) msha::launch_check(msha::launch_group_fill(a, st), "k_group_fill launch");
    gs.ws.commit(st, capturing);
    const float ms = timer.stop();

    msha_group_stats& s = gs.stats;
    s.calls++;
    s.digests += n;
    s.launches += kernels;
    s.table_slots = lay.cap;
    s.last_kernel_ms = ms;
  });
}

int msha_get_group_stats(const msha_ctx* ctx, msha_group_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_group_stats(const_cast<msha_ctx*>(ctx));
  return MSHA_OK;
}

}  // extern "C"
