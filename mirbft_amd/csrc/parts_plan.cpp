// msha_hash_actions_device_planned: multi-part actions named through part lists
// (include/mirsha.h "Multi-part actions through part LISTS"), folded and ordered on the
// GPU inside the call (parts_plan.hip). Its kernels all go on the caller's stream (the
// first resets the workspace: there is no memset); the workspace is the context's (ctx_access.hpp PartsPlanState) and grows
// only outside stream capture. The host checks what it can see; the kernels report the
// rest through the device error word (msha_device_status).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/mirsha.h"
#include "host_call.hpp"
#include "parts_plan.hpp"

namespace {

const char* const kEntry = "msha_hash_actions_device_planned";

uint64_t round64(uint64_t x) { return (x + 63) & ~uint64_t(63); }

// The workspace of a call over n lists: info (16 words) and the counters, one array to
// k_parts_init; then the order, at an offset that does not depend on n
// (msha_parts_plan_read_order reads it after the call); then the keys, the used flags
// and the digest table.
struct Layout {
  uint64_t zero_bytes, order, key16, used, table, bytes;
  Layout(uint64_t n, bool with_list) {
    zero_bytes = round64(4ull * (16 + msha::parts_plan::kKeys));
    order = zero_bytes;
    key16 = order + round64(4 * n);
    used = key16 + round64(2 * n);
    table = used + (with_list ? round64(n) : 0);
    bytes = table + (with_list ? 32 * n : 0) + 64;
  }
};

}  // namespace

extern "C" {

int msha_hash_actions_device_planned(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_part_off,
                                     const uint64_t* d_part_len, const uint64_t* d_list_part_begin,
                                     uint64_t n_lists, const uint32_t* d_action_list, uint64_t n_actions,
                                     uint32_t flags, uint8_t* d_out, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (flags & ~(uint32_t)MSHA_PARTS_FOLD) return msha::bad_arg(ctx, kEntry, "unknown flags " + std::to_string(flags));
  if (n_lists >= 0xffffffffull || n_actions >= 0xffffffffull)
    return msha::bad_arg(ctx, kEntry, "n_lists and n_actions must be below 2^32 - 1");
  if (!d_action_list && n_actions != n_lists)
    return msha::bad_arg(ctx, kEntry, "without d_action_list action i is list i: n_actions (" +
                                          std::to_string(n_actions) + ") must equal n_lists (" +
                                          std::to_string(n_lists) + ")");
  if (n_actions == 0) return MSHA_OK;
  if (!d_arena || !d_part_off || !d_part_len || !d_list_part_begin || !d_out)
    return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_arena must be 16-byte aligned");

  return msha::guard(ctx, [&] {
    // a capturing stream allows no allocation: know that before the context's first
    // device call would make one (the error word) or the workspace would grow
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    msha::PartsPlanState& ps = msha::ctx_parts_plan(ctx);
    const Layout lay(n_lists, d_action_list != nullptr);
    if (capturing && (!msha::ctx_first_device_ready(ctx) || lay.bytes > ps.ws_bytes))
      throw msha::MshaError(MSHA_ERR_INVALID_ARG,
                            std::string(kEntry) + ": the workspace cannot grow while the stream is being captured: "
                                                  "make one call of this size outside the capture first");
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, kEntry, stream, capturing, &d);

    if (lay.bytes > ps.ws_bytes) {
      // an earlier call may still be using the old buffer
      if (ps.last) HIPCHK(hipEventSynchronize(ps.last));
      if (ps.ws) HIPCHK(hipFree(ps.ws));
      ps.ws = nullptr;
      ps.ws_bytes = 0;
      ps.ran = false;
      const uint64_t want = lay.bytes + lay.bytes / 4;
      HIPCHK(hipMalloc(&ps.ws, want));
      ps.ws_bytes = want;
    }
    if (!ps.last && !capturing) HIPCHK(hipEventCreateWithFlags(&ps.last, hipEventDisableTiming));
    // two streams must not race on the workspace: after the previous call's last kernel
    if (!capturing && ps.ran) HIPCHK(hipStreamWaitEvent(st, ps.last, 0));

    uint8_t* ws = static_cast<uint8_t*>(ps.ws);
    msha::PartsPlanArgs a;
    a.arena = d_arena;
    a.part_off = d_part_off;
    a.part_len = d_part_len;
    a.begin = d_list_part_begin;
    a.n_lists = n_lists;
    a.action_list = d_action_list;
    a.n_actions = n_actions;
    a.info = reinterpret_cast<uint32_t*>(ws);
    a.cnt = a.info + 16;
    a.order = reinterpret_cast<uint32_t*>(ws + lay.order);
    a.key16 = reinterpret_cast<uint16_t*>(ws + lay.key16);
    a.used = d_action_list ? ws + lay.used : nullptr;
    a.table = d_action_list ? ws + lay.table : nullptr;
    a.out = d_out;
    a.err = d.err;
    const int t = msha::env_int("MSHA_PARTS_PLAN_WAVE_SUM", (int)msha::parts_plan::kWaveSumParts);
    a.wave_sum_parts = t < 1 ? 1u : (uint32_t)t;
    // MSHA_PARTS_PLAN_ONLY=1 (diagnostic, tools/parts_plan_bench.py): stop after the
    // scatter, so the plan kernels can be timed alone; no digest is written
    const bool plan_only = msha::env_int("MSHA_PARTS_PLAN_ONLY", 0) == 1;

    // under MSHA_PARTS_TIMING=1 the lane and block counts are read back too, which makes
    // the call wait
    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    uint32_t plan_launches = 0;
    msha::launch_check(msha::launch_parts_plan(a, st, &plan_launches), "parts plan launch");
    if (!plan_only) msha::launch_check(msha::launch_digest_parts_planned(a, st), "k_digest_parts_planned launch");
    if (!plan_only && d_action_list) msha::launch_check(msha::launch_parts_fill(a, st), "k_parts_fill launch");
    ps.ran = true;
    ps.last_lists = n_lists;
    if (!capturing) HIPCHK(hipEventRecord(ps.last, st));

    const float ms = timer.stop();
    uint32_t info[4] = {0, 0, 0, 0};
    if (timer.enabled()) HIPCHK(hipMemcpy(info, a.info, sizeof info, hipMemcpyDeviceToHost));
    msha_parts_plan_stats& s = ps.stats;
    s.calls++;
    s.actions += n_actions;
    s.lists += n_lists;
    s.launches_plan += plan_launches;
    if (!plan_only) s.launches_hash++;
    if (!plan_only && d_action_list) s.launches_fill++;
    s.last_lanes = info[0];
    s.last_blocks = (uint64_t)info[3] << 32 | info[2];
    s.last_kernel_ms = ms;
  });
}

int msha_get_parts_plan_stats(const msha_ctx* ctx, msha_parts_plan_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_parts_plan(const_cast<msha_ctx*>(ctx)).stats;
  return MSHA_OK;
}

int msha_parts_plan_read_order(msha_ctx* ctx, uint32_t* order, uint64_t cap, uint64_t* lanes) {
  if (!ctx || !lanes || (cap && !order)) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  msha::PartsPlanState& ps = msha::ctx_parts_plan(ctx);
  *lanes = 0;
  if (!ps.ran) return MSHA_OK;
  return msha::guard(ctx, [&] {
    (void)msha::ctx_first_device(ctx);
    HIPCHK(hipDeviceSynchronize());
    const uint8_t* ws = static_cast<const uint8_t*>(ps.ws);
    uint32_t n = 0;
    HIPCHK(hipMemcpy(&n, ws, 4, hipMemcpyDeviceToHost));
    if (n > ps.last_lists) n = (uint32_t)ps.last_lists;  // the order holds last_lists positions
    *lanes = n;
    const uint64_t k = n < cap ? n : cap;
    const Layout lay(ps.last_lists, false);
    if (k) HIPCHK(hipMemcpy(order, ws + lay.order, 4 * k, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
