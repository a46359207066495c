// msha_hash_actions_device_planned: multi-part actions named through part lists
// (include/mirsha.h "Multi-part actions through part LISTS"), folded and ordered on the
// GPU inside the call (parts_plan.hip). Its kernels all go on the caller's stream (the
// first resets the workspace: there is no memset); the workspace is the context's
// (call_workspace.hpp PartsPlanState, laid out by parts_plan.hpp Layout) and follows the
// workspace rule stated there. The host checks what it can see; the kernels report the
// rest through the device error word (msha_device_status).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/mirsha.h"
#include "call_workspace.hpp"

namespace {

const char* const kEntry = "msha_hash_actions_device_planned";
using Layout = msha::parts_plan::Layout;

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
    if (capturing && !msha::ctx_first_device_ready(ctx)) msha::CallWorkspace::refuse(kEntry);
    ps.ws.refuse_growth(kEntry, lay.bytes, capturing);
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, kEntry, stream, capturing, &d);

    uint8_t* ws = ps.ws.acquire(kEntry, lay.bytes, lay.bytes / 4, capturing, st);
    const msha::PartsPlanArgs a = msha::plan_args(d_arena, d_part_off, d_part_len, d_list_part_begin, n_lists,
                                                  d_action_list, n_actions, d_out, d.err, ws, lay);
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
    ps.last_lists = n_lists;
    ps.ws.commit(st, capturing);

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
  return msha::read_plan_order(ctx, ps.ws, ps.last_lists, Layout(ps.last_lists, false).order, order, cap, lanes);
}

}  // extern "C"
