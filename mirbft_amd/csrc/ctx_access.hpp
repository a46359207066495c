// What a translation unit that does not include ctx.hpp may reach of a context (msha_ctx
// is defined there): its lock, its first device, its error text and what the device
// entries keep in it (the states by name only: call_workspace.hpp defines them). Defined
// at the end of ctx.cpp; used, through host_call.hpp, by streams.cpp, parts.cpp,
// parts_plan.cpp, parts_concat.cpp, parts_route.cpp, stream_device.cpp, verify.cpp,
// group.cpp and dmap.cpp. The host paths and device_batch.cpp include ctx.hpp and see the context itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/mirsha.h"

struct msha_ctx;

namespace msha {

struct CtxDevice {
  int id = 0;                    // HIP device
  int cus = 0;
  hipStream_t stream = nullptr;  // the context's own stream on that device
  uint32_t* err = nullptr;       // the device error word msha_device_status reports (zeroed on first use)
};

// The lock every call on the context takes.
std::mutex& ctx_mutex(const msha_ctx* ctx);
// The context's first device, made current, with its error word allocated. Throws
// (host_call.hpp MshaError): call inside guard(), with the lock held.
CtxDevice ctx_first_device(msha_ctx* ctx);
// Sets the context's error text and returns code (msg null: clears the text).
int ctx_fail(msha_ctx* ctx, int code, const char* msg);
// The counters of msha_hash_actions_device (parts.cpp). Call with the lock held.
msha_parts_stats& ctx_parts_stats(msha_ctx* ctx);
// The counters of msha_concat_lists_device (parts_concat.cpp). Call with the lock held.
msha_concat_stats& ctx_concat_stats(msha_ctx* ctx);
// The counters of msha_verify_digests_device (verify.cpp). Call with the lock held.
msha_verify_stats& ctx_verify_stats(msha_ctx* ctx);

// What msha_hash_actions_device_planned and _routed keep in the context. Call with the lock held.
struct PartsPlanState;
struct PartsRouteState;
PartsPlanState& ctx_parts_plan(msha_ctx* ctx);
PartsRouteState& ctx_parts_route(msha_ctx* ctx);
// What msha_group_digests_device keeps in the context (group.cpp): workspace, seed and
// counters. Call with the lock held.
struct GroupState;
GroupState& ctx_group_state(msha_ctx* ctx);
msha_group_stats& ctx_group_stats(msha_ctx* ctx);
// Counts a launch_digest_batch launch of a device entry in msha_stats (the routed
// entry's chain: launches_coop and launches_chain8), as device_batch.cpp's entries
// count theirs. kind: the kernels.hpp LaunchKind the launcher reported.
void ctx_count_launch(msha_ctx* ctx, int kind);
// Has a device call already allocated the first device's error word? Until then
// ctx_first_device allocates, which a capturing stream does not allow.
bool ctx_first_device_ready(const msha_ctx* ctx);

}  // namespace msha
