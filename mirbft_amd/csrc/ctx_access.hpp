// What a translation unit outside mirsha.cpp may reach of a context (msha_ctx is
// defined there): its lock, its first device, its error text and what the device
// entries keep in it. Defined at the end of mirsha.cpp; used, through host_call.hpp, by
// streams.cpp, parts.cpp, parts_plan.cpp, parts_concat.cpp, parts_route.cpp and
// stream_device.cpp.
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

// What msha_hash_actions_device_planned (parts_plan.cpp) keeps in the context: its
// device workspace (one allocation, on the first device), the event that orders a call
// after the previous one's use of it, and its counters. Freed by msha_ctx_destroy.
struct PartsPlanState {
  void* ws = nullptr;
  uint64_t ws_bytes = 0;
  hipEvent_t last = nullptr;  // recorded after each call outside capture
  uint64_t last_lists = 0;    // n_lists of the last call (msha_parts_plan_read_order)
  bool ran = false;           // some call has filled the workspace
  msha_parts_plan_stats stats{};
  void release() {
    if (last) {
      (void)hipEventSynchronize(last);
      (void)hipEventDestroy(last);
    }
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    last = nullptr;
    ws_bytes = 0;
  }
};
// Call with the lock held.
PartsPlanState& ctx_parts_plan(msha_ctx* ctx);

// What msha_hash_actions_device_routed (parts_route.cpp) keeps in the context: a
// workspace of its own (the planned call's arrays, the route's slots and the flatten
// buffer in one allocation on the first device: a planned and a routed call share no
// memory), the event that orders a call after the previous one's use of it, where the
// last call's arrays lie in it (msha_parts_route_read*) and its counters. Freed by
// msha_ctx_destroy.
struct PartsRouteState {
  void* ws = nullptr;
  uint64_t ws_bytes = 0;
  hipEvent_t last = nullptr;  // recorded after each call outside capture
  bool ran = false;           // some call has filled the workspace
  uint64_t last_lists = 0, last_slots = 0;               // n_lists and max_long of the last call
  uint64_t at_order = 0, at_chain = 0, at_out_idx = 0, at_claim = 0;  // byte offsets in ws of its arrays
  msha_parts_route_stats stats{};
  void release() {
    if (last) {
      (void)hipEventSynchronize(last);
      (void)hipEventDestroy(last);
    }
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    last = nullptr;
    ws_bytes = 0;
  }
};
// Call with the lock held.
PartsRouteState& ctx_parts_route(msha_ctx* ctx);
// Counts a launch_digest_batch launch of a device entry in msha_stats (the routed
// entry's chain: launches_coop and launches_chain8), as mirsha.cpp's own device entries
// count theirs. kind: the kernels.hpp LaunchKind the launcher reported.
void ctx_count_launch(msha_ctx* ctx, int kind);
// Has a device call already allocated the first device's error word? Until then
// ctx_first_device allocates, which a capturing stream does not allow.
bool ctx_first_device_ready(const msha_ctx* ctx);

}  // namespace msha
