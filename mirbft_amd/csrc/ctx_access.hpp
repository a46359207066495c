// What a translation unit outside mirsha.cpp may reach of a context (msha_ctx is
// defined there): its lock, its first device, its error text. Defined in
// mirsha.cpp; used by the stream sets (streams.cpp).
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
// The context's first device, made current, with its error word allocated. Returns
// MSHA_OK, or an MSHA_ERR_* code with the context's error text set. Call with the
// lock held.
int ctx_first_device(msha_ctx* ctx, CtxDevice* out);
// Sets the context's error text and returns code (msg null: clears the text).
int ctx_fail(msha_ctx* ctx, int code, const char* msg);
// The counters of msha_hash_actions_device (parts.cpp). Call with the lock held.
msha_parts_stats& ctx_parts_stats(msha_ctx* ctx);

}  // namespace msha
