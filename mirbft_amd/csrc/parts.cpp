// msha_hash_actions_device: ProcessHashActions (pkg/processor/serial.go:180-198) over
// parts that stay where they are in device memory (include/mirsha.h "ProcessHashActions
// from HBM"). One launch of k_digest_parts (parts_kernels.hip) on the caller's stream;
// the host checks what it can see (null pointers, the arena's base alignment) and the
// kernel reports the rest through the device error word (msha_device_status).
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/mirsha.h"
#include "host_call.hpp"

extern "C" {

int msha_hash_actions_device(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_part_off,
                             const uint64_t* d_part_len, const uint64_t* d_action_part_begin,
                             const uint32_t* d_order, uint64_t n_actions, uint8_t* d_out, void* stream) {
  static const char* const kEntry = "msha_hash_actions_device";
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n_actions == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (!d_arena || !d_part_off || !d_part_len || !d_action_part_begin || !d_out)
    return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  // the kernel reads aligned 16-byte granules of offsets: they must be granules of addresses
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_arena must be 16-byte aligned");
  return msha::guard(ctx, [&] {
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, kEntry, stream, &d);
    msha::LaunchTimer timer(st);
    msha::launch_check(msha::launch_digest_parts(d_arena, d_part_off, d_part_len, d_action_part_begin, d_order,
                                                 n_actions, d_out, d.err, st),
                       "k_digest_parts launch");
    const float ms = timer.stop();
    msha_parts_stats& ps = msha::ctx_parts_stats(ctx);
    ps.calls++;
    ps.actions += n_actions;
    ps.launches++;
    ps.last_lanes = n_actions;
    ps.last_kernel_ms = ms;
  });
}

int msha_get_parts_stats(const msha_ctx* ctx, msha_parts_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_parts_stats(const_cast<msha_ctx*>(ctx));
  return MSHA_OK;
}

}  // extern "C"
