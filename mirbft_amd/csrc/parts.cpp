// msha_hash_actions_device: ProcessHashActions (pkg/processor/serial.go:180-198) over
// parts that stay where they are in device memory (include/mirsha.h "ProcessHashActions
// from HBM"). One launch of k_digest_parts (parts_kernels.hip) on the caller's stream;
// the host checks what it can see (null pointers, the arena's base alignment) and the
// kernel reports the rest through the device error word (msha_device_status).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/mirsha.h"
#include "ctx_access.hpp"
#include "kernels.hpp"

namespace {

int hip_fail(msha_ctx* ctx, const char* what, hipError_t e) {
  return msha::ctx_fail(ctx, e == hipErrorOutOfMemory ? MSHA_ERR_OUT_OF_MEMORY : MSHA_ERR_HIP,
                        (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace

extern "C" {

int msha_hash_actions_device(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_part_off,
                             const uint64_t* d_part_len, const uint64_t* d_action_part_begin,
                             const uint32_t* d_order, uint64_t n_actions, uint8_t* d_out, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n_actions == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (!d_arena || !d_part_off || !d_part_len || !d_action_part_begin || !d_out)
    return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  // the kernel reads aligned 16-byte granules of offsets: they must be granules of addresses
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "msha_hash_actions_device: d_arena must be 16-byte aligned");
  msha::CtxDevice d;
  const int rc = msha::ctx_first_device(ctx, &d);
  if (rc != MSHA_OK) return rc;
  const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : d.stream;

  // MSHA_PARTS_TIMING=1 (diagnostic): time the launch with HIP events, which makes the
  // call wait for the kernel; never on a capturing stream
  static const bool timing = msha::env_int("MSHA_PARTS_TIMING", 0) == 1;
  bool timed = false;
  hipError_t e;
  if (timing) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if ((e = hipStreamIsCapturing(st, &cap)) != hipSuccess) return hip_fail(ctx, "hipStreamIsCapturing", e);
    timed = cap == hipStreamCaptureStatusNone;
  }
  EventPair ev;
  if (timed) {
    if ((e = hipEventCreate(&ev.a)) != hipSuccess) return hip_fail(ctx, "hipEventCreate", e);
    if ((e = hipEventCreate(&ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventCreate", e);
    if ((e = hipEventRecord(ev.a, st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
  }
  e = msha::launch_digest_parts(d_arena, d_part_off, d_part_len, d_action_part_begin, d_order, n_actions, d_out,
                                d.err, st);
  if (e != hipSuccess) return hip_fail(ctx, "k_digest_parts launch", e);
  float ms = 0;
  if (timed) {
    if ((e = hipEventRecord(ev.b, st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
    if ((e = hipEventSynchronize(ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventSynchronize", e);
    if ((e = hipEventElapsedTime(&ms, ev.a, ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventElapsedTime", e);
  }
  msha_parts_stats& ps = msha::ctx_parts_stats(ctx);
  ps.calls++;
  ps.actions += n_actions;
  ps.launches++;
  ps.last_lanes = n_actions;
  ps.last_kernel_ms = ms;
  return MSHA_OK;
}

int msha_get_parts_stats(const msha_ctx* ctx, msha_parts_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_parts_stats(const_cast<msha_ctx*>(ctx));
  return MSHA_OK;
}

}  // extern "C"
