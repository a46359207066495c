// msha_concat_lists_device: part lists flattened into contiguous, 16-byte aligned
// messages on the GPU (include/mirsha.h "Part lists flattened on the GPU";
// parts_concat.hip). Three kernels on the caller's stream and nothing else: no memset,
// no library stream, no host wait, no workspace of the context's. The host checks what
// it can see; the kernels report the rest through the device error word
// (msha_device_status).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/mirsha.h"
#include "ctx_access.hpp"
#include "kernels.hpp"
#include "parts_concat.hpp"
#include "parts_plan.hpp"

namespace {

const char* const kEntry = "msha_concat_lists_device";

int hip_fail(msha_ctx* ctx, const char* what, hipError_t e) {
  return msha::ctx_fail(ctx, e == hipErrorOutOfMemory ? MSHA_ERR_OUT_OF_MEMORY : MSHA_ERR_HIP,
                        (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

int bad_arg(msha_ctx* ctx, const std::string& what) {
  return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, (std::string(kEntry) + ": " + what).c_str());
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

int msha_concat_lists_device(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_part_off,
                             const uint64_t* d_part_len, const uint64_t* d_list_part_begin, uint64_t n_lists,
                             const uint32_t* d_select, uint64_t n_select, uint8_t* d_dst, uint64_t dst_bytes,
                             uint64_t* d_msg_off, uint64_t* d_msg_len, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (n_lists >= 0xffffffffull || n_select >= 0xffffffffull)
    return bad_arg(ctx, "n_lists and n_select must be below 2^32 - 1");
  if (!d_select && n_select != n_lists)
    return bad_arg(ctx, "without d_select message k is list k: n_select (" + std::to_string(n_select) +
                            ") must equal n_lists (" + std::to_string(n_lists) + ")");
  if (n_select == 0) return MSHA_OK;
  if (!d_arena || !d_part_off || !d_part_len || !d_list_part_begin || !d_dst || !d_msg_off || !d_msg_len)
    return bad_arg(ctx, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return bad_arg(ctx, "d_arena must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_dst) % MSHA_DEVICE_ALIGN)
    return bad_arg(ctx, "d_dst must be 16-byte aligned");

  // a capturing stream allows no allocation: know that before the context's first
  // device call would make one (the error word)
  hipError_t e;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (stream && (e = hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cap)) != hipSuccess)
    return hip_fail(ctx, "hipStreamIsCapturing", e);
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (capturing && !msha::ctx_first_device_ready(ctx))
    return bad_arg(ctx, "the context's error word cannot be allocated while the stream is being captured: "
                        "make one call of this size outside the capture first");

  msha::CtxDevice d;
  const int rc = msha::ctx_first_device(ctx, &d);
  if (rc != MSHA_OK) return rc;
  const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : d.stream;

  // MSHA_PARTS_TIMING=1 (diagnostic): time the kernels with HIP events and read the
  // layout back, which makes the call wait; never on a capturing stream
  const bool timed = !capturing && msha::env_int("MSHA_PARTS_TIMING", 0) == 1;
  EventPair ev;
  if (timed) {
    if ((e = hipEventCreate(&ev.a)) != hipSuccess) return hip_fail(ctx, "hipEventCreate", e);
    if ((e = hipEventCreate(&ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventCreate", e);
  }

  msha::ConcatArgs a;
  a.arena = d_arena;
  a.part_off = d_part_off;
  a.part_len = d_part_len;
  a.begin = d_list_part_begin;
  a.n_lists = n_lists;
  a.select = d_select;
  a.n_select = n_select;
  a.dst = d_dst;
  a.dst_bytes = dst_bytes;
  a.msg_off = d_msg_off;
  a.msg_len = d_msg_len;
  a.err = d.err;
  const int t = msha::env_int("MSHA_PARTS_PLAN_WAVE_SUM", (int)msha::parts_plan::kWaveSumParts);
  a.wave_sum_parts = t < 1 ? 1u : (uint32_t)t;

  if (timed && (e = hipEventRecord(ev.a, st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
  // MSHA_CONCAT_SCAN_ONLY (diagnostic, tools/parts_concat_bench.py), read at each call:
  // 1 stops after the scan, so measure and scan can be timed without the copy; 2 runs
  // the scan alone, over whatever d_msg_len and d_msg_off (the flags) hold. No byte of
  // d_dst is written under either.
  const int scan_only = msha::env_int("MSHA_CONCAT_SCAN_ONLY", 0);
  const bool with_measure = scan_only != 2, with_copy = scan_only != 1 && scan_only != 2;
  if (with_measure && (e = msha::launch_concat_measure(a, st)) != hipSuccess)
    return hip_fail(ctx, "k_concat_measure launch", e);
  if ((e = msha::launch_concat_scan(a, st)) != hipSuccess) return hip_fail(ctx, "k_concat_scan launch", e);
  if (with_copy && (e = msha::launch_concat_copy(a, st)) != hipSuccess)
    return hip_fail(ctx, "k_concat_copy launch", e);

  float ms = 0;
  uint64_t last_bytes = 0;
  if (timed) {
    if ((e = hipEventRecord(ev.b, st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
    if ((e = hipEventSynchronize(ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventSynchronize", e);
    if ((e = hipEventElapsedTime(&ms, ev.a, ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventElapsedTime", e);
    // the last valid message's end: refused ones have off = len = 0, and a valid empty
    // message stands where the one before it ended
    std::vector<uint64_t> off(n_select), len(n_select);
    if ((e = hipMemcpy(off.data(), d_msg_off, 8 * n_select, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(len.data(), d_msg_len, 8 * n_select, hipMemcpyDeviceToHost)) != hipSuccess)
      return hip_fail(ctx, "hipMemcpy", e);
    for (uint64_t k = n_select; k-- > 0;)
      if (off[k] | len[k]) {
        last_bytes = off[k] + msha::parts_concat::round16(len[k]);
        break;
      }
  }
  msha_concat_stats& s = msha::ctx_concat_stats(ctx);
  s.calls++;
  s.lists += n_select;
  s.launches += 1 + (with_measure ? 1 : 0) + (with_copy ? 1 : 0);
  s.last_bytes = last_bytes;
  s.last_kernel_ms = ms;
  return MSHA_OK;
}

int msha_get_concat_stats(const msha_ctx* ctx, msha_concat_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_concat_stats(const_cast<msha_ctx*>(ctx));
  return MSHA_OK;
}

}  // extern "C"
