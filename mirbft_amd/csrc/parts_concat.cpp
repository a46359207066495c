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
#include "call_workspace.hpp"
#include "parts_concat.hpp"

extern "C" {

int msha_concat_lists_device(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_part_off,
                             const uint64_t* d_part_len, const uint64_t* d_list_part_begin, uint64_t n_lists,
                             const uint32_t* d_select, uint64_t n_select, uint8_t* d_dst, uint64_t dst_bytes,
                             uint64_t* d_msg_off, uint64_t* d_msg_len, void* stream) {
  static const char* const kEntry = "msha_concat_lists_device";
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (n_lists >= 0xffffffffull || n_select >= 0xffffffffull)
    return msha::bad_arg(ctx, kEntry, "n_lists and n_select must be below 2^32 - 1");
  if (!d_select && n_select != n_lists)
    return msha::bad_arg(ctx, kEntry, "without d_select message k is list k: n_select (" + std::to_string(n_select) +
                                          ") must equal n_lists (" + std::to_string(n_lists) + ")");
  if (n_select == 0) return MSHA_OK;
  if (!d_arena || !d_part_off || !d_part_len || !d_list_part_begin || !d_dst || !d_msg_off || !d_msg_len)
    return msha::bad_arg(ctx, kEntry, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_arena must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_dst) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_dst must be 16-byte aligned");

  return msha::guard(ctx, [&] {
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, kEntry, stream, &d);

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
    a.wave_sum_parts = msha::wave_sum_parts();
    // MSHA_CONCAT_SCAN_ONLY (diagnostic, tools/parts_concat_bench.py), read at each call:
    // 1 stops after the scan, so measure and scan can be timed without the copy; 2 runs
    // the scan alone, over whatever d_msg_len and d_msg_off (the flags) hold. No byte of
    // d_dst is written under either.
    const int scan_only = msha::env_int("MSHA_CONCAT_SCAN_ONLY", 0);
    const bool with_measure = scan_only != 2, with_copy = scan_only != 1 && scan_only != 2;

    // under MSHA_PARTS_TIMING=1 the layout is read back too, which makes the call wait
    msha::LaunchTimer timer(st);
    if (with_measure) msha::launch_check(msha::launch_concat_measure(a, st), "k_concat_measure launch");
    msha::launch_check(msha::launch_concat_scan(a, st), "k_concat_scan launch");
    if (with_copy) msha::launch_check(msha::launch_concat_copy(a, st), "k_concat_copy launch");
    const float ms = timer.stop();

    uint64_t last_bytes = 0;
    if (timer.enabled()) {
      // the last valid message's end: refused ones have off = len = 0, and a valid empty
      // message stands where the one before it ended
      std::vector<uint64_t> off(n_select), len(n_select);
      HIPCHK(hipMemcpy(off.data(), d_msg_off, 8 * n_select, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(len.data(), d_msg_len, 8 * n_select, hipMemcpyDeviceToHost));
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
  });
}

int msha_get_concat_stats(const msha_ctx* ctx, msha_concat_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_concat_stats(const_cast<msha_ctx*>(ctx));
  return MSHA_OK;
}

}  // extern "C"
