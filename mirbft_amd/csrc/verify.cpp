// msha_verify_digests_device: digests compared on the GPU with the ones the caller
// expects (include/mirsha.h "Digests verified on the GPU"; verify.hip). Two kernels on the
// caller's stream and nothing else: no memset, no library stream, no host wait, no
// workspace of the context's. The host checks what it can see; everything the kernels
// find is in the caller's d_result, and the device error word is not used.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/mirsha.h"
#include "host_call.hpp"
#include "verify.hpp"

static_assert(sizeof(msha_verify_result) == 5 * sizeof(uint64_t), "k_verify_scan writes the result as five words");

extern "C" {

int msha_verify_digests_device(msha_ctx* ctx, const uint8_t* d_got, uint64_t n, const uint8_t* d_expected,
                               uint64_t n_expected, const uint32_t* d_expected_idx, uint64_t* d_bad_mask,
                               uint32_t* d_bad_list, uint64_t list_cap, msha_verify_result* d_result, void* stream) {
  static const char* const kEntry = "msha_verify_digests_device";
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (n >= 0xffffffffull) return msha::bad_arg(ctx, kEntry, "n must be below 2^32 - 1");
  if (!d_expected_idx && n != n_expected)
    return msha::bad_arg(ctx, kEntry, "without d_expected_idx slot i expects row i: n (" + std::to_string(n) +
                                          ") must equal n_expected (" + std::to_string(n_expected) + ")");
  if (n == 0) return MSHA_OK;
  if (!d_got || !d_expected || !d_bad_mask || !d_result) return msha::bad_arg(ctx, kEntry, "null pointer argument");
  if (list_cap > 0 && !d_bad_list) return msha::bad_arg(ctx, kEntry, "d_bad_list is null with list_cap > 0");
  if (reinterpret_cast<uintptr_t>(d_got) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_got must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_expected) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_expected must be 16-byte aligned");

  return msha::guard(ctx, [&] {
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, kEntry, stream, &d);

    msha::VerifyArgs a;
    a.got = d_got;
    a.n = n;
    a.expected = d_expected;
    a.n_expected = n_expected;
    a.expected_idx = d_expected_idx;
    a.bad_mask = d_bad_mask;
    a.bad_list = d_bad_list;
    a.list_cap = list_cap;
    a.result = reinterpret_cast<uint64_t*>(d_result);

    // MSHA_VERIFY_ONLY (diagnostic, tools/verify_bench.py), read at each call: 1 runs
    // the compare alone, 2 the scan alone, over whatever d_bad_mask holds, so that each
    // kernel can be timed by itself.
    const int only = msha::env_int("MSHA_VERIFY_ONLY", 0);
    const bool with_compare = only != 2, with_scan = only != 1;

    msha::LaunchTimer timer(st);
    if (with_compare) msha::launch_check(msha::launch_verify_compare(a, st), "k_verify_compare launch");
    if (with_scan) msha::launch_check(msha::launch_verify_scan(a, st), "k_verify_scan launch");
    const float ms = timer.stop();

    msha_verify_stats& s = msha::ctx_verify_stats(ctx);
    s.calls++;
    s.digests += n;
    s.launches += (with_compare ? 1 : 0) + (with_scan ? 1 : 0);
    s.last_kernel_ms = ms;
  });
}

int msha_get_verify_stats(const msha_ctx* ctx, msha_verify_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_verify_stats(const_cast<msha_ctx*>(ctx));
  out->scan_words = msha::verify::kScanWords;  // a constant: valid before any call
  return MSHA_OK;
}

}  // extern "C"
