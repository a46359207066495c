// The host scaffold of an entry point: how a failed HIP call becomes a return code and
// the context's error text, how a raw-pointer device entry starts, and how a launch is
// timed under MSHA_PARTS_TIMING=1. Host-only, no kernel; every translation unit beside
// the kernels includes it.
//
// An entry checks its arguments (bad_arg), then runs the rest inside guard(): there a
// HIP call goes through HIPCHK, a launcher's result through launch_check, and
// device_entry() gives the device and the stream. What is thrown becomes the return code.
#pragma once
#include <hip/hip_runtime.h>

#include <exception>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/mirsha.h"
#include "ctx_access.hpp"
#include "kernels.hpp"
#include "msha_error.hpp"

namespace msha {

// The error of a failed HIP call: what names the call (or the kernel launched).
inline MshaError hip_fail(const char* what, hipError_t e) {
  return MshaError(e == hipErrorOutOfMemory ? MSHA_ERR_OUT_OF_MEMORY : MSHA_ERR_HIP,
                   std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(expr)                                         \
  do {                                                       \
    hipError_t e_ = (expr);                                  \
    if (e_ != hipSuccess) throw ::msha::hip_fail(#expr, e_); \
  } while (0)

// For a launcher that returns hipError_t: what names its kernel ("k_digest_parts launch").
inline void launch_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw hip_fail(what, e);
}

// Runs f and maps what it throws to the return code and the context's error text;
// success clears the text. ctx may be null (the code is returned all the same).
template <class F>
int guard(msha_ctx* ctx, F&& f) {
  try {
    f();
    return ctx_fail(ctx, MSHA_OK, nullptr);
  } catch (const MshaError& e) {
    return ctx_fail(ctx, e.code, e.what());
  } catch (const std::bad_alloc&) {
    return ctx_fail(ctx, MSHA_ERR_OUT_OF_MEMORY, "host allocation failed");
  } catch (const std::exception& e) {
    return ctx_fail(ctx, MSHA_ERR_HIP, e.what());
  } catch (...) {
    return ctx_fail(ctx, MSHA_ERR_HIP, "unknown error");
  }
}

inline int bad_arg(msha_ctx* ctx, const char* entry, const std::string& what) {
  return ctx_fail(ctx, MSHA_ERR_INVALID_ARG, (std::string(entry) + ": " + what).c_str());
}

inline bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIPCHK(hipStreamIsCapturing(st, &cap));
  return cap != hipStreamCaptureStatusNone;
}

// The start of a raw-pointer device entry, inside guard() with the lock held: the
// context's first device made current, and the caller's stream or the context's own.
// The first device call of a context allocates its error word, which a capturing stream
// does not allow: such a call is refused before anything is touched. The capture status
// is asked for only then; an entry that knows it already passes it in.
inline hipStream_t device_entry(msha_ctx* ctx, const char* entry, void* stream, bool capturing, CtxDevice* d) {
  if (capturing && !ctx_first_device_ready(ctx))
    throw MshaError(MSHA_ERR_INVALID_ARG,
                    std::string(entry) + ": the context's error word cannot be allocated while the stream is "
                                         "being captured: make one call of this size outside the capture first");
  *d = ctx_first_device(ctx);
  return stream ? static_cast<hipStream_t>(stream) : d->stream;
}
inline hipStream_t device_entry(msha_ctx* ctx, const char* entry, void* stream, CtxDevice* d) {
  const bool capturing = stream && !ctx_first_device_ready(ctx) && stream_capturing(static_cast<hipStream_t>(stream));
  return device_entry(ctx, entry, stream, capturing, d);
}

// MSHA_PARTS_TIMING=1 (diagnostic, read at each call): the launches between the
// construction and stop() are timed with HIP events, which makes the call wait for
// them; never on a capturing stream. Otherwise no HIP call is made and stop() gives 0.
class LaunchTimer {
 public:
  static bool wanted() { return env_int("MSHA_PARTS_TIMING", 0) == 1; }
  explicit LaunchTimer(hipStream_t st) : LaunchTimer(st, wanted() && !stream_capturing(st)) {}
  // enabled: wanted() and the stream known not to be capturing
  LaunchTimer(hipStream_t st, bool enabled) : st_(st), on_(enabled) {
    if (!on_) return;
    try {
      HIPCHK(hipEventCreate(&a_));
      HIPCHK(hipEventCreate(&b_));
      HIPCHK(hipEventRecord(a_, st_));
    } catch (...) {
      destroy();
      throw;
    }
  }
  LaunchTimer(const LaunchTimer&) = delete;
  LaunchTimer& operator=(const LaunchTimer&) = delete;
  ~LaunchTimer() { destroy(); }
  bool enabled() const { return on_; }
  // milliseconds from the construction to here, once the stream has got here
  float stop() {
    float ms = 0;
    if (!on_) return ms;
    HIPCHK(hipEventRecord(b_, st_));
    HIPCHK(hipEventSynchronize(b_));
    HIPCHK(hipEventElapsedTime(&ms, a_, b_));
    return ms;
  }

 private:
  void destroy() {
    if (a_) (void)hipEventDestroy(a_);
    if (b_) (void)hipEventDestroy(b_);
    a_ = b_ = nullptr;
  }
  hipStream_t st_;
  bool on_;
  hipEvent_t a_ = nullptr, b_ = nullptr;
};

}  // namespace msha
