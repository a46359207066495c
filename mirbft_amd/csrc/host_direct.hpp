// The direct path of msha_digest_batch (host_direct.cpp): a dense arena uploaded as it is
// (pinned) or through staging slots (pageable), its lanes planned on the GPU (plan.hip).
#pragma once
#include "ctx.hpp"

namespace msha {

// Pinned off/len of a one-shard call: uploaded to the shard's p_meta as the
// call starts, before validation, which the link would otherwise sit idle for
// (c5 on one GPU: 1.3 ms of a 72 ms call). Only the direct path consumes the
// upload; on any other path (or an error) the destructor drains it, so off/len
// are no longer read once the call returns.
struct EarlyMeta {
  Device* d = nullptr;
  bool used = false;
  EarlyMeta(msha_ctx* ctx, const uint64_t* off, const uint64_t* len, uint64_t n) {
    if (ctx->devs.size() != 1 || n <= small_msgs()) return;
    if (!(is_pinned_host(off) && is_pinned_host(off + n - 1) && is_pinned_host(len) && is_pinned_host(len + n - 1)))
      return;
    Device& dv = ctx->devs[0];
    HIPCHK(hipSetDevice(dv.id));
    dv.p_meta.ensure(16 * n);
    HIPCHK(hipEventRecord(dv.ev_up0, dv.copy_stream));
    HIPCHK(hipMemcpyAsync(dv.p_meta.p, off, 8 * n, hipMemcpyHostToDevice, dv.copy_stream));
    HIPCHK(hipMemcpyAsync(dv.p_meta.as<uint64_t>() + n, len, 8 * n, hipMemcpyHostToDevice, dv.copy_stream));
    d = &dv;
  }
  bool queued() const { return d != nullptr; }
  ~EarlyMeta() {
    if (d && !used) (void)hipStreamSynchronize(d->copy_stream);
  }
};

// (host_direct.cpp)
void run_direct(msha_ctx* ctx, double t0, uint64_t n, const uint64_t* off, const uint64_t* len,
                const uint8_t* arena, uint8_t* out, const BatchScan& sc, EarlyMeta* early, bool staged);

}  // namespace msha
