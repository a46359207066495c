// The latency path's non-template part (host_small.hpp).
#include "host_small.hpp"

namespace msha {

// Stats of a latency-path call (run_small, run_small_zc).
void small_stats(msha_ctx* ctx, Device& d, double t0, double t_pack, double t_dev, uint64_t m, uint64_t pay,
                 uint64_t h2d, uint64_t d2h, bool packed, msha::LaunchKind kind) {
  for (Device& o : ctx->devs) {
    o.st = msha_shard_stats{};
    o.st.device = o.id;
  }
  d.st.messages = d.st.lanes = m;
  d.st.h2d_payload_bytes = pay;
  d.st.h2d_bytes = h2d;
  d.st.d2h_bytes = d2h;
  d.st.device_ms = t_dev - t_pack;
  count_launch(ctx, &d, kind);
  ctx->stats.calls++;
  ctx->stats.small_calls++;
  ctx->stats.plan_ms = t_pack - t0;
  ctx->stats.pack_ms = packed ? t_pack - t0 : 0;
  ctx->stats.device_ms = t_dev - t_pack;
  ctx->stats.h2d_bytes = h2d;
  ctx->stats.d2h_bytes = d2h;
  ctx->stats.total_ms = now_ms() - t0;
  trace("done", t0);
}

}  // namespace msha
