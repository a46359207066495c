// msha_hash_actions_device_routed: msha_hash_actions_device_planned with its long lists
// routed to the eight-lane chain (include/mirsha.h "Part lists with their long lists
// routed to the chains"). The decision is k_route_measure's (parts_plan.hip,
// parts_route.hpp); this file lays out the workspace and enqueues, all on the caller's
// stream:
//   init, mark, route measure, scan, scatter   launch_parts_route_plan
//   k_concat_copy over the max_long slots      (unfilled slots: msg_len 0, skipped)
//   the chain over the flatten buffer          launch_digest_batch, n = max_long, AUTO:
//                                              max_long <= 16 x CUs makes it
//                                              k_digest_chain8; digests land in the
//                                              lists' own rows (out_idx)
//   k_digest_parts_planned, k_parts_fill       the lanes that remain
// The lengths come out of the measure, so k_concat_measure and k_concat_scan do not run:
// a list's parts are summed once a call. The workspace is this entry's own
// (call_workspace.hpp PartsRouteState, laid out by parts_route.hpp Layout) and follows
// the workspace rule stated there.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/mirsha.h"
#include "call_workspace.hpp"
#include "parts_route.hpp"

namespace {

const char* const kEntry = "msha_hash_actions_device_routed";

}  // namespace

extern "C" {

int msha_hash_actions_device_routed(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_part_off,
                                    const uint64_t* d_part_len, const uint64_t* d_list_part_begin,
                                    uint64_t n_lists, const uint32_t* d_action_list, uint64_t n_actions,
                                    const msha_route_opts* opts, uint8_t* d_out, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (n_lists >= 0xffffffffull || n_actions >= 0xffffffffull)
    return msha::bad_arg(ctx, kEntry, "n_lists and n_actions must be below 2^32 - 1");
  if (!d_action_list && n_actions != n_lists)
    return msha::bad_arg(ctx, kEntry, "without d_action_list action i is list i: n_actions (" +
                                          std::to_string(n_actions) + ") must equal n_lists (" +
                                          std::to_string(n_lists) + ")");
  if (n_actions == 0) return MSHA_OK;  // before opts, whose max_long bound needs the device
  // opts: the long_bytes bounds here, the max_long bound once the device is known
  const int rc = msha::guard(ctx, [&] { (void)msha::route_opts(kEntry, "list", opts, 0, MSHA_ROUTE_LONG_BLOCKS_DEFAULT); });
  if (rc != MSHA_OK) return rc;
  if (!d_arena || !d_part_off || !d_part_len || !d_list_part_begin || !d_out)
    return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(ctx, kEntry, "d_arena must be 16-byte aligned");

  return msha::guard(ctx, [&] {
    // a capturing stream allows no allocation: know that before the context's first
    // device call would make one (the error word) or the workspace would grow
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    msha::PartsRouteState& rs = msha::ctx_parts_route(ctx);
    if (capturing && !msha::ctx_first_device_ready(ctx)) msha::CallWorkspace::refuse(kEntry);
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, kEntry, stream, capturing, &d);

    const msha_route_opts o = msha::route_opts(kEntry, "list", opts, d.cus, MSHA_ROUTE_LONG_BLOCKS_DEFAULT);
    msha::RouteArgs r;
    r.long_blocks = o.long_blocks;
    r.max_long = o.max_long;
    r.long_bytes = o.long_bytes;

    const msha::parts_route::Layout lay(n_lists, r.max_long, r.long_bytes, d_action_list != nullptr);
    // the arrays grow with a quarter to spare, the flatten buffer is what was asked for
    uint8_t* ws = rs.ws.acquire(kEntry, lay.bytes, lay.flat / 4, capturing, st);
    const msha::PartsPlanArgs a = msha::plan_args(d_arena, d_part_off, d_part_len, d_list_part_begin, n_lists,
                                                  d_action_list, n_actions, d_out, d.err, ws, lay.plan);
    r.claim = reinterpret_cast<unsigned long long*>(ws + lay.claim);
    r.msg_off = reinterpret_cast<uint64_t*>(ws + lay.msg_off);
    r.msg_len = reinterpret_cast<uint64_t*>(ws + lay.msg_len);
    r.sel = reinterpret_cast<uint32_t*>(ws + lay.sel);
    r.chain_order = reinterpret_cast<uint32_t*>(ws + lay.chain);
    r.out_idx = reinterpret_cast<uint32_t*>(ws + lay.out_idx);
    uint8_t* const flat = ws + lay.flat;

    // the copy reads the route's slots as the messages of a concat call whose scan has run
    msha::ConcatArgs c;
    c.arena = d_arena;
    c.part_off = d_part_off;
    c.part_len = d_part_len;
    c.begin = d_list_part_begin;
    c.n_lists = n_lists;
    c.select = r.sel;
    c.n_select = r.max_long;
    c.dst = flat;
    c.dst_bytes = r.long_bytes;
    c.msg_off = r.msg_off;
    c.msg_len = r.msg_len;
    c.err = d.err;
    c.wave_sum_parts = a.wave_sum_parts;

    // under MSHA_PARTS_TIMING=1 the counts are read back too, which makes the call wait
    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    uint32_t plan_launches = 0;
    msha::launch_check(msha::launch_parts_route_plan(a, r, st, &plan_launches), "parts route plan launch");
    msha::launch_check(msha::launch_concat_copy(c, st), "k_concat_copy launch");
    msha::LaunchKind kind = msha::kLaunchNone;
    msha::launch_check(msha::launch_digest_batch(flat, r.msg_off, r.msg_len, r.chain_order, r.out_idx, r.max_long,
                                                 d_action_list ? a.table : d_out, d.err, d.cus,
                                                 MSHA_KERNEL_AUTO, st, nullptr, &kind),
                       "routed chain launch");
    msha::ctx_count_launch(ctx, kind);
    msha::launch_check(msha::launch_digest_parts_planned(a, st), "k_digest_parts_planned launch");
    if (d_action_list) msha::launch_check(msha::launch_parts_fill(a, st), "k_parts_fill launch");
    rs.last_lists = n_lists;
    rs.last_slots = r.max_long;
    rs.at_order = lay.plan.order;
    rs.at_chain = lay.chain;
    rs.at_out_idx = lay.out_idx;
    rs.at_claim = lay.claim;
    rs.ws.commit(st, capturing);

    const float ms = timer.stop();
    uint32_t info[4] = {0, 0, 0, 0};
    unsigned long long claim[msha::parts_route::kClaimWords] = {};
    if (timer.enabled()) {
      HIPCHK(hipMemcpy(info, a.info, sizeof info, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(claim, r.claim, sizeof claim, hipMemcpyDeviceToHost));
    }
    msha_parts_route_stats& s = rs.stats;
    s.calls++;
    s.actions += n_actions;
    s.lists += n_lists;
    s.launches_plan += plan_launches;
    s.launches_copy++;
    s.launches_chain++;
    s.launches_hash++;
    if (d_action_list) s.launches_fill++;
    s.last_lanes = info[0];
    s.last_blocks = (uint64_t)info[3] << 32 | info[2];
    s.last_routed = claim[msha::parts_route::kClaimRouted];
    s.last_routed_bytes = claim[msha::parts_route::kClaimBytes];
    s.last_kernel_ms = ms;
  });
}

int msha_get_parts_route_stats(const msha_ctx* ctx, msha_parts_route_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  *out = msha::ctx_parts_route(const_cast<msha_ctx*>(ctx)).stats;
  return MSHA_OK;
}

int msha_parts_route_read(msha_ctx* ctx, uint32_t* lists, uint64_t cap, uint64_t* n_routed,
                          uint64_t* routed_bytes) {
  if (!ctx || !n_routed || !routed_bytes || (cap && !lists)) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  msha::PartsRouteState& rs = msha::ctx_parts_route(ctx);
  *n_routed = 0;
  *routed_bytes = 0;
  if (!rs.ws.ran()) return MSHA_OK;
  return msha::guard(ctx, [&] {
    (void)msha::ctx_first_device(ctx);
    HIPCHK(hipDeviceSynchronize());
    const uint8_t* ws = rs.ws.data();
    const uint64_t m = rs.last_slots;
    std::vector<uint32_t> chain(m), idx(m);
    unsigned long long claim[msha::parts_route::kClaimWords] = {};
    HIPCHK(hipMemcpy(chain.data(), ws + rs.at_chain, 4 * m, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(idx.data(), ws + rs.at_out_idx, 4 * m, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(claim, ws + rs.at_claim, sizeof claim, hipMemcpyDeviceToHost));
    uint64_t k = 0;
    for (uint64_t s = 0; s < m; ++s) {
      if (chain[s] == msha::parts_route::kUnfilledOrder) continue;  // a slot nobody filled
      if (k < cap) lists[k] = idx[s];
      ++k;
    }
    *n_routed = k;
    *routed_bytes = claim[msha::parts_route::kClaimBytes];
  });
}

int msha_parts_route_read_order(msha_ctx* ctx, uint32_t* order, uint64_t cap, uint64_t* lanes) {
  if (!ctx || !lanes || (cap && !order)) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  msha::PartsRouteState& rs = msha::ctx_parts_route(ctx);
  return msha::read_plan_order(ctx, rs.ws, rs.last_lists, rs.at_order, order, cap, lanes);
}

}  // extern "C"
