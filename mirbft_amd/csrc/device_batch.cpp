// The raw-pointer batch entries of libmirsha: msha_digest_batch_device, the planned device
// call with its three streams (msha_digest_batch_device_planned; planner kernels in
// plan.hip), msha_digest_uniform_device and msha_digest_of_digests_device.
#include <mutex>
#include <string>

#include "ctx.hpp"

using namespace msha;

namespace {

// msha_digest_batch_device_planned's knobs, read once per call
// (tests switch them within one process), and the kernel choices they decide.
struct PlanKnobs {
  bool all_coop;    // few messages: one cooperative launch over the planned order
  bool head;        // otherwise: the longest chains (if any outlast the launch) on a head kernel
  bool two_lane;    // the head on k_digest_chain2, not the cooperative kernel
  bool eight_lane;  // the early head on k_digest_chain8
  bool early;       // an early head (FoldArgs::longs)
  bool ws;          // the lane kernel steals work (k_digest_batch_ws)
  uint32_t head_pct, lane_cycles, wave_block_cycles;
  bool poison_table, check_lookback, trace;
};
PlanKnobs read_plan_knobs(const msha_ctx* ctx, const Device& d, uint64_t n, bool fold) {
  PlanKnobs k;
  k.all_coop = msha::uses_coop(n, d.cus, ctx->kernel_policy);
  k.head = !k.all_coop && ctx->kernel_policy != MSHA_KERNEL_LANE && env_u64("MSHA_PLAN_HEAD", 1) != 0;
  // The head's kernel. Folded, a head is the few distinct long payloads: the
  // two-lane chain (k_digest_chain2, 64 messages per CU, ~10 % fewer cycles a
  // block) shortens it. Unfolded, a storm's head can be thousands of chains
  // (19,456 over 8 GPUs): the cooperative kernel holds twice as many per CU,
  // and the two-lane one made that case 3.0 -> 4.2 ms (profiles/r03_chain_dpp/).
  // MSHA_HEAD_CHAIN2: 0 never, 2 always (A/B).
  const uint64_t chain2 = env_u64("MSHA_HEAD_CHAIN2", 1);
  k.two_lane = chain2 == 2 || (chain2 == 1 && fold);
  // The EARLY head runs on the eight-lane kernel (k_digest_chain8: ~9 % fewer
  // cycles a round, 24 messages a CU instead of 64). It exists only when its
  // chain outlasts the lane kernel's share, so its latency is the call's; the
  // late head (after the scan's cut, when the early head stood down: the lane
  // kernel is the long pole) keeps the denser two-lane kernel -- on it the
  // eight-lane one took 5 CUs' worth of the lane kernel's SIMDs for c5's 100
  // payloads, one GPU 2.73 -> 2.84 ms (profiles/r05_chain8/).
  // MSHA_HEAD_CHAIN8=0: the early head on the two-lane kernel too (A/B).
  k.eight_lane = k.two_lane && env_u64("MSHA_HEAD_CHAIN8", 1) != 0;
  // The early head (folded calls with a two-lane head): unless its gate stands it
  // down (the short messages alone outlast the longest chain), the distinct
  // payloads of >= kLongBlocks blocks are listed (k_fold_longs, beside the alias
  // insert) and, when at most an eighth of the CUs' worth, start on a stream of
  // their own right then, while the insert, the scan and the scatter still run --
  // a folded storm's head does not wait for the whole plan. MSHA_EARLY_HEAD=0:
  // the head after the scan's cut (A/B).
  k.early = fold && k.head && k.two_lane && env_u64("MSHA_EARLY_HEAD", 1) != 0;
  // The lane kernel of a folded call steals work (k_digest_batch_ws: folded c5
  // 2.79 -> 2.69 ms, profiles/r06_ws/); an unfolded one keeps the statically
  // mapped kernel, whose oldest-first issue runs a storm's thousands of long
  // chains one after another (work stealing: 13.3 -> 17.6 ms). MSHA_LANE_WS:
  // 0 never, 2 always (A/B).
  const uint64_t lane_ws = env_u64("MSHA_LANE_WS", 1);
  k.ws = !k.all_coop && (lane_ws == 2 || (lane_ws == 1 && fold));
  const msha::FoldArgs dflt{};
  k.head_pct = (uint32_t)env_u64("MSHA_PLAN_HEAD_PCT", dflt.head_pct);
  k.lane_cycles = (uint32_t)env_u64("MSHA_PLAN_LANE_CYCLES", dflt.lane_cycles);  // A/B of the cost model
  k.wave_block_cycles = (uint32_t)env_u64("MSHA_PLAN_WAVE_CYCLES", dflt.wave_block_cycles);
  // MSHA_POISON_FOLD_TABLE=1 (tests): a fresh alias table is filled with words
  // tagged with the coming epoch, as recycled memory may be -- a table that
  // was not cleared then claims garbage indices (tests/test_gpu_planned.py)
  k.poison_table = env_u64("MSHA_POISON_FOLD_TABLE", 0) != 0;
  k.check_lookback = env_u64("MSHA_CHECK_LOOKBACK", 0) != 0;  // tests: no look-back gave up
  k.trace = trace_on() || env_u64("MSHA_TRACE_PLAN", 0) != 0;
  return k;
}

// A planned call's scratch and streams: sized, the zeroed part cleared on st (after
// the previous planned call, whose kernels still read it), and described in the
// FoldArgs its planner kernels take.
msha::FoldArgs prepare_plan(Device& d, const PlanKnobs& k, const uint64_t* d_off, const uint64_t* d_len,
                            uint64_t n, bool fold, hipStream_t st) {
  const uint64_t ptiles = (n + msha::kPlanTile - 1) / msha::kPlanTile;
  uint64_t cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  // one zeroed block: info (32 words, 128 bytes), the bucket counters, FoldArgs::big,
  // the work-stealing lane kernel's tile counters, the grid reductions' words and
  // (folded) the look-back's status words and give-up count -- cleared by ONE
  // memset per call
  constexpr uint64_t zero_fixed = 128 + 4 * msha::kFoldBuckets + 16 * msha::kFoldBigBuckets +
                                  4 * msha::kWsSlots * msha::kWsStride + 4 * 2 * msha::kGridWords;
  static_assert(zero_fixed % 8 == 0, "the look-back's status words follow 8-byte aligned");
  // (a multiple of 64 bytes: an unaligned tail made hipMemsetAsync a second fill kernel)
  const uint64_t zero_bytes = (zero_fixed + (fold ? 8 * (ptiles + 1) : 0) + 63) / 64 * 64;
  d.f_cnt.ensure(zero_bytes);
  d.f_key.ensure(2 * n);
  d.f_tkeys.ensure(8 * n + 4 * ptiles + 8 * msha::kPlanTile);  // per-tile key lists, then their counts
  d.f_order.ensure(4 * n);
  bool clear_table = false;
  if (fold) {
    // epoch-tagged slots (plan.hip fold_claim): cleared only when the table
    // is (re)allocated -- hipMalloc does not zero -- or the epoch wraps. A
    // reallocation is told by the capacity, not the pointer: hipFree then
    // hipMalloc can hand back the same address, and the grown tail would then
    // hold recycled words whose high half may equal the current epoch.
    const uint64_t cap_before = d.f_table.cap;
    d.f_table.ensure(8 * cap);
    const bool grown = d.f_table.cap != cap_before;
    if (grown && k.poison_table)
      HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d.f_table.p, d.f_epoch + 1, d.f_table.cap / 4, st));
    if (grown || d.f_epoch == 0xFFFFFFFFu) {
      clear_table = true;
      d.f_epoch = 0;
    }
    ++d.f_epoch;
    d.f_rep.ensure(8 * n + 4 * ptiles);  // alias pairs, then their count per tile
  }
  // The planner's scratch (table, order, counters) is the context's: a call
  // on another stream must not overwrite it while an earlier call still reads it.
  if (!d.ev_fdone) HIPCHK(hipEventCreateWithFlags(&d.ev_fdone, hipEventDisableTiming));
  if (d.fdone_recorded) HIPCHK(hipStreamWaitEvent(st, d.ev_fdone, 0));
  if (k.head) {
    if (!d.side_stream) HIPCHK(hipStreamCreateWithFlags(&d.side_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&d.ev_fork, &d.ev_fplan, &d.ev_join})
      if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  if (clear_table) HIPCHK(hipMemsetAsync(d.f_table.p, 0, d.f_table.cap, st));
  HIPCHK(hipMemsetAsync(d.f_cnt.p, 0, zero_bytes, st));
  // (the order's positions past the last lane are filled by k_fold_scatter)
  msha::FoldArgs fa;
  fa.off = d_off;
  fa.len = d_len;
  fa.n = n;
  fa.vec = ((reinterpret_cast<uintptr_t>(d_off) | reinterpret_cast<uintptr_t>(d_len)) & 15) == 0;
  fa.tmask = cap - 1;
  fa.epoch = d.f_epoch;
  if (fold) {
    fa.table = d.f_table.as<uint64_t>();
    fa.apairs = d.f_rep.as<uint64_t>();
    fa.acount = reinterpret_cast<uint32_t*>(fa.apairs + n);
    fa.tstat = reinterpret_cast<uint64_t*>(d.f_cnt.as<uint8_t>() + zero_fixed);
  }
  fa.info = d.f_cnt.as<uint32_t>();
  fa.cnt = fa.info + 32;
  fa.key16 = d.f_key.as<uint16_t>();
  fa.tkeys = d.f_tkeys.as<uint64_t>();
  fa.tkcount = reinterpret_cast<uint32_t*>(fa.tkeys + ptiles * msha::kPlanTile);
  fa.big = reinterpret_cast<uint64_t*>(fa.cnt + msha::kFoldBuckets);  // kFoldBuckets is even: 8-byte aligned
  fa.order = d.f_order.as<uint32_t>();
  fa.grid_ws = reinterpret_cast<uint32_t*>(fa.big + 2 * msha::kFoldBigBuckets) + msha::kWsSlots * msha::kWsStride;
  fa.simds = (uint32_t)d.cus * 4;
  fa.head_per_wg = k.two_lane ? msha::kChain2MsgsPerWg : msha::kCoopMsgsPerWg;
  fa.head_cap = k.head ? (uint32_t)std::min<uint64_t>(n, (uint64_t)d.cus * fa.head_per_wg) : 0;
  // cycles a chain block: two-lane head 1,427 blocks in 2.04 ms at ~2.4 GHz (r04);
  // eight-lane (the early head): tools/chain2_anatomy 1427 8, profiles/r05_chain8/
  fa.coop_cycles = k.two_lane ? 3500 : 4200;
  fa.early_cycles = k.eight_lane ? 3250 : 3500;  // eight-lane: 1,427 blocks in 1.93 ms at ~2.4 GHz (r05)
  fa.head_pct = k.head_pct;
  fa.lane_cycles = k.lane_cycles;
  fa.wave_block_cycles = k.wave_block_cycles;
#ifdef MSHA_FOLD_RACE_TEST
  fa.race_test = (uint32_t)env_u64("MSHA_FOLD_LONGS_SKIP_ODD", 0);
#endif
  if (k.early) {
    fa.long_blocks = (uint32_t)kLongBlocks;
    fa.long_cap = (uint32_t)(d.cus * (k.eight_lane ? msha::kChain8MsgsPerWg : msha::kChain2MsgsPerWg) / 8);
    d.f_longs.ensure(4 * (uint64_t)fa.long_cap);
    fa.longs = d.f_longs.as<uint32_t>();
    if (!d.head_stream) HIPCHK(hipStreamCreateWithFlags(&d.head_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&d.ev_longs, &d.ev_join2})
      if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  return fa;
}

}  // namespace

extern "C" {

int msha_digest_batch_device(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                             const uint64_t* d_len, const uint32_t* d_order, uint64_t n,
                             uint8_t* d_out, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (!d_arena || !d_off || !d_len || !d_out) return fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return guarded(ctx, [&] {
    hipStream_t st;
    device_prologue(ctx, stream, &st);
    Device& d = ctx->devs[0];
    msha::SplitPlan sp;
    msha::LaunchKind kind;
    HIPCHK(msha::launch_digest_batch(d_arena, d_off, d_len, d_order, nullptr, n, d_out,
                                     d.err.as<uint32_t>(), d.cus, ctx->kernel_policy, st,
                                     split_for(d, n, ctx->kernel_policy, sp), &kind));
    count_launch(ctx, nullptr, kind);
  });
}

int msha_digest_batch_device_planned(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                                     const uint64_t* d_len, uint64_t n, uint32_t flags, uint8_t* d_out,
                                     void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (!d_arena || !d_off || !d_len || !d_out) return fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (flags & ~(uint32_t)MSHA_PLAN_FOLD_ALIASES) return fail(ctx, MSHA_ERR_INVALID_ARG, "unknown plan flags");
  if (n >= (1ull << 31)) return fail(ctx, MSHA_ERR_INVALID_ARG, "planned device batches hold < 2^31 messages");
  return guarded(ctx, [&] {
    hipStream_t st;
    device_prologue(ctx, stream, &st);
    Device& d = ctx->devs[0];
    // Not capturable into a HIP graph (mirsha.h): the call waits on the previous
    // planned call's event, recorded outside any capture, and forks to and joins
    // from a library-owned side stream. Say so instead of failing inside HIP.
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(st, &cap_status));
    if (cap_status != hipStreamCaptureStatusNone)
      throw MshaError(MSHA_ERR_INVALID_ARG,
                     "msha_digest_batch_device_planned cannot be captured into a HIP graph; "
                     "use msha_digest_batch_device there");
    const bool fold = flags & MSHA_PLAN_FOLD_ALIASES;
    const PlanKnobs k = read_plan_knobs(ctx, d, n, fold);
    // Three streams. The memsets, the insert (or the counts), the scan, the lane
    // kernel and the fill run on the caller's stream, so a step starts without a
    // cross-queue hand-off (~20 us of a folded c5 step's timeline, profiles/r06_plan7/).
    // The early head's gate, list and chain run on head_stream, forked right after
    // the memsets (DESIGN.md §(d) "Head before the tile prefix"). The scatter and
    // the late head run on side_stream, forked after the scan: the head's packet
    // follows the scatter in its own queue while the lane kernel's needs a
    // cross-queue signal, so the head's workgroups are resident before the lane
    // kernel fills every SIMD (queued the other way round, the head could not get
    // a CU's registers until the lane kernel drained: c5 folded 6.2 ms, its
    // 1,427-block chain starting at the end). The variants that moved the list into
    // the insert or dropped the late head lost: DESIGN.md §(d) "The folded planner".
    // 1. the memsets
    d.f_last.n = 0;  // (msha_planned_read_plan: the scratch may be regrown from here on)
    const msha::FoldArgs fa = prepare_plan(d, k, d_off, d_len, n, fold, st);
    d.f_last.n = n;  // and now describes this call
    d.f_last.fold = fold;
    d.f_last.early = k.early;
    d.f_last.long_cap = fa.long_cap;
    d.f_last.head_cap = fa.head_cap;
    d.f_last.head_per_wg = fa.head_per_wg;
    d.f_last.gave_up_at =
        fold ? (uint64_t)(reinterpret_cast<const uint8_t*>(fa.tstat + (n + msha::kPlanTile - 1) / msha::kPlanTile) -
                          d.f_cnt.as<uint8_t>())
             : 0;
    if (k.early) {
      // 2. the head stream's fork
      HIPCHK(hipEventRecord(d.ev_longs, st));
      HIPCHK(hipStreamWaitEvent(d.head_stream, d.ev_longs, 0));
      // 3. the gate and the list, beside the alias insert
      HIPCHK(msha::launch_fold_longs(fa, d.cus, d.head_stream));
      HIPCHK(hipEventRecord(d.ev_longs, d.head_stream));
      // 4. the early head: the listed payloads (info[4] of them; 0: it stood down)
      msha::LaneGate eg;
      eg.head = fa.info + 4;
      eg.head_part = true;
      eg.two_lane = true;
      eg.eight_lane = k.eight_lane;
      msha::LaunchKind ek;
      HIPCHK(msha::launch_digest_batch(d_arena, d_off, d_len, fa.longs, nullptr, fa.long_cap, d_out,
                                       d.err.as<uint32_t>(), d.cus, MSHA_KERNEL_COOP, d.head_stream, nullptr,
                                       &ek, &eg));
      count_launch(ctx, nullptr, ek);
      HIPCHK(hipEventRecord(d.ev_join2, d.head_stream));
    }
    // 5. the insert and the scan, then the scatter (with a head on the side stream,
    // and after the list, against which it resolves the heads)
    HIPCHK(msha::launch_fold_plan(fa, st, k.head ? d.side_stream : st, d.ev_fork, k.early ? d.ev_longs : nullptr));
    msha::LaunchKind kind;
    if (k.all_coop) {
      HIPCHK(msha::launch_digest_batch(d_arena, d_off, d_len, fa.order, nullptr, n, d_out, d.err.as<uint32_t>(),
                                       d.cus, MSHA_KERNEL_COOP, st, nullptr, &kind));
      count_launch(ctx, nullptr, kind);
    } else {
      if (k.head) {
        // 6. the late head: the scan's cut (info[5]; 0 when the early head has the long lanes)
        HIPCHK(hipEventRecord(d.ev_fplan, d.side_stream));
        msha::LaneGate hg;
        hg.head = fa.info + 5;
        hg.head_part = true;
        hg.two_lane = k.two_lane;
        HIPCHK(msha::launch_digest_batch(d_arena, d_off, d_len, fa.order, nullptr, fa.head_cap, d_out,
                                         d.err.as<uint32_t>(), d.cus, MSHA_KERNEL_COOP, d.side_stream, nullptr,
                                         &kind, &hg));
        count_launch(ctx, nullptr, kind);
        HIPCHK(hipEventRecord(d.ev_join, d.side_stream));
        HIPCHK(hipStreamWaitEvent(st, d.ev_fplan, 0));
      }
      // 7. the lane kernel, over every lane the heads leave (info[1] skipped); the
      // work-stealing one visits the planned lanes only (info[0])
      msha::LaneGate body;
      body.head = fa.info + 1;
      if (k.ws) {
        body.ws_ctr = reinterpret_cast<uint32_t*>(fa.big + 2 * msha::kFoldBigBuckets);
        body.lanes = fa.info;
      }
      HIPCHK(msha::launch_digest_batch(d_arena, d_off, d_len, fa.order, nullptr, n, d_out, d.err.as<uint32_t>(),
                                       d.cus, ctx->kernel_policy, st, nullptr, &kind, &body));
      count_launch(ctx, nullptr, kind);
      // 8. the joins
      if (k.head) HIPCHK(hipStreamWaitEvent(st, d.ev_join, 0));
      if (k.early) HIPCHK(hipStreamWaitEvent(st, d.ev_join2, 0));
    }
    // 9. the fill: every folded message copies its representative's digest
    if (fold) HIPCHK(msha::launch_fold_fill(fa, d_out, st));
    if (fold && k.check_lookback) {  // (waits for the call)
      uint64_t gave_up = 0;
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(&gave_up, fa.tstat + (n + msha::kPlanTile - 1) / msha::kPlanTile, sizeof gave_up,
                       hipMemcpyDeviceToHost));
      if (gave_up)
        throw MshaError(MSHA_ERR_HIP, "planner tile look-back gave up waiting " + std::to_string(gave_up) +
                                          " time(s) (digests exact, folding reduced)");
    }
    HIPCHK(hipEventRecord(d.ev_fdone, st));
    d.fdone_recorded = true;
    ctx->stats.planned_device_calls++;
    if (k.trace) {  // MSHA_TRACE / MSHA_TRACE_PLAN: the GPU's plan (waits for the call)
      uint32_t info[2] = {0, 0};
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(info, fa.info, sizeof info, hipMemcpyDeviceToHost));
      fprintf(stderr, "[msha] planned device call: %llu messages, %u lanes, head %u\n", (unsigned long long)n,
              info[0], info[1]);
    }
  });
}

int msha_planned_read_plan(msha_ctx* ctx, msha_planned_plan* out, uint32_t* order, uint64_t order_cap,
                           uint32_t* longs, uint64_t longs_cap) {
  if (!ctx || !out || (order_cap && !order) || (longs_cap && !longs)) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);
  *out = msha_planned_plan{};
  if (ctx->devs.empty() || ctx->devs[0].f_last.n == 0) return MSHA_OK;
  return guarded(ctx, [&] {
    Device& d = ctx->devs[0];
    const Device::LastPlanned& lp = d.f_last;
    HIPCHK(hipSetDevice(d.id));
    HIPCHK(hipDeviceSynchronize());
    uint32_t info[32];
    HIPCHK(hipMemcpy(info, d.f_cnt.p, sizeof info, hipMemcpyDeviceToHost));
    out->n = lp.n;
    out->folded = lp.fold;
    out->lanes = info[0];
    out->head = info[1];
    out->early = info[4];
    out->late = info[5];
    out->long_lanes = info[16];
    out->long_listed = info[2];
    out->gate = info[6];
    out->long_cap = lp.long_cap;
    out->head_cap = lp.head_cap;
    out->head_per_wg = lp.head_per_wg;
    if (lp.fold)
      HIPCHK(hipMemcpy(&out->gave_up, d.f_cnt.as<uint8_t>() + lp.gave_up_at, 8, hipMemcpyDeviceToHost));
    const uint64_t k = std::min(lp.n, order_cap);
    if (k) HIPCHK(hipMemcpy(order, d.f_order.p, 4 * k, hipMemcpyDeviceToHost));
    // (f_longs exists only for calls with an early head to try: long_cap 0 otherwise)
    const uint64_t kl = lp.early ? std::min<uint64_t>(std::min(info[2], lp.long_cap), longs_cap) : 0;
    if (kl) HIPCHK(hipMemcpy(longs, d.f_longs.p, 4 * kl, hipMemcpyDeviceToHost));
  });
}

int msha_digest_uniform_device(msha_ctx* ctx, const uint8_t* d_arena, uint64_t stride,
                               uint64_t msg_len, uint64_t n, uint8_t* d_out, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (!d_arena || !d_out) return fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (stride % MSHA_DEVICE_ALIGN) return fail(ctx, MSHA_ERR_ALIGNMENT, "stride must be a multiple of 16");
  return guarded(ctx, [&] {
    hipStream_t st;
    device_prologue(ctx, stream, &st);
    Device& d = ctx->devs[0];
    msha::LaunchKind kind;
    HIPCHK(msha::launch_digest_uniform(d_arena, stride, msg_len, n, d_out, d.err.as<uint32_t>(), d.cus, st,
                                       &kind));
    count_launch(ctx, nullptr, kind);
  });
}

int msha_digest_of_digests_device(msha_ctx* ctx, const uint8_t* d_table, const uint32_t* d_idx,
                                  const uint64_t* d_begin, uint64_t n, uint8_t* d_out, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (!d_table || !d_idx || !d_begin || !d_out) return fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return guarded(ctx, [&] {
    hipStream_t st;
    device_prologue(ctx, stream, &st);
    Device& d = ctx->devs[0];
    msha::SplitPlan sp;
    msha::LaunchKind kind;
    HIPCHK(msha::launch_digest_of_digests(d_table, d_idx, d_begin, n, d_out, d.err.as<uint32_t>(), st,
                                          split_for(d, n, ctx->kernel_policy, sp, msha::kMaxSegmentsDod),
                                          &kind));
    count_launch(ctx, nullptr, kind);
  });
}

}  // extern "C"
