// The direct path of msha_digest_batch: run_direct. Its host planning (granule marking,
// granule map, upload enumeration) is in host_plan.hpp; the shard steps it shares with
// the gather pipeline are in host_pipeline.cpp.
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "host_direct.hpp"
#include "host_pipeline.hpp"

namespace msha {

static_assert(kDirectChunk == 1ull << msha::kDirectChunkShift, "host_plan.hpp states kernels.hpp's upload piece");

namespace {

// Direct (pinned-arena) host call, planned on the GPU. Each shard, on a host
// thread of its own (for_each_shard), and with no whole-batch phase after the
// scan:
//   1. one threaded pass over its messages stages their raw (off, len) in
//      pinned memory and marks the granules (>= 64 KiB) of the arena they touch;
//   2. the copy stream uploads the metadata and granule map, then the marked
//      byte ranges (runs of granules, compacted) in 64 MiB device pieces with
//      one event each -- no gather copy;
//   3. the planner kernels (plan.hip) fold aliases, order the lanes by (piece
//      completing the payload, descending block count) and write lane-indexed
//      off/len/slot; the host reads back the group cuts and per-group minima;
//   4. each lane group is launched behind its piece's event, and the digest
//      slots that are final stream back after each launch.
// The host's share of the call is the scan and pass 1, ~2 passes over 16 bytes
// per message; everything per-lane runs on the GPU.
// A one-use barrier for the shard threads of one call. A thread that leaves
// early (an empty shard, an exception) still counts itself in (Arrival's
// destructor) so the others never wait forever.
struct CallBarrier {
  std::mutex mu;
  std::condition_variable cv;
  uint32_t left;
  explicit CallBarrier(uint32_t n) : left(n) {}
  void arrive(bool wait) {
    std::unique_lock<std::mutex> g(mu);
    if (--left == 0) cv.notify_all();
    else if (wait) cv.wait(g, [&] { return left == 0; });
  }
};
struct Arrival {
  CallBarrier* b;
  bool done = false;
  void wait() {
    if (b && !done) b->arrive(true);
    done = true;
  }
  ~Arrival() {
    if (b && !done) b->arrive(false);
  }
};

// Has event e completed? (A not-ready query leaves no error behind for a later
// hipGetLastError to pick up.)
bool event_done(hipEvent_t e) {
  const hipError_t r = hipEventQuery(e);
  if (r == hipSuccess) return true;
  (void)hipGetLastError();
  if (r != hipErrorNotReady) HIPCHK(r);
  return false;
}

}  // namespace

void run_direct(msha_ctx* ctx, double t0, uint64_t n, const uint64_t* off, const uint64_t* len,
                const uint8_t* arena, uint8_t* out, const BatchScan& sc, EarlyMeta* early, bool staged) {
  const uint32_t k = (uint32_t)ctx->devs.size();
  const bool out_pinned = is_pinned_host(out) && is_pinned_host(out + 32 * n - 1);
  // Interleaving knobs (tests, read per call): upload pieces of 2^MSHA_DIRECT_PIECE_SHIFT
  // device bytes (16..26; 26 = 64 MiB, the default) and, on the staged path,
  // staging slots of MSHA_STAGED_SLOT_BYTES (64 KiB .. 32 MiB, the default) with
  // a pause of MSHA_STAGED_DELAY_US before each refill. Small pieces and slots
  // and a pause make the plan arrive, and heads and lane groups launch, between
  // slot refills while later pieces still upload (tests/test_gpu_parity.py
  // test_staged_direct_interleaved).
  const unsigned piece_shift =
      (unsigned)std::min<uint64_t>(msha::kDirectChunkShift, std::max<uint64_t>(16, env_u64("MSHA_DIRECT_PIECE_SHIFT", msha::kDirectChunkShift)));
  const uint64_t piece_bytes = 1ull << piece_shift;
  const uint64_t slot_bytes =
      std::min<uint64_t>(kChunkBytes, std::max<uint64_t>(64 << 10, env_u64("MSHA_STAGED_SLOT_BYTES", kChunkBytes))) & ~uint64_t(63);
  const uint64_t slot_delay_us = std::min<uint64_t>(env_u64("MSHA_STAGED_DELAY_US", 0), 100000);
  // off/len in pinned memory (msha_pinned_alloc, as the Go adapter packs them):
  // uploaded as they are, no staging copy (one shard: already on the way, EarlyMeta)
  const bool meta_early = early && early->queued();
  if (meta_early) early->used = true;
  const bool meta_pinned = meta_early || (is_pinned_host(off) && is_pinned_host(off + n - 1) &&
                                          is_pinned_host(len) && is_pinned_host(len + n - 1));
  std::vector<uint64_t> bounds(k + 1);
  if (k == 1) {
    bounds[0] = 0;
    bounds[1] = n;
  } else {
    partition_pieces(len, n, k, sc.csum, bounds.data());
  }
  // One granule grid over the batch's span: at most 2^20 granules of >= 64 KiB.
  unsigned gs = 16;
  while (((sc.hi - (sc.lo & ~((1ull << gs) - 1))) >> gs) >= (1ull << 20)) ++gs;
  const uint64_t G = 1ull << gs;
  const uint64_t glo = sc.lo & ~(G - 1);
  const uint64_t nG = ((sc.hi - glo) >> gs) + 1;
  // Shards sharing one GPU (MSHA_VIRTUAL_SHARDS) share its PCIe link and DMA
  // engines: every shard's metadata goes up before any shard's payload, or a
  // shard's planner waits behind the other shards' payload (up to the whole
  // batch). Separate GPUs have links of their own and never wait on each other.
  bool shared_gpu = false;
  for (uint32_t s = 1; s < k; ++s) shared_gpu |= ctx->devs[s].id == ctx->devs[0].id;
  CallBarrier meta_up(k), plan_up(k);
  std::vector<uint8_t> meta_queued(k, 0);
  std::vector<Plan>& plans = ctx->plans;
  plans.resize(k);
  for (uint32_t s = 0; s < k; ++s) {
    Plan& P = plans[s];
    P = Plan{};
    P.ordered = true;
    Device& d = ctx->devs[s];
    d.lo = bounds[s];
    d.hi = bounds[s + 1];
    d.st = msha_shard_stats{};
    d.st.device = d.id;
  }
  for_each_shard(ctx, [&](uint32_t s) {
    Device& d = ctx->devs[s];
    Plan& P = plans[s];
    Arrival arrival{shared_gpu ? &meta_up : nullptr}, arrival2{shared_gpu ? &plan_up : nullptr};
    const uint64_t m = d.hi - d.lo;
    P.m = m;
    d.st.messages = m;
    if (m == 0) return;
    const uint64_t* O = off + d.lo;
    const uint64_t* L = len + d.lo;
    HIPCHK(hipSetDevice(d.id));
    // 1. stage (off, len) (unless the caller's arrays are pinned), mark granules, the shard's span.
    // Pinned off/len go up right away, under the marking pass (c5 on one GPU:
    // 134 MB, ~2.5 ms of PCIe that no longer waits for the host).
    d.p_meta.ensure(16 * m);
    if (meta_pinned && !meta_early) {
      HIPCHK(hipEventRecord(d.ev_up0, d.copy_stream));
      HIPCHK(hipMemcpyAsync(d.p_meta.p, O, 8 * m, hipMemcpyHostToDevice, d.copy_stream));
      HIPCHK(hipMemcpyAsync(d.p_meta.as<uint64_t>() + m, L, 8 * m, hipMemcpyHostToDevice, d.copy_stream));
    }
    if (!meta_pinned) d.h_meta.ensure(16 * m);
    uint64_t* h_off = meta_pinned ? nullptr : d.h_meta.as<uint64_t>();
    uint64_t* h_len = meta_pinned ? nullptr : h_off + m;
    std::vector<uint8_t>& mark = d.direct_mark;
    mark.assign(nG, 0);
    // Long chains (>= kLongBlocks blocks) get their payloads uploaded first and,
    // when few enough, a head launch of their own (below).
    const uint64_t long_blocks = long_chain_blocks(sc.bmax, ctx->kernel_policy);
    const ShardSpan sh = stage_and_mark(O, L, m, glo, gs, h_off, h_len, mark, long_blocks);
    const bool any = sh.any();                       // some payload byte at all
    const uint64_t gbase = any ? sh.g0 : 0, ng = any ? sh.g1 - sh.g0 + 1 : 1;
    d.h_gmap.ensure(8 * ng);
    uint64_t* gmap = d.h_gmap.as<uint64_t>();
    const uint64_t dev_bytes = build_gmap(mark, any ? gbase : UINT64_MAX, ng, gs, gmap);
    d.arena_bytes = dev_bytes;
    trace("staged + marked", s, t0);
    // 2. uploads: metadata + granule map first (the planner needs them)
    const uint64_t pieces = std::max<uint64_t>(1, (dev_bytes + piece_bytes - 1) / piece_bytes);
    const uint64_t chunks = long_blocks ? 2 * pieces : pieces;  // lane groups: (region, piece)
    d.arena.ensure(dev_bytes + msha::kArenaSlack);
    d.p_gmap.ensure(8 * ng);
    while (d.span_ev.size() < pieces) {
      hipEvent_t e;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      d.span_ev.push_back(e);
    }
    if (!meta_pinned) {
      HIPCHK(hipEventRecord(d.ev_up0, d.copy_stream));
      HIPCHK(hipMemcpyAsync(d.p_meta.p, h_off, 16 * m, hipMemcpyHostToDevice, d.copy_stream));
    }
    HIPCHK(hipMemcpyAsync(d.p_gmap.p, gmap, 8 * ng, hipMemcpyHostToDevice, d.copy_stream));
    HIPCHK(hipEventRecord(d.ev_meta, d.copy_stream));
    meta_queued[s] = 1;
    arrival.wait();  // shared GPU: every shard's metadata is queued before any planner or payload
    // 3. planning on the GPU, behind the metadata. Queued before the payload:
    // with streams of several shards sharing a GPU's hardware queues (HIP
    // multiplexes streams over GPU_MAX_HW_QUEUES), a planner queued behind
    // another stream's payload or kernel waits would wait for them too.
    // a message at or below an earlier start may repeat a payload: fold aliases
    // (a span test -- bytes > span -- missed a shard whose own messages are sparse
    // in the arena while its EpochChange re-hashes point back into a shared pool)
    const bool aliases = m > 1 && any && sh.backward;
    const uint64_t B = chunks * (sc.bmax + 1) <= (1u << 20) ? sc.bmax + 1 : 1;
    const uint64_t nb = chunks * B;
    uint64_t cap = 1024;
    while (cap < 2 * m) cap <<= 1;
    d.p_devoff.ensure(8 * m);
    d.p_rep.ensure(4 * m);
    d.p_cnt.ensure(4 * nb);
    d.p_small.ensure(4 * (2 * chunks + 2));
    if (aliases) {
      d.p_table.ensure(4 * cap);
      d.p_slot.ensure(4 * m);
    }
    d.off.ensure(8 * m);
    d.len.ensure(8 * m);
    d.order.ensure(4 * m);
    d.out.ensure(32 * m);
    d.err.ensure(4);
    d.h_out.ensure(32 * m + 4);
    d.h_small.ensure(4 * (2 * chunks + 2));
    if (aliases) d.h_rep.ensure(4 * m);
    if (aliases) HIPCHK(hipMemsetAsync(d.p_table.p, 0, 4 * cap, d.stream));
    HIPCHK(hipMemsetAsync(d.p_cnt.p, 0, 4 * nb, d.stream));
    HIPCHK(hipMemsetAsync(d.p_small.p, 0xFF, 4 * chunks, d.stream));  // gmin
    HIPCHK(hipMemsetAsync(d.err.p, 0, 4, d.stream));
    HIPCHK(hipStreamWaitEvent(d.stream, d.ev_meta, 0));
    HIPCHK(hipEventRecord(d.ev_p0, d.stream));
    msha::PlanArgs pa;
    pa.off = d.p_meta.as<uint64_t>();
    pa.len = pa.off + m;
    pa.gmap = d.p_gmap.as<uint64_t>();
    pa.glo = glo;
    pa.gbase = gbase;
    pa.gshift = gs;
    pa.m = m;
    pa.dev_off = d.p_devoff.as<uint64_t>();
    pa.table = aliases ? d.p_table.as<uint32_t>() : nullptr;
    pa.tmask = cap - 1;
    pa.slot = aliases ? d.p_slot.as<uint32_t>() : nullptr;
    pa.rep = d.p_rep.as<uint32_t>();
    pa.pieces = pieces;
    pa.piece_shift = piece_shift;
    pa.long_blocks = long_blocks;
    pa.chunks = chunks;
    pa.B = B;
    pa.bmax = sc.bmax;
    pa.nb = nb;
    pa.cnt = d.p_cnt.as<uint32_t>();
    pa.gmin = d.p_small.as<uint32_t>();
    pa.cut = pa.gmin + chunks;
    pa.info = pa.cut + chunks + 1;
    pa.lane_off = d.off.as<uint64_t>();
    pa.lane_len = d.len.as<uint64_t>();
    pa.lane_slot = d.order.as<uint32_t>();
    HIPCHK(msha::launch_plan(pa, d.stream));
    HIPCHK(hipEventRecord(d.ev_p1, d.stream));
    HIPCHK(hipMemcpyAsync(d.h_small.p, d.p_small.p, 4 * (2 * chunks + 2), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipEventRecord(d.ev_plan, d.stream));
    if (aliases) HIPCHK(hipMemcpyAsync(d.h_rep.p, d.p_rep.p, 4 * m, hipMemcpyDeviceToHost, d.stream));
    d.st.d2h_bytes = 4 * (2 * chunks + 2) + (aliases ? 4 * m : 0);
    // 4. the payload: behind every shard's metadata on a shared GPU
    arrival2.wait();  // shared GPU: every shard's planner is queued before any payload
    for (uint32_t o = 0; shared_gpu && o < k; ++o)
      if (o != s && meta_queued[o] && ctx->devs[o].id == d.id)
        HIPCHK(hipStreamWaitEvent(d.copy_stream, ctx->devs[o].ev_meta, 0));
    // 5. the plan's lane groups (read back once the planner is done), each
    // launched behind the upload piece that completes its payloads. The long
    // chains' groups (region 0: their payloads went up first), when they hold
    // at most head_cap lanes, run as heads: the two-lane chain kernel on CUs of
    // their own (k_digest_chain2 EXCL), on the side stream, so they start as
    // soon as their piece lands, beside the lane kernel, instead of crawling on
    // it (~2x the cycles per block) -- or ending the call when the caller packed
    // them last (weak #6 of round 3). Their digests go to p_head, lane-indexed,
    // and are placed after the sync (finish_shard).
    bool planned = false;
    size_t groups = 0, next_group = 0, next_head = 0;
    std::vector<std::pair<uint64_t, uint64_t>> head_groups;  // (lane cut, piece) of region-0 groups
    auto read_plan = [&] {
      d.st.plan_kernel_ms = elapsed_ms(d.ev_p0, d.ev_p1);
      const uint32_t* gmin = d.h_small.as<uint32_t>();
      const uint32_t* cut = gmin + chunks;
      P.lanes = cut[chunks];
      d.st.lanes = P.lanes;
      P.rep_dev = aliases ? d.h_rep.as<uint32_t>() : nullptr;
      const uint64_t head_lanes = long_blocks ? cut[pieces] : 0;  // region 0 = lanes [0, cut[pieces])
      const bool heads = head_lanes > 0 && head_lanes <= head_cap(d);
      P.head = heads ? head_lanes : 0;
      P.launched = P.head;
      d.st.head_lanes = (uint32_t)P.head;
      // lane groups: one per (region, piece) that completes at least one payload
      P.lane_cut.assign(1, P.head);
      P.cut_chunk.clear();
      head_groups.clear();
      std::vector<uint64_t> gm;
      for (uint64_t q = 0; q < chunks; ++q) {
        if (cut[q + 1] == cut[q]) continue;
        if (heads && q < pieces) {
          head_groups.push_back({cut[q + 1], q});
          continue;
        }
        P.lane_cut.push_back(cut[q + 1]);
        P.cut_chunk.push_back(q % pieces);
        gm.push_back(gmin[q]);
      }
      groups = gm.size();
      P.later_min.assign(groups + 1, m);
      for (size_t g = groups; g-- > 0;) P.later_min[g] = std::min<uint64_t>(gm[g], P.later_min[g + 1]);
      if (heads) {
        d.p_head.ensure(32 * P.head);
        d.h_head.ensure(36 * P.head);
      }
      planned = true;
      trace("planned on GPU", s, t0);
    };
    auto launch_upto = [&](uint64_t pieces_queued) {  // pieces [0, pieces_queued) have their events
      for (; next_head < head_groups.size() && head_groups[next_head].second < pieces_queued; ++next_head)
        launch_head(ctx, d, P, next_head ? head_groups[next_head - 1].first : 0, head_groups[next_head].first,
                    d.span_ev[head_groups[next_head].second], t0);
      for (; next_group < groups && P.cut_chunk[next_group] < pieces_queued; ++next_group) {
        HIPCHK(hipStreamWaitEvent(d.stream, d.span_ev[P.cut_chunk[next_group]], 0));
        launch_lanes(ctx, d, P, next_group, next_group + 1 == groups, t0, out, out_pinned);
      }
    };
    // event c once every byte below device offset (c+1)*piece_bytes is queued
    uint64_t c = 0, uploaded = 0;
    auto pieces_done = [&](uint64_t dev_end) {
      for (; c < pieces && (c + 1) * piece_bytes <= dev_end; ++c) HIPCHK(hipEventRecord(d.span_ev[c], d.copy_stream));
    };
    unsigned slot_i = 0;
    if (staged) {  // two pinned staging slots, refilled as their H2D drains
      d.slot[0].ensure(kChunkBytes);
      d.slot[1].ensure(kChunkBytes);
      HIPCHK(hipEventRecord(d.slot_free[0], d.copy_stream));
      HIPCHK(hipEventRecord(d.slot_free[1], d.copy_stream));
    }
    if (any)
      for_each_upload(gmap, mark, ng, gbase, glo, gs, sh.lo, sh.hi, [&](uint64_t pos, uint64_t dev, uint64_t bytes) {
        if (!staged) {  // the caller's pinned bytes, DMA'd as they are
          HIPCHK(hipMemcpyAsync(d.arena.as<uint8_t>() + dev, arena + pos, bytes, hipMemcpyHostToDevice,
                                d.copy_stream));
          uploaded += bytes;
          pieces_done(dev + bytes);
          return;
        }
        // pageable: copied into a staging slot by the shard's threads (large
        // contiguous runs, not message by message), then DMA'd; kernels start
        // as their pieces land and the planner's result is in
        for (uint64_t o = 0; o < bytes;) {
          const uint64_t take = std::min(bytes - o, slot_bytes);
          const unsigned si = slot_i++ & 1;
          HIPCHK(hipEventSynchronize(d.slot_free[si]));
          if (slot_delay_us) std::this_thread::sleep_for(std::chrono::microseconds(slot_delay_us));
          const double g0 = now_ms();
          copy_threads(d.slot[si].as<uint8_t>(), arena + pos + o, take);
          const double g1 = now_ms();
          if (d.st.gather_begin_ms == 0) d.st.gather_begin_ms = std::max(g0 - t0, 1e-6);
          d.st.gather_end_ms = g1 - t0;
          d.st.gather_ms += g1 - g0;
          HIPCHK(hipMemcpyAsync(d.arena.as<uint8_t>() + dev + o, d.slot[si].p, take, hipMemcpyHostToDevice,
                                d.copy_stream));
          HIPCHK(hipEventRecord(d.slot_free[si], d.copy_stream));
          o += take;
          uploaded += take;
          pieces_done(dev + o);
          if (!planned && event_done(d.ev_plan)) read_plan();
          if (planned) launch_upto(c);
        }
      }, piece_bytes);
    for (; c < pieces; ++c) HIPCHK(hipEventRecord(d.span_ev[c], d.copy_stream));
    HIPCHK(hipEventRecord(d.ev_up1, d.copy_stream));
    d.st.h2d_payload_bytes = uploaded;
    d.st.h2d_bytes = 16 * m + 8 * ng;
    trace("payload queued", s, t0);
    if (!planned) {
      HIPCHK(hipEventSynchronize(d.ev_plan));
      read_plan();
    }
    launch_upto(pieces);
    queue_tail(d, P, out, out_pinned);
    finish_shard(ctx, s, out, out_pinned, t0);
  });
  double t_plan = t0;  // plan_ms: until the last shard's first kernel is queued
  for (const Device& d : ctx->devs) t_plan = std::max(t_plan, t0 + d.st.first_launch_ms);
  call_stats(ctx, t0, t_plan);
}

}  // namespace msha
