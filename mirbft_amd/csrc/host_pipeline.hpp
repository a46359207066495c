// The gather pipeline of the host entries (run_pipeline, a template over the per-message
// gather each entry passes, inlined into the staging loop) and the shard steps it shares
// with the direct path (host_direct.cpp): launching lanes and heads, queueing the tail,
// finishing a shard, the call's figures. Their bodies are in host_pipeline.cpp.
#pragma once
#include <unordered_map>

#include "ctx.hpp"

namespace msha {

// Host-memory execution of one batch (the body of every host entry point):
//   shard messages [0, n) over the context's GPUs by cumulative block count;
//   per GPU, give one lane to each distinct payload (aliases fold into their
//   first occurrence), order lanes by descending block count (a wave's lanes
//   then run equal block counts), place the payloads at 16-byte aligned
//   offsets of the device arena, upload lane-indexed off/len + the lane ->
//   message map, and stream the payload in chunks through two pinned staging
//   slots: host threads gather chunk c+1 while chunk c's H2D runs on the copy
//   stream. Kernels (compute stream, event-ordered after their chunks) run over
//   accumulated chunks once these fill the GPU, or at the last chunk. Digests
//   come back with one D2H per GPU; aliases copy their representative's.
//   gather(i, dst) copies message i's bytes to dst.
constexpr uint64_t kChunkBytes = 32ull << 20;

// uid (may be null): messages with equal uid[i] have identical bytes (aliases,
// e.g. one EpochChange re-hashed N^2 times, epoch_target.go:486-505); their
// payload is copied and hashed once per GPU.
// t0: when the entry point was called (plan_ms includes its validation).

// Launch shard d's accumulated lanes up to the end of lane group c (host_pipeline.cpp).
hipStream_t d2h_stream_after(Device& d, hipStream_t after);
void launch_lanes(msha_ctx* ctx, Device& d, Plan& P, size_t c, bool last, double t0, uint8_t* out,
                  bool out_pinned);
uint64_t head_cap(const Device& d);
void launch_head(msha_ctx* ctx, Device& d, Plan& P, uint64_t l0, uint64_t l1, hipEvent_t piece_in, double t0);
void queue_tail(Device& d, Plan& P, uint8_t* out, bool out_pinned);
float elapsed_ms(hipEvent_t a, hipEvent_t b);
void finish_shard(msha_ctx* ctx, uint32_t s, uint8_t* out, bool out_pinned, double t0);
void call_stats(msha_ctx* ctx, double t0, double t_plan);

template <class Gather>
void run_pipeline(msha_ctx* ctx, double t0, uint64_t n, const uint64_t* len, const uint64_t* uid,
                  uint8_t* out, Gather&& gather, const uint64_t* pre_bounds = nullptr) {
  const uint32_t k = (uint32_t)ctx->devs.size();
  const bool out_pinned = is_pinned_host(out) && is_pinned_host(out + 32 * n - 1);
  std::vector<uint64_t> bounds(k + 1);
  if (pre_bounds) std::copy(pre_bounds, pre_bounds + k + 1, bounds.begin());
  else partition(len, n, k, bounds.data());

  std::vector<Plan>& plans = ctx->plans;
  plans.resize(k);
  for (uint32_t s = 0; s < k; ++s) {
    Plan& P = plans[s];
    P.m = 0;
    P.next = 0;
    P.launched = 0;
    P.d2h_done = 0;
    P.later_min.clear();
    P.rep_dev = nullptr;
    P.head = 0;
    P.k0 = false;
    msha_shard_stats& st = ctx->devs[s].st;
    st = msha_shard_stats{};
    st.device = ctx->devs[s].id;
  }
  for (uint32_t s = 0; s < k; ++s) {
    ctx->devs[s].lo = bounds[s];
    ctx->devs[s].hi = bounds[s + 1];
  }
  // Plan every shard (several GPUs: side by side, for_each_shard).
  for_each_shard(ctx, [&](uint32_t s) {
    Device& d = ctx->devs[s];
    Plan& P = plans[s];
    P.m = d.hi - d.lo;
    d.st.messages = P.m;
    if (P.m == 0) return;
    // this GPU current before any staging allocation: without
    // hipHostMallocNumaUser the runtime takes pinned memory from the host pool
    // of the current device's nearest CPU agent (its NUMA node)
    HIPCHK(hipSetDevice(d.id));
    const uint64_t* L = len + d.lo;
    // Aliases (same uid) have identical bytes, hence identical digests: only
    // the first message of each uid gets a lane; the others copy its digest
    // after the D2H (EpochChange re-hashing, epoch_target.go:486-505).
    P.rep.clear();
    P.lanes = P.m;
    if (uid && k == 1) {  // one shard: uid[i] (the first index with i's payload) is the lane's message
      P.rep.resize(P.m);
      const unsigned T = plan_threads(P.m);
      std::vector<uint64_t> nl(T, 0);
      parallel_chunks(P.m, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
        uint64_t c = 0;
        for (uint64_t i = lo; i < hi; ++i) {
          P.rep[i] = (uint32_t)uid[i];
          c += uid[i] == i;
        }
        nl[t] = c;
      });
      P.lanes = 0;
      for (uint64_t c : nl) P.lanes += c;
      if (P.lanes == P.m) P.rep.clear();
    } else if (uid) {
      // rep[i] = the shard-local index of the shard's first message with i's
      // payload. uid[i] (the batch-wide first occurrence) at or past the shard's
      // start lies in this shard, so it is also the shard's first: threaded.
      // An earlier uid (a payload first seen by an earlier shard, e.g. the shared
      // EpochChange pool) is resolved in index order through `placed`, over
      // those messages only.
      P.rep.resize(P.m);
      const unsigned T = plan_threads(P.m);
      std::vector<uint64_t> nl(T, 0);
      std::vector<std::vector<uint32_t>> cross(T);
      parallel_chunks(P.m, T, [&](unsigned t, uint64_t a, uint64_t b) {
        uint64_t c = 0;
        for (uint64_t i = a; i < b; ++i) {
          const uint64_t u = uid[d.lo + i];
          if (u >= d.lo) {
            P.rep[i] = (uint32_t)(u - d.lo);
            c += u == d.lo + i;
          } else {
            cross[t].push_back((uint32_t)i);
          }
        }
        nl[t] = c;
      });
      P.lanes = 0;
      for (uint64_t c : nl) P.lanes += c;
      uint64_t ncross = 0;
      for (const std::vector<uint32_t>& v : cross) ncross += v.size();
      std::unordered_map<uint64_t, uint32_t> first;  // uid -> the shard's first message with it
      first.reserve(std::min<uint64_t>(ncross, 1u << 16));
      for (const std::vector<uint32_t>& v : cross)
        for (uint32_t i : v) {
          const auto it = first.try_emplace(uid[d.lo + i], i);
          P.rep[i] = it.first->second;
          P.lanes += it.second;
        }
      if (P.lanes == P.m) P.rep.clear();
    }
    d.st.lanes = P.lanes;
    trace("representatives", t0);
    P.perm.resize(P.lanes);
    d.h_meta.ensure(16 * P.m + 4 * P.m);
    uint64_t* h_off = d.h_meta.as<uint64_t>();
    uint64_t* h_len = h_off + P.m;
    if (!P.rep.empty()) {  // lanes = the representatives, by descending block count
      order_by_blocks_desc(L, P.m, P.perm.data(), d.sort_tmp, P.rep.data());
      P.ordered = true;
    } else {
      P.ordered = !all_equal_blocks(L, P.m);
      if (P.ordered) order_by_blocks_desc(L, P.m, P.perm.data(), d.sort_tmp);
      else for (uint64_t i = 0; i < P.m; ++i) P.perm[i] = (uint32_t)i;
    }
    trace("lane order", t0);
    // Place payloads in lane order (each lane's payload is distinct: aliases
    // were folded into their representative above), so every lane of chunk c
    // reads bytes uploaded by the end of chunk c.
    uint64_t acc = 0;
    {
      // lane-indexed metadata: an exclusive scan of the 16-byte-rounded lengths
      // (lane q's payload lands at h_off[q]; payloads are placed in lane order)
      const unsigned T = plan_threads(P.lanes);
      std::vector<uint64_t> part(T + 1, 0);
      parallel_chunks(P.lanes, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
        uint64_t a = 0;
        for (uint64_t q = lo; q < hi; ++q) {
          const uint64_t l = L[P.perm[q]];
          h_len[q] = l;
          a += round16(l);
        }
        part[t + 1] = a;
      });
      for (unsigned t = 0; t < T; ++t) part[t + 1] += part[t];
      parallel_chunks(P.lanes, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
        uint64_t a = part[t];
        for (uint64_t q = lo; q < hi; ++q) {
          h_off[q] = a;
          a += round16(h_len[q]);
        }
      });
      acc = part[T];
      // greedy chunks of >= kChunkBytes: cut after the first lane whose end
      // reaches the chunk's start + kChunkBytes (binary search on the scan)
      P.lane_cut.assign(1, 0);
      for (uint64_t q0 = 0;;) {
        const uint64_t target = h_off[q0] + kChunkBytes;
        const uint64_t r = (uint64_t)(std::lower_bound(h_off + q0 + 1, h_off + P.lanes, target) - h_off);
        if (r >= P.lanes) break;  // the rest (ending at acc) is the last chunk
        P.lane_cut.push_back(r);
        q0 = r;
      }
      P.lane_cut.push_back(P.lanes);
    }
    d.arena_bytes = acc;
    trace("placement", t0);
    if (P.ordered) std::memcpy(h_len + P.m, P.perm.data(), 4 * P.lanes);
    {
      uint64_t slot_bytes = 0;
      for (size_t c = 0; c + 1 < P.lane_cut.size(); ++c) {
        const uint64_t e = P.lane_cut[c + 1] < P.lanes ? h_off[P.lane_cut[c + 1]] : acc;
        slot_bytes = std::max(slot_bytes, e - h_off[P.lane_cut[c]]);
      }
      d.slot[0].ensure(std::max<uint64_t>(slot_bytes, 16));
      d.slot[1].ensure(std::max<uint64_t>(slot_bytes, 16));
    }
    HIPCHK(hipSetDevice(d.id));
    d.arena.ensure(acc + msha::kArenaSlack);
    d.h_out.ensure(32 * P.m + 4);
    d.off.ensure(8 * P.m);
    d.len.ensure(8 * P.m);
    d.out.ensure(32 * P.m);
    d.err.ensure(4);
    if (P.ordered) d.order.ensure(4 * P.lanes);
    HIPCHK(hipEventRecord(d.ev_up0, d.stream));
    HIPCHK(hipMemcpyAsync(d.off.p, h_off, 8 * P.lanes, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipMemcpyAsync(d.len.p, h_len, 8 * P.lanes, hipMemcpyHostToDevice, d.stream));
    d.st.h2d_bytes = 16 * P.lanes;
    if (P.ordered) {
      HIPCHK(hipMemcpyAsync(d.order.p, h_len + P.m, 4 * P.lanes, hipMemcpyHostToDevice, d.stream));
      d.st.h2d_bytes += 4 * P.lanes;
    }
    HIPCHK(hipMemsetAsync(d.err.p, 0, 4, d.stream));
    HIPCHK(hipEventRecord(d.ev0, d.stream));
    HIPCHK(hipStreamWaitEvent(d.copy_stream, d.ev0, 0));  // uploads start after ev0: device_ms spans them
    HIPCHK(hipEventRecord(d.slot_free[0], d.copy_stream));
    HIPCHK(hipEventRecord(d.slot_free[1], d.copy_stream));
  });
  const double t_plan = now_ms();
  trace("planned (metadata H2D queued)", t0);

  // Issue chunk P.next of shard s: gather it into a staging slot, upload it, and
  // launch the lanes accumulated so far when they fill the GPU (launch_lanes).
  // Returns whether shard s has chunks left.
  auto issue_chunk = [&](uint32_t s, WorkerPool& pool) -> bool {
    Device& d = ctx->devs[s];
    Plan& P = plans[s];
    if (P.m == 0 || P.next + 1 >= P.lane_cut.size()) return false;
    const size_t c = P.next++;
    const uint64_t u0 = P.lane_cut[c], u1 = P.lane_cut[c + 1];
    const uint64_t* h_off = d.h_meta.as<uint64_t>();  // lane -> arena offset
    HIPCHK(hipSetDevice(d.id));
    const uint64_t b0 = h_off[u0];
    const uint64_t b1 = u1 >= P.lanes ? d.arena_bytes : h_off[u1];
    PinBuf& slot = d.slot[c & 1];
    HIPCHK(hipEventSynchronize(d.slot_free[c & 1]));  // its previous H2D has drained
    const double g0 = now_ms();
    uint8_t* dst = slot.as<uint8_t>();
    parallel_ranges(pool, u1 - u0, b1 - b0, [&](uint64_t a, uint64_t b) {
      for (uint64_t u = u0 + a; u < u0 + b; ++u) gather(d.lo + P.perm[u], dst + (h_off[u] - b0));
    });
    const double g1 = now_ms();
    if (d.st.gather_begin_ms == 0) d.st.gather_begin_ms = std::max(g0 - t0, 1e-6);
    d.st.gather_end_ms = g1 - t0;
    d.st.gather_ms += g1 - g0;
    if (b1 > b0)
      HIPCHK(hipMemcpyAsync(d.arena.as<uint8_t>() + b0, slot.p, b1 - b0, hipMemcpyHostToDevice,
                            d.copy_stream));
    d.st.h2d_payload_bytes += b1 - b0;
    HIPCHK(hipEventRecord(d.slot_free[c & 1], d.copy_stream));
    HIPCHK(hipEventRecord(d.chunk_in, d.copy_stream));
    const bool last = P.next + 1 >= P.lane_cut.size();
    if (last) HIPCHK(hipEventRecord(d.ev_up1, d.copy_stream));
    HIPCHK(hipStreamWaitEvent(d.stream, d.chunk_in, 0));
    launch_lanes(ctx, d, P, c, last, t0, out, out_pinned);
    return !last;
  };
  if (k > 1) {
    // Pageable arenas over several GPUs: one issuing thread per GPU, each with
    // its own gather helpers, so the host copy for GPU s+1 never waits on GPU
    // s's staging slot (msha_shard_stats gather_begin/end show the overlap).
    for_each_shard(ctx, [&](uint32_t s) {
      while (issue_chunk(s, cur_pool())) {
      }
    });
  } else {
    // One GPU: the calling thread issues its chunks.
    for (bool more = true; more;) {
      more = false;
      for (uint32_t s = 0; s < k; ++s) more |= issue_chunk(s, WorkerPool::get());
    }
  }
  for_each_shard(ctx, [&](uint32_t s) {
    queue_tail(ctx->devs[s], plans[s], out, out_pinned);
    finish_shard(ctx, s, out, out_pinned, t0);
  });
  call_stats(ctx, t0, t_plan);
}

}  // namespace msha
