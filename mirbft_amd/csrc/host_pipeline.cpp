// The shard steps of a host call that the gather pipeline (host_pipeline.hpp
// run_pipeline) and the direct path (host_direct.cpp run_direct) share.
#include "host_pipeline.hpp"

namespace msha {

namespace {

// Re-run shard s of a host call in one unsplit launch over all its lanes, after
// a split-chain handoff timed out (error bit 2: some of its digests are
// undefined). Its payload and metadata are still on the device. Synchronous.
void rerun_unsplit(msha_ctx* ctx, Device& d, const Plan& P, uint8_t* d2h_dst) {
  HIPCHK(hipSetDevice(d.id));
  HIPCHK(hipMemsetAsync(d.err.p, 0, 4, d.stream));
  msha::LaunchKind kind;
  HIPCHK(msha::launch_digest_batch(d.arena.as<uint8_t>(), d.off.as<uint64_t>(), d.len.as<uint64_t>(),
                                   nullptr, P.ordered ? d.order.as<uint32_t>() : nullptr, P.lanes,
                                   d.out.as<uint8_t>(), d.err.as<uint32_t>(), d.cus, ctx->kernel_policy,
                                   d.stream, nullptr, &kind));
  count_launch(ctx, &d, kind);
  HIPCHK(hipMemcpyAsync(d2h_dst, d.out.p, 32 * P.m, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(d.h_out.as<uint8_t>() + 32 * P.m, d.err.p, 4, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  __atomic_fetch_add(&ctx->stats.split_retries, 1, __ATOMIC_RELAXED);
}

}  // namespace

// Launch shard d's lanes accumulated since its last launch, up to the end of
// lane group c, once they fill the GPU (2 waves per SIMD) or at the last group:
// hashing runs ~30x faster than PCIe delivers bytes, so a launch per group would
// only buy overlap worth a few % while a group of large messages (512 x 64 KiB)
// leaves most SIMDs idle for the whole of its long chains. Then bring back the
// digests that are final: identity lanes' own slots, or (ordered lanes with
// later_min) every slot below the lowest slot a later group writes -- into the
// caller's buffer itself when it is pinned -- while later groups upload.
// The stream a host call's digest D2H goes on: d2h_stream, ordered after
// everything queued so far on `after` (its kernels). On the kernel stream itself
// a D2H would hold up the next launch for as long as the copy takes, and on a
// box whose PCIe writes are slowed by other traffic that delayed c5's last
// kernels by up to 9 ms. MSHA_D2H_STREAM=0 keeps the D2H on the kernel stream
// (A/B, tools/ab_d2h.py). Shards sharing one GPU (MSHA_VIRTUAL_SHARDS) keep it
// on the kernel stream: HIP multiplexes streams over GPU_MAX_HW_QUEUES (4)
// hardware queues per device, and a third stream per shard put D2H waits in
// front of other shards' uploads (c5 at 2 virtual shards 71.5 -> 89 ms per call).
hipStream_t d2h_stream_after(Device& d, hipStream_t after) {
  if (!d.d2h_stream || env_u64("MSHA_D2H_STREAM", 1) == 0) return after;
  HIPCHK(hipEventRecord(d.ev_k, after));
  HIPCHK(hipStreamWaitEvent(d.d2h_stream, d.ev_k, 0));
  return d.d2h_stream;
}

void launch_lanes(msha_ctx* ctx, Device& d, Plan& P, size_t c, bool last, double t0, uint8_t* out,
                  bool out_pinned) {
  const uint64_t q1 = P.lane_cut[c + 1];
  const uint64_t fill = (uint64_t)d.cus * 4 * 64 * 2;
  if (!last && q1 - P.launched < fill) return;
  const uint64_t l0 = P.launched, lanes = q1 - l0;
  P.launched = q1;
  if (!P.k0) {
    HIPCHK(hipEventRecord(d.ev_k0, d.stream));
    d.st.first_launch_ms = now_ms() - t0;
    P.k0 = true;
    trace("first launch", d.index, t0);
  }
  // off/len are lane-indexed; out_idx maps lane -> shard-local message
  // (identity placement: lane q is message q)
  msha::SplitPlan sp;
  msha::LaunchKind kind;
  HIPCHK(msha::launch_digest_batch(
      d.arena.as<uint8_t>(), d.off.as<uint64_t>() + l0, d.len.as<uint64_t>() + l0, nullptr,
      P.ordered ? d.order.as<uint32_t>() + l0 : nullptr, lanes,
      d.out.as<uint8_t>() + (P.ordered ? 0 : 32 * l0), d.err.as<uint32_t>(), d.cus,
      ctx->kernel_policy, d.stream, split_for(d, lanes, ctx->kernel_policy, sp), &kind));
  count_launch(ctx, &d, kind);
  uint8_t* dst = out_pinned ? out + 32 * d.lo : d.h_out.as<uint8_t>();
  const bool d2h = P.identity() || (!P.later_min.empty() && P.later_min[c + 1] > P.d2h_done);
  hipStream_t ds = d2h ? d2h_stream_after(d, d.stream) : d.stream;
  if (P.identity()) {
    HIPCHK(hipMemcpyAsync(dst + 32 * l0, d.out.as<uint8_t>() + 32 * l0, 32 * lanes, hipMemcpyDeviceToHost, ds));
    d.st.d2h_bytes += 32 * lanes;
  } else if (!P.later_min.empty()) {
    // aliases among the streamed slots are filled on the host after the sync
    const uint64_t x = P.later_min[c + 1];
    if (x > P.d2h_done) {
      HIPCHK(hipMemcpyAsync(dst + 32 * P.d2h_done, d.out.as<uint8_t>() + 32 * P.d2h_done, 32 * (x - P.d2h_done),
                            hipMemcpyDeviceToHost, ds));
      d.st.d2h_bytes += 32 * (x - P.d2h_done);
      P.d2h_done = x;
    }
  }
}

// At most this many long lanes run as heads (two-lane chains, 64 per CU): half
// the CUs. More long chains than that fill the GPU by themselves, and the lane
// kernel runs them.
uint64_t head_cap(const Device& d) { return (uint64_t)d.cus * msha::kChain2MsgsPerWg / 2; }

// Lanes [l0, l1) of shard d (long chains, lane-indexed metadata) as a head:
// k_digest_chain2 with CUs of its own, behind the upload piece `piece_in`,
// digests lane-indexed into p_head. On a GPU of its own the heads go on the
// side stream and run beside the lane kernel; on a shared GPU
// (MSHA_VIRTUAL_SHARDS) a third stream per shard would contend for the GPU's
// hardware queues (d2h_stream_after), so they go on the kernel stream.
void launch_head(msha_ctx* ctx, Device& d, Plan& P, uint64_t l0, uint64_t l1, hipEvent_t piece_in, double t0) {
  hipStream_t hs = d.stream;
  d.head_side = d.d2h_stream != nullptr;
  if (d.head_side) {
    if (!d.side_stream) HIPCHK(hipStreamCreateWithFlags(&d.side_stream, hipStreamNonBlocking));
    if (!d.ev_head) HIPCHK(hipEventCreateWithFlags(&d.ev_head, hipEventDisableTiming));
    hs = d.side_stream;
  }
  HIPCHK(hipStreamWaitEvent(hs, piece_in, 0));
  if (!P.k0) {
    HIPCHK(hipEventRecord(d.ev_k0, hs));
    d.st.first_launch_ms = now_ms() - t0;
    P.k0 = true;
    trace("first launch (head)", d.index, t0);
  }
  msha::LaneGate hg;
  hg.head_part = true;
  hg.two_lane = true;
  msha::LaunchKind kind;
  HIPCHK(msha::launch_digest_batch(d.arena.as<uint8_t>(), d.off.as<uint64_t>() + l0, d.len.as<uint64_t>() + l0,
                                   nullptr, nullptr, l1 - l0, d.p_head.as<uint8_t>() + 32 * l0, d.err.as<uint32_t>(),
                                   d.cus, MSHA_KERNEL_COOP, hs, nullptr, &kind, &hg));
  count_launch(ctx, &d, kind);
  if (d.head_side) HIPCHK(hipEventRecord(d.ev_head, hs));
}

// Queue the end of shard d's call on its stream: ev1 after its last kernel,
// the digest slots not streamed back yet, the error word.
void queue_tail(Device& d, Plan& P, uint8_t* out, bool out_pinned) {
  const uint64_t m = P.m;
  if (m == 0) return;
  HIPCHK(hipSetDevice(d.id));
  if (P.head) {  // the heads' digests and their lanes' slots, behind the heads
    if (d.head_side) HIPCHK(hipStreamWaitEvent(d.stream, d.ev_head, 0));
    HIPCHK(hipMemcpyAsync(d.h_head.p, d.p_head.p, 32 * P.head, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipMemcpyAsync(d.h_head.as<uint8_t>() + 32 * P.head, d.order.p, 4 * P.head, hipMemcpyDeviceToHost,
                          d.stream));
    d.st.d2h_bytes += 36 * P.head;
  }
  HIPCHK(hipEventRecord(d.ev1, d.stream));
  const hipStream_t ds = d2h_stream_after(d, d.stream);
  const uint64_t done = P.d2h_done;  // slots streamed back after earlier launches
  if (!P.identity() && done < m) {
    // d.out is message-ordered (lane q wrote its message's slot); a pinned result
    // buffer takes it as is, the aliases' slots are filled on the host afterwards
    HIPCHK(hipMemcpyAsync((out_pinned ? out + 32 * d.lo : d.h_out.as<uint8_t>()) + 32 * done,
                          d.out.as<uint8_t>() + 32 * done, 32 * (m - done), hipMemcpyDeviceToHost, ds));
    d.st.d2h_bytes += 32 * (m - done);
  }
  HIPCHK(hipMemcpyAsync(d.h_out.as<uint8_t>() + 32 * m, d.err.p, 4, hipMemcpyDeviceToHost, ds));
  d.st.d2h_bytes += 4;
}

float elapsed_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  HIPCHK(hipEventSynchronize(b));
  HIPCHK(hipEventElapsedTime(&ms, a, b));
  return ms;
}

// Finish shard s of a host call, on the shard's own thread (shards finish side
// by side): wait for its stream, re-run it unsplit if a split chain's hand-off
// timed out, fill its aliases' digests (each copies its representative's) and
// complete its msha_shard_stats: device_ms = first upload .. last kernel,
// upload_ms = first .. last upload, kernel_ms = first kernel .. last (HIP events).
void finish_shard(msha_ctx* ctx, uint32_t s, uint8_t* out, bool out_pinned, double t0) {
  Device& d = ctx->devs[s];
  Plan& P = ctx->plans[s];
  const uint64_t m = P.m;
  if (m == 0) return;
  HIPCHK(hipSetDevice(d.id));
  HIPCHK(hipStreamSynchronize(d.stream));
  if (d.d2h_stream) HIPCHK(hipStreamSynchronize(d.d2h_stream));
  d.st.device_ms = elapsed_ms(d.ev_up0, d.ev1);
  d.st.upload_ms = elapsed_ms(d.ev_up0, d.ev_up1);
  d.st.kernel_ms = elapsed_ms(d.ev_k0, d.ev1);
  if (trace_on())
    fprintf(stderr, "[msha] shard %u %-16s %9.2f ms (device %.2f, upload %.2f, kernels %.2f ms)\n", s, "synced",
            now_ms() - t0, d.st.device_ms, d.st.upload_ms, d.st.kernel_ms);
  uint32_t errflag;
  std::memcpy(&errflag, d.h_out.as<uint8_t>() + 32 * m, 4);
  const bool straight = out_pinned;  // the digests were D2H'd straight into out
  if (errflag & 2) {
    // a split chain's handoff timed out: its digests are undefined; the
    // payload is still on the device, so re-hash the shard unsplit
    rerun_unsplit(ctx, d, P, straight ? out + 32 * d.lo : d.h_out.as<uint8_t>());
    d.st.d2h_bytes += 32 * m + 4;
    std::memcpy(&errflag, d.h_out.as<uint8_t>() + 32 * m, 4);
    if (errflag & 2) throw MshaError(MSHA_ERR_HIP, "split-chain handoff timed out (re-run failed)");
  }
  if (errflag) throw MshaError(MSHA_ERR_ALIGNMENT, "internal: misaligned staged message");
  d.st.h2d_bytes += d.st.h2d_payload_bytes;
  const uint32_t* rep = P.rep_of();
  const uint8_t* h = d.h_out.as<uint8_t>();
  if (P.head) {  // the heads' digests into their slots (before the aliases copy them)
    const uint8_t* hd = d.h_head.as<uint8_t>();
    const uint32_t* slot = reinterpret_cast<const uint32_t*>(hd + 32 * P.head);
    uint8_t* base = straight ? out + 32 * d.lo : d.h_out.as<uint8_t>();
    for (uint64_t i = 0; i < P.head; ++i) std::memcpy(base + 32 * (uint64_t)slot[i], hd + 32 * i, 32);
  }
  if (straight) {
    if (rep)  // aliases copy their representative's digest
      parallel_chunks(m, plan_threads(m), [&](unsigned, uint64_t a, uint64_t b) {
        uint8_t* o = out + 32 * d.lo;
        for (uint64_t i = a; i < b; ++i)
          if (rep[i] != i) std::memcpy(o + 32 * i, o + 32 * (uint64_t)rep[i], 32);
      });
    return;
  }
  parallel_chunks(m, plan_threads(m), [&](unsigned, uint64_t a, uint64_t b) {
    if (!rep)
      std::memcpy(out + 32 * (d.lo + a), h + 32 * a, 32 * (b - a));
    else
      for (uint64_t i = a; i < b; ++i) std::memcpy(out + 32 * (d.lo + i), h + 32 * (uint64_t)rep[i], 32);
  });
}

// The call's figures (msha_stats) from its finished shards'.
void call_stats(msha_ctx* ctx, double t0, double t_plan) {
  double device_ms = 0, gather_ms = 0;
  uint64_t h2d = 0, d2h = 0;
  for (uint32_t s = 0; s < (uint32_t)ctx->devs.size(); ++s) {
    if (ctx->plans[s].m == 0) continue;
    const msha_shard_stats& st = ctx->devs[s].st;
    device_ms = std::max(device_ms, st.device_ms);
    gather_ms += st.gather_ms;
    h2d += st.h2d_bytes;
    d2h += st.d2h_bytes;
  }
  ctx->stats.calls++;
  ctx->stats.plan_ms = t_plan - t0;
  ctx->stats.pack_ms = gather_ms;
  ctx->stats.device_ms = device_ms;
  ctx->stats.h2d_bytes = h2d;
  ctx->stats.d2h_bytes = d2h;
  ctx->stats.total_ms = now_ms() - t0;
}

}  // namespace msha
