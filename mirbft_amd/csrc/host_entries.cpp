// The host-memory entries of libmirsha (C ABI in include/mirsha.h).
//
// One call == one processor.ProcessHashActions over a whole ActionList
// (MirBFT's pkg/processor/serial.go:180-198): validate, pack into
// pinned staging, shard across the context's GPUs by cumulative block count,
// H2D per shard on that GPU's stream, one kernel launch per shard, D2H of the
// digests, join. There is no collective and no CPU hashing anywhere here.
// Each entry validates, then takes the latency path (host_small.hpp), the direct path
// (host_direct.hpp) or the gather pipeline (host_pipeline.hpp); the pure planning
// wrappers (msha_blocks_for_len .. msha_alias_first) expose host_plan.hpp to the tests.
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "host_direct.hpp"
#include "host_pipeline.hpp"
#include "host_small.hpp"

using namespace msha;

extern "C" {

uint64_t msha_blocks_for_len(uint64_t len) { return blocks_for(len); }

int msha_order_by_blocks(const uint64_t* len, uint64_t n, uint32_t* order) {
  if (n && (!len || !order)) return MSHA_ERR_INVALID_ARG;
  if (n > 0xffffffffull) return MSHA_ERR_INVALID_ARG;
  try {
    std::vector<uint32_t> tmp;
    order_by_blocks_desc(len, n, order, tmp);
  } catch (...) {
    return MSHA_ERR_OUT_OF_MEMORY;
  }
  return MSHA_OK;
}

int msha_partition_by_blocks(const uint64_t* len, uint64_t n, uint32_t n_shards, uint64_t* bounds) {
  if (!bounds || n_shards == 0 || (n && !len)) return MSHA_ERR_INVALID_ARG;
  partition(len, n, n_shards, bounds);
  return MSHA_OK;
}

int msha_alias_first(const uint64_t* off, const uint64_t* len, uint64_t n, uint64_t* first) {
  if (n && (!off || !len || !first)) return MSHA_ERR_INVALID_ARG;
  if (n >= 0xffffffffull) return MSHA_ERR_INVALID_ARG;
  try {
    std::vector<uint64_t> uid, table, bucket;
    std::vector<uint32_t> tag;
    alias_uids(off, len, n, uid, table, bucket, tag);
    std::memcpy(first, uid.data(), 8 * n);
  } catch (...) {
    return MSHA_ERR_OUT_OF_MEMORY;
  }
  return MSHA_OK;
}

int msha_digest_batch(msha_ctx* ctx, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                      const uint64_t* len, uint64_t n, uint8_t* out) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (!off || !len || !out || (arena_len && !arena))
    return fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (n >= 0xffffffffull) return fail(ctx, MSHA_ERR_INVALID_ARG, "more than 2^32-2 messages in one call");
  const double t0 = now_ms();
  return guarded(ctx, [&] {
    EarlyMeta early(ctx, off, len, n);
    BatchScan sc;
    scan_batch(arena, arena_len, off, len, n, sc);
    const uint64_t lo = sc.lo, hi = sc.hi, sum = sc.sum;
    const bool aligned16 = (sc.offbits & 15) == 0;
    auto count = [&] {
      ctx->stats.messages += n;
      ctx->stats.message_bytes += sum;
      ctx->stats.blocks += sc.blocks;
    };
    if (n <= small_msgs()) {  // the latency path (run_small)
      // A pinned arena goes up as is only above 512 KiB: below that, packing it
      // behind the metadata (one H2D instead of two) is the faster of the two
      // (tools/latency.cpp: 32 KiB pinned 57 us as two copies, 44 us packed).
      const bool span = small_bytes() > 0 && aligned16 && hi - lo > kSmallSpanMin &&
                        hi - lo <= small_span_bytes() && is_pinned_host(arena + lo) &&
                        is_pinned_host(arena + hi - 1);
      // Packed, an aliased payload goes up once: offsets that strictly increase
      // cannot repeat a payload (the common case, one pass); otherwise the
      // host's alias detection names each message's first.
      uint64_t packed = 0;
      bool increasing = true;
      for (uint64_t i = 0; i < n && !span; ++i) {
        packed += round16(len[i]);
        increasing = increasing && (i == 0 || off[i] > off[i - 1]);
      }
      std::vector<uint64_t> first;
      if (!span && !increasing) {
        std::vector<uint64_t> table, bucket;
        std::vector<uint32_t> tag;
        alias_uids(off, len, n, first, table, bucket, tag);
        packed = 0;
        for (uint64_t i = 0; i < n; ++i)
          if (first[i] == i) packed += round16(len[i]);
      }
      if (span || small_call(n, packed)) {
        const SmallSpan sp{arena, off, lo, hi};
        run_small(ctx, t0, n, len, out, [&](uint64_t i, uint8_t* dst) { std::memcpy(dst, arena + off[i], len[i]); },
                  span ? &sp : nullptr, first.empty() ? nullptr : first.data());
        ctx->stats.direct_calls += span;
        count();
        return;
      }
    }
    trace("validated", t0);
    // Zero-copy upload when the caller packed into pinned memory (msha_pinned_alloc)
    // with 16-byte aligned message starts and little waste between messages:
    // the touched byte ranges go up as they are and the GPU plans the lanes.
    // A pageable arena of the same shape takes the same path, its touched runs
    // copied through pinned staging slots (staged_calls; MSHA_STAGED_DIRECT=0:
    // the gather pipeline below instead).
    const bool dense = aligned16 && hi > lo && hi - lo <= std::min(sum, hi - lo) + 16 * n + (1u << 20);
    const bool pinned = dense && is_pinned_host(arena + lo) && is_pinned_host(arena + hi - 1);
    if (pinned || (dense && env_u64("MSHA_STAGED_DIRECT", 1) != 0)) {
      run_direct(ctx, t0, n, off, len, arena, out, sc, &early, !pinned);
      (pinned ? ctx->stats.direct_calls : ctx->stats.staged_calls)++;
      count();
      return;
    }
    // Overlapping payloads (sum of lengths > the span they cover) means there
    // may be aliases: give every message the index of the first message with
    // the same (off, len).
    const bool aliases = n > 1 && sum > hi - lo;
    if (aliases) alias_uids(off, len, n, ctx->uid, ctx->alias_table, ctx->alias_bucket, ctx->alias_tag);
    trace("aliases", t0);
    std::vector<uint64_t> bounds(ctx->devs.size() + 1);
    partition_pieces(len, n, (uint32_t)ctx->devs.size(), sc.csum, bounds.data());
    run_pipeline(ctx, t0, n, len, aliases ? ctx->uid.data() : nullptr, out,
                 [&](uint64_t i, uint8_t* dst) { std::memcpy(dst, arena + off[i], len[i]); }, bounds.data());
    count();
  });
}

int msha_hash_actions(msha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                      const uint64_t* part_off, const uint64_t* part_len, uint64_t n_parts,
                      const uint64_t* action_part_begin, uint64_t n_actions, uint8_t* out) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n_actions == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (!action_part_begin || !out || (n_parts && (!part_off || !part_len)) || (arena_len && !arena))
    return fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (action_part_begin[0] != 0 || action_part_begin[n_actions] != n_parts)
    return fail(ctx, MSHA_ERR_INVALID_ARG, "action_part_begin must start at 0 and end at n_parts");
  const double t0 = now_ms();
  return guarded(ctx, [&] {
    // One threaded pass (2^18 parts and up) after the cheap monotonicity check:
    // each thread validates the parts of its actions and sums their lengths
    // (h.Write appends, so an action's message is its parts back to back). The
    // error names the first bad part, as a serial scan would.
    const unsigned T = plan_threads(std::max(n_actions, n_parts));
    std::vector<uint64_t> bad(T, UINT64_MAX);
    parallel_chunks(n_actions, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
      for (uint64_t i = lo; i < hi; ++i)
        if (action_part_begin[i + 1] < action_part_begin[i]) {
          bad[t] = i;
          return;
        }
    });
    for (uint64_t b : bad)
      if (b != UINT64_MAX) throw MshaError(MSHA_ERR_INVALID_ARG, "action_part_begin must be non-decreasing");
    std::vector<uint64_t>& alen = ctx->tmp_len;
    alen.resize(n_actions);
    std::vector<uint64_t> packed_t(T, 0), bytes_t(T, 0), blocks_t(T, 0);
    parallel_chunks(n_actions, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
      uint64_t packed = 0, bytes = 0, blocks = 0;
      for (uint64_t i = lo; i < hi; ++i) {
        uint64_t l = 0;
        for (uint64_t j = action_part_begin[i]; j < action_part_begin[i + 1]; ++j) {
          if (part_len[j] > arena_len || part_off[j] > arena_len - part_len[j]) {
            bad[t] = j;
            return;
          }
          l += part_len[j];
        }
        alen[i] = l;
        packed += round16(l);
        bytes += l;
        blocks += blocks_for(l);
      }
      packed_t[t] = packed;
      bytes_t[t] = bytes;
      blocks_t[t] = blocks;
    });
    for (uint64_t b : bad)
      if (b != UINT64_MAX) throw MshaError(MSHA_ERR_INVALID_ARG, "part " + std::to_string(b) + " outside arena");
    uint64_t packed = 0, bytes = 0, blocks = 0;
    for (unsigned t = 0; t < T; ++t) {
      packed += packed_t[t];
      bytes += bytes_t[t];
      blocks += blocks_t[t];
    }
    auto gather = [&](uint64_t a, uint8_t* dst) {
      for (uint64_t j = action_part_begin[a]; j < action_part_begin[a + 1]; ++j) {
        std::memcpy(dst, arena + part_off[j], part_len[j]);
        dst += part_len[j];
      }
    };
    if (small_call(n_actions, packed))
      run_small(ctx, t0, n_actions, alen.data(), out, gather);
    else
      run_pipeline(ctx, t0, n_actions, alen.data(), nullptr, out, gather);
    ctx->stats.messages += n_actions;
    ctx->stats.message_bytes += bytes;
    ctx->stats.blocks += blocks;
  });
}

int msha_digest_of_digests(msha_ctx* ctx, const uint8_t* table, uint64_t n_table,
                           const uint32_t* idx, uint64_t n_idx, const uint64_t* begin, uint64_t n,
                           uint8_t* out) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (!begin || !out || (n_idx && !idx) || (n_table && !table))
    return fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (begin[0] != 0 || begin[n] != n_idx)
    return fail(ctx, MSHA_ERR_INVALID_ARG, "begin must start at 0 and end at n_idx");
  for (uint64_t i = 0; i < n; ++i)
    if (begin[i + 1] < begin[i]) return fail(ctx, MSHA_ERR_INVALID_ARG, "begin must be non-decreasing");
  return guarded(ctx, [&] {
    {  // threaded from 2^18 indices on
      const unsigned T = plan_threads(n_idx);
      std::vector<uint8_t> bad(T, 0);
      parallel_chunks(n_idx, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
        uint32_t worst = 0;
        for (uint64_t k = lo; k < hi; ++k) worst = std::max(worst, idx[k]);
        bad[t] = hi > lo && worst >= n_table;
      });
      for (uint8_t b : bad)
        if (b) throw MshaError(MSHA_ERR_INVALID_ARG, "idx out of table range");
    }
    std::vector<uint64_t>& alen = ctx->tmp_len;
    alen.resize(n);
    uint64_t packed = 0;
    for (uint64_t i = 0; i < n; ++i) {
      alen[i] = 32 * (begin[i + 1] - begin[i]);
      packed += alen[i];  // multiples of 32: already 16-aligned
    }
    if (small_call(n, packed) && packed <= kSmallDodBytes) {  // latency path: a Batch's digests = one message
      run_small(ctx, now_ms(), n, alen.data(), out, [&](uint64_t i, uint8_t* dst) {
        for (uint64_t k = begin[i]; k < begin[i + 1]; ++k, dst += 32) std::memcpy(dst, table + 32 * (uint64_t)idx[k], 32);
      });
      uint64_t blocks = 0;
      for (uint64_t i = 0; i < n; ++i) blocks += blocks_for(alen[i]);
      ctx->stats.messages += n;
      ctx->stats.message_bytes += 32 * n_idx;
      ctx->stats.blocks += blocks;
      return;
    }
    const uint32_t k = (uint32_t)ctx->devs.size();
    std::vector<uint64_t> bounds(k + 1);
    partition(alen.data(), n, k, bounds.data());
    double t0 = now_ms();
    for (uint32_t s = 0; s < k; ++s) {
      Device& d = ctx->devs[s];
      const uint64_t lo = bounds[s], hi = bounds[s + 1], m = hi - lo;
      d.lo = lo;
      d.hi = hi;
      d.st = msha_shard_stats{};
      d.st.device = d.id;
      d.st.messages = d.st.lanes = m;
      if (m == 0) continue;
      const uint64_t i0 = begin[lo], i1 = begin[hi];
      HIPCHK(hipSetDevice(d.id));
      d.table.ensure(32 * std::max<uint64_t>(n_table, 1));
      d.idx.ensure(4 * std::max<uint64_t>(i1 - i0, 1));
      d.begin.ensure(8 * (m + 1));
      d.out.ensure(32 * m);
      d.h_meta.ensure(8 * (m + 1));
      uint64_t* hb = d.h_meta.as<uint64_t>();
      for (uint64_t i = 0; i <= m; ++i) hb[i] = begin[lo + i] - i0;
      if (n_table) HIPCHK(hipMemcpyAsync(d.table.p, table, 32 * n_table, hipMemcpyHostToDevice, d.stream));
      if (i1 > i0) HIPCHK(hipMemcpyAsync(d.idx.p, idx + i0, 4 * (i1 - i0), hipMemcpyHostToDevice, d.stream));
      HIPCHK(hipMemcpyAsync(d.begin.p, hb, 8 * (m + 1), hipMemcpyHostToDevice, d.stream));
      d.err.ensure(4);
      HIPCHK(hipMemsetAsync(d.err.p, 0, 4, d.stream));
      HIPCHK(hipEventRecord(d.ev0, d.stream));
      d.st.h2d_payload_bytes = 32 * n_table;
      d.st.h2d_bytes = 32 * n_table + 4 * (i1 - i0) + 8 * (m + 1);
      msha::SplitPlan sp;
      msha::LaunchKind kind;
      HIPCHK(msha::launch_digest_of_digests(d.table.as<uint8_t>(), d.idx.as<uint32_t>(),
                                            d.begin.as<uint64_t>(), m, d.out.as<uint8_t>(),
                                            d.err.as<uint32_t>(), d.stream,
                                            split_for(d, m, ctx->kernel_policy, sp, msha::kMaxSegmentsDod),
                                            &kind));
      count_launch(ctx, &d, kind);
      HIPCHK(hipEventRecord(d.ev1, d.stream));
      d.h_out.ensure(32 * m + 4);
      HIPCHK(hipMemcpyAsync(d.h_out.p, d.out.p, 32 * m, hipMemcpyDeviceToHost, d.stream));
      HIPCHK(hipMemcpyAsync(d.h_out.as<uint8_t>() + 32 * m, d.err.p, 4, hipMemcpyDeviceToHost, d.stream));
      d.st.d2h_bytes = 32 * m + 4;
    }
    double kernel_ms = 0;
    uint64_t h2d = 0, d2h = 0;
    for (uint32_t s = 0; s < k; ++s) {
      Device& d = ctx->devs[s];
      const uint64_t m = d.hi - d.lo;
      if (m == 0) continue;
      HIPCHK(hipSetDevice(d.id));
      HIPCHK(hipStreamSynchronize(d.stream));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, d.ev0, d.ev1));
      d.st.device_ms = ms;
      kernel_ms = std::max<double>(kernel_ms, ms);
      uint32_t errflag;
      std::memcpy(&errflag, d.h_out.as<uint8_t>() + 32 * m, 4);
      if (errflag & 2) {
        // a split chain's handoff timed out (its digests are undefined): the
        // inputs are still on the device, re-hash the shard unsplit
        HIPCHK(hipMemsetAsync(d.err.p, 0, 4, d.stream));
        msha::LaunchKind kind;
        HIPCHK(msha::launch_digest_of_digests(d.table.as<uint8_t>(), d.idx.as<uint32_t>(),
                                              d.begin.as<uint64_t>(), m, d.out.as<uint8_t>(),
                                              d.err.as<uint32_t>(), d.stream, nullptr, &kind));
        count_launch(ctx, &d, kind);
        HIPCHK(hipMemcpyAsync(d.h_out.p, d.out.p, 32 * m, hipMemcpyDeviceToHost, d.stream));
        HIPCHK(hipStreamSynchronize(d.stream));
        d.st.d2h_bytes += 32 * m;
        ctx->stats.split_retries++;
      }
      std::memcpy(out + 32 * d.lo, d.h_out.p, 32 * m);
      h2d += d.st.h2d_bytes;
      d2h += d.st.d2h_bytes;
    }
    uint64_t blocks = 0;
    for (uint64_t i = 0; i < n; ++i) blocks += blocks_for(alen[i]);
    ctx->stats.calls++;
    ctx->stats.messages += n;
    ctx->stats.message_bytes += 32 * n_idx;
    ctx->stats.blocks += blocks;
    ctx->stats.plan_ms = 0;
    ctx->stats.pack_ms = 0;
    ctx->stats.device_ms = kernel_ms;
    ctx->stats.h2d_bytes = h2d;
    ctx->stats.d2h_bytes = d2h;
    ctx->stats.total_ms = now_ms() - t0;
  });
}

}  // extern "C"
