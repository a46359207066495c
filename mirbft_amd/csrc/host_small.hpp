// The latency path of the host entries: run_small and its zero-copy variant. Templates
// over the per-message copy (each host entry passes its own, inlined into the packing
// loop); included by host_entries.cpp. small_stats is in host_small.cpp; the limits that
// choose this path are in host_plan.hpp.
#pragma once
#include <atomic>

#include "ctx.hpp"

namespace msha {

// ---------------------------------------------------------------------------
// Small calls: the latency path. MirBFT's hash worker hands over one
// ActionList per call (mirbft.go:282-302), and at low load that is a handful of
// actions. run_pipeline's round trip costs ~60-80 us whatever the size (seven
// queue operations over two streams, events, planning passes), while the GPU
// floor of H2D + kernel + D2H is ~18 us (tools/op_latency.hip). A call of at
// most small_msgs() messages and small_bytes() of payload (limits below)
// therefore runs on the context's first GPU as: messages packed behind their
// metadata in one pinned staging buffer -> ONE H2D (a pinned, 16-byte aligned
// arena span over 512 KiB is uploaded as is instead: metadata H2D + span H2D),
// one launch, ONE D2H of [error word | digests]. No alias folding (an identical
// payload is simply hashed again) and no sharding: neither pays at this size.
// ---------------------------------------------------------------------------

// Stats of a latency-path call (run_small, run_small_zc).
void small_stats(msha_ctx* ctx, Device& d, double t0, double t_pack, double t_dev, uint64_t m, uint64_t pay,
                 uint64_t h2d, uint64_t d2h, bool packed, msha::LaunchKind kind);

// The zero-copy latency path (see run_small): [off | len | payload] packed into
// coherent pinned memory, read in place by the kernel, digests written in place.
template <class Fill>
void run_small_zc(msha_ctx* ctx, Device& d, double t0, uint64_t m, uint64_t meta, uint64_t pay, const uint64_t* len,
                  uint8_t* out, Fill& fill, const uint64_t* first) {
  d.sm_zc_in.ensure(meta + pay + msha::kArenaSlack);
  d.sm_zc_out.ensure(32 * m);
  uint64_t* h_off = d.sm_zc_in.as<uint64_t>();
  uint64_t* h_len = h_off + m;
  uint8_t* h_pay = d.sm_zc_in.as<uint8_t>() + meta;
  uint64_t a = 0;
  for (uint64_t i = 0; i < m; ++i) {
    h_len[i] = len[i];
    if (first && first[i] != i) {
      h_off[i] = h_off[first[i]];
    } else {
      h_off[i] = a;
      if (len[i]) fill(i, h_pay + a);
      a += round16(len[i]);
    }
  }
  const double t_pack = now_ms();
  HIPCHK(hipSetDevice(d.id));
  const uint64_t out_cap = d.sm_out.cap;
  d.sm_out.ensure(32);  // the device error word (never set here: the packer's offsets are aligned)
  if (d.sm_out.cap != out_cap) HIPCHK(hipMemsetAsync(d.sm_out.p, 0, 32, d.stream));
  void *dev_in = nullptr, *dev_out = nullptr;
  HIPCHK(hipHostGetDevicePointer(&dev_in, d.sm_zc_in.p, 0));
  HIPCHK(hipHostGetDevicePointer(&dev_out, d.sm_zc_out.p, 0));
  const uint64_t* d_off = static_cast<const uint64_t*>(dev_in);
  // Completion by polling the digests themselves (MSHA_SMALL_ZC_POLL=0: a stream
  // synchronize, A/B): every 8-byte word starts as a sentinel, and the kernel
  // overwrites each with its final value in one PCIe write (16-byte digest halves).
  // A word that still reads as the sentinel is waited for until hipStreamQuery
  // reports the launch done -- so a digest word that happens to equal the
  // sentinel (2^-64 a word) only costs the wait, never a wrong digest -- and a
  // failed launch is reported from there.
  const bool poll = env_u64("MSHA_SMALL_ZC_POLL", 1) != 0;
  constexpr uint64_t kSentinel = 0xC3A55A3C96E1F00Full;
  volatile uint64_t* words = static_cast<volatile uint64_t*>(d.sm_zc_out.p);
  if (poll)
    for (uint64_t k = 0; k < 4 * m; ++k) words[k] = kSentinel;
  msha::LaunchKind kind;
  HIPCHK(msha::launch_digest_batch(static_cast<const uint8_t*>(dev_in) + meta, d_off, d_off + m, nullptr, nullptr, m,
                                   static_cast<uint8_t*>(dev_out), d.sm_out.as<uint32_t>(), d.cus, MSHA_KERNEL_AUTO,
                                   d.stream, nullptr, &kind));
  if (poll) {
    uint64_t k = 0;
    for (uint64_t spin = 1; k < 4 * m; ++spin) {
      while (k < 4 * m && words[k] != kSentinel) ++k;
      if (k == 4 * m || spin % 64) {
        __builtin_ia32_pause();
        continue;
      }
      const hipError_t q = hipStreamQuery(d.stream);
      if (q == hipSuccess) break;  // done: every word is final, whatever it reads
      if (q != hipErrorNotReady) HIPCHK(q);
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  } else {
    HIPCHK(hipStreamSynchronize(d.stream));
  }
  const double t_dev = now_ms();
  std::memcpy(out, d.sm_zc_out.p, 32 * m);
  ctx->stats.small_zc_calls++;
  small_stats(ctx, d, t0, t_pack, t_dev, m, pay, 0, 0, true, kind);
}

// The caller's pinned arena, uploaded as is: messages i at base + off[i], all
// inside [lo, hi), 16-byte aligned.
struct SmallSpan {
  const uint8_t* base;
  const uint64_t* off;
  uint64_t lo, hi;
};

// first (may be null): first[i] = the earliest message with message i's (off,
// len) (alias_uids): an aliased payload is packed once and its aliases point at
// it (EpochChange re-hashes, epoch_target.go:486-505; the Go adapter shares a
// payload between actions, gpuhash.go epochChangeAliases).
//
// Zero-copy (round 6): a call of at most small_zc_msgs()
// messages and small_zc_bytes() packed (a few actions: MirBFT's hash worker at low
// load) skips both copies. The list is packed into coherent pinned memory that the
// kernel (the eight-lane chain: at most 16 messages a CU) reads in place over PCIe,
// and the digests are written straight into coherent pinned memory: one launch and
// one synchronize per call. The packer's own 16-byte aligned offsets cannot raise
// the device error word (check_aligned), so it stays on the device.
// Limits measured per call (tools/latency.cpp, profiles/r06_latency/): 512-B
// requests zero-copy / copying, 1: 29.6 / 38.1 us, 64: 31.7 / 42.0, 256: 33.9 /
// 46.8, 1,024: 47.9 / 70.5, 4,096: 108.1 / 111.2 (the kernel's PCIe reads then cost
// what the copy saved).
inline uint64_t small_zc_bytes() { return env_u64("MSHA_SMALL_ZC_BYTES", 1ull << 20); }  // 0 disables
inline uint64_t small_zc_msgs(const Device& d) { return std::min<uint64_t>(env_u64("MSHA_SMALL_ZC_MSGS", 2048),
                                                                    (uint64_t)d.cus * msha::kChain8MsgsPerWg); }

template <class Fill>
void run_small(msha_ctx* ctx, double t0, uint64_t m, const uint64_t* len, uint8_t* out, Fill&& fill,
               const SmallSpan* span = nullptr, const uint64_t* first = nullptr) {
  Device& d = ctx->devs[0];
  const uint64_t meta = (16 * m + 63) & ~uint64_t(63);  // off[m], len[m]; payload 64-B aligned after
  uint64_t pay = 0;
  if (span) {
    pay = span->hi - span->lo;
  } else {
    for (uint64_t i = 0; i < m; ++i)
      if (!first || first[i] == i) pay += round16(len[i]);
  }
  const bool zc = !span && ctx->kernel_policy == MSHA_KERNEL_AUTO && m <= small_zc_msgs(d) &&
                  meta + pay <= small_zc_bytes();
  if (zc) return run_small_zc(ctx, d, t0, m, meta, pay, len, out, fill, first);
  d.sm_stage.ensure(meta + (span ? 0 : pay));
  uint64_t* h_off = d.sm_stage.as<uint64_t>();
  uint64_t* h_len = h_off + m;
  uint8_t* h_pay = d.sm_stage.as<uint8_t>() + meta;
  uint64_t a = 0;
  for (uint64_t i = 0; i < m; ++i) {
    h_len[i] = len[i];
    if (span) {
      h_off[i] = span->off[i] - span->lo;
    } else if (first && first[i] != i) {
      h_off[i] = h_off[first[i]];
    } else {
      h_off[i] = a;
      if (len[i]) fill(i, h_pay + a);
      a += round16(len[i]);
    }
  }
  const double t_pack = now_ms();
  HIPCHK(hipSetDevice(d.id));
  d.sm_in.ensure(meta + pay + msha::kArenaSlack);
  const uint64_t out_cap = d.sm_out.cap;
  d.sm_out.ensure(32 + 32 * m);
  // the error word heads the output buffer; zeroed once per allocation and
  // again only after a call that found it set
  if (d.sm_out.cap != out_cap) HIPCHK(hipMemsetAsync(d.sm_out.p, 0, 32, d.stream));
  d.sm_res.ensure(32 + 32 * m);
  uint8_t* dev_in = d.sm_in.as<uint8_t>();
  if (span) {
    HIPCHK(hipMemcpyAsync(dev_in, h_off, 16 * m, hipMemcpyHostToDevice, d.stream));
    if (pay) HIPCHK(hipMemcpyAsync(dev_in + meta, span->base + span->lo, pay, hipMemcpyHostToDevice, d.stream));
  } else {
    HIPCHK(hipMemcpyAsync(dev_in, h_off, meta + pay, hipMemcpyHostToDevice, d.stream));
  }
  msha::LaunchKind kind;
  HIPCHK(msha::launch_digest_batch(dev_in + meta, reinterpret_cast<const uint64_t*>(dev_in),
                                   reinterpret_cast<const uint64_t*>(dev_in) + m, nullptr, nullptr, m,
                                   d.sm_out.as<uint8_t>() + 32, d.sm_out.as<uint32_t>(), d.cus,
                                   ctx->kernel_policy, d.stream, nullptr, &kind));
  HIPCHK(hipMemcpyAsync(d.sm_res.p, d.sm_out.p, 32 + 32 * m, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  const double t_dev = now_ms();
  uint32_t errflag;
  std::memcpy(&errflag, d.sm_res.p, 4);
  if (errflag) {  // cannot happen (aligned payloads, no split chains): leave the word clean, report
    HIPCHK(hipMemsetAsync(d.sm_out.p, 0, 32, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    throw MshaError(MSHA_ERR_HIP, "internal: device error flag " + std::to_string(errflag) + " on a small call");
  }
  std::memcpy(out, d.sm_res.as<uint8_t>() + 32, 32 * m);
  const uint64_t h2d = 16 * m + (span ? pay : meta - 16 * m + pay);
  small_stats(ctx, d, t0, t_pack, t_dev, m, pay, h2d, 32 + 32 * m, !span, kind);
}

}  // namespace msha
