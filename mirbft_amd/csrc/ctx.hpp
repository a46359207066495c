// The context (msha_ctx) and its per-GPU state, as libmirsha's own units see them, with the
// helpers more than one path uses. Internal: ctx.cpp defines the non-template helpers,
// creates and destroys the context and answers ctx_access.hpp; the host paths
// (host_small, host_pipeline, host_direct), their entries (host_entries.cpp) and the
// raw-pointer batch entries (device_batch.cpp) include this. The other device entries
// see only ctx_access.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <exception>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mirsha.h"
#include "kernels.hpp"
#include "ctx_access.hpp"
#include "host_call.hpp"
#include "call_workspace.hpp"
#include "host_plan.hpp"

namespace msha {

// Growable device buffer (never shrinks; reallocation only between calls).
struct DevBuf {
  void* p = nullptr;
  uint64_t cap = 0;
  void ensure(uint64_t bytes) {
    if (bytes <= cap) return;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    cap = 0;
    uint64_t want = std::max<uint64_t>(bytes + bytes / 4, 4096);
    HIPCHK(hipMalloc(&p, want));
    cap = want;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// Growable pinned host buffer.
struct PinBuf {
  void* p = nullptr;
  uint64_t cap = 0;
  // hipHostMallocCoherent: the GPU reads and writes it over PCIe uncached (the
  // latency path's zero-copy buffers, which kernels access in place)
  unsigned flags = hipHostMallocPortable;
  void ensure(uint64_t bytes) {
    if (bytes <= cap) return;
    if (p) HIPCHK(hipHostFree(p));
    p = nullptr;
    cap = 0;
    uint64_t want = std::max<uint64_t>(bytes + bytes / 4, 4096);
    HIPCHK(hipHostMalloc(&p, want, flags));
    cap = want;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// Per-GPU state: stream, timing events, device buffers, pinned staging.
struct Device {
  int id = 0;
  uint32_t index = 0;  // shard number in the context
  int numa = -1;       // NUMA node of the GPU's PCI device (-1: unknown)
  int cus = 256;
  hipStream_t stream = nullptr;       // kernels (and everything on single-stream paths)
  hipStream_t copy_stream = nullptr;  // H2D of staged chunks, overlapping the kernels
  hipStream_t d2h_stream = nullptr;   // host calls: digests back, behind their kernels (ev_k);
                                      // only on a GPU no other shard shares (d2h_stream_after)
  hipEvent_t ev_k = nullptr;          // the latest hash launch of a host call
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // device_ms / upload_ms / kernel_ms of the last host call: first H2D (copy
  // stream) .. last H2D, first hash kernel .. last kernel (msha_shard_stats)
  hipEvent_t ev_up0 = nullptr, ev_up1 = nullptr, ev_k0 = nullptr;
  hipEvent_t ev_meta = nullptr, ev_plan = nullptr;  // direct path: metadata landed / GPU plan done
  hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;      // direct path: the planner kernels (plan_kernel_ms)
  hipEvent_t slot_free[2] = {nullptr, nullptr};  // staging slot s may be refilled
  hipEvent_t chunk_in = nullptr;                 // last chunk's bytes are on the device
  std::vector<hipEvent_t> span_ev;               // direct mode: upload piece c is on the device
  DevBuf arena, off, len, order, out, err, idx, begin, table;
  // pinned staging, allocated with this GPU current (the runtime's pool for its NUMA node)
  PinBuf h_arena, h_meta, h_out, slot[2];
  // small-call path (run_small): [meta | payload] in, [error word | digests] out
  DevBuf sm_in, sm_out;
  PinBuf sm_stage, sm_res;
  // zero-copy latency path: [meta | payload] and the digests in coherent pinned
  // memory the kernel reads and writes in place (no H2D, no D2H)
  PinBuf sm_zc_in{nullptr, 0, hipHostMallocPortable | hipHostMallocCoherent};
  PinBuf sm_zc_out{nullptr, 0, hipHostMallocPortable | hipHostMallocCoherent};
  // direct path, planned on the GPU (plan.hip): raw metadata, granule map,
  // device offsets, alias table and slots, representatives, bucket counters,
  // [gmin | cut | info] read back to h_small; rep read back to h_rep
  DevBuf p_meta, p_gmap, p_devoff, p_table, p_slot, p_rep, p_cnt, p_small;
  PinBuf h_gmap, h_small, h_rep;
  // planned device calls (msha_digest_batch_device_planned): alias table,
  // representatives, bucket counters, lane order, [lanes | head]; the head of
  // long chains runs on side_stream, forked from and joined to the caller's
  DevBuf f_table, f_rep, f_cnt, f_order, f_key, f_tkeys, f_longs;
  hipStream_t head_stream = nullptr;  // a folded call's early head (FoldArgs::longs)
  hipEvent_t ev_longs = nullptr, ev_join2 = nullptr;
  uint32_t f_epoch = 0;  // the alias table's epoch tag of the last folded call (plan.hip fold_claim)
  // What msha_planned_read_plan needs of the last planned call (n 0: none yet): the rest
  // it reads from f_cnt (info; gave_up_at: the look-back's give-up count, in bytes),
  // f_order and f_longs.
  struct LastPlanned {
    uint64_t n = 0, gave_up_at = 0;
    bool fold = false, early = false;
    uint32_t long_cap = 0, head_cap = 0, head_per_wg = 0;
  } f_last;
  DevBuf probe;  // msha_clock_probe: stamps + sink
  // direct path heads (launch_head): their digests, lane-indexed; read back with
  // their lanes' digest slots into h_head ([digests | slots])
  DevBuf p_head;
  PinBuf h_head;
  hipEvent_t ev_head = nullptr;  // the latest head launch (side stream)
  bool head_side = false;        // this call's heads went on side_stream
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_fplan = nullptr, ev_join = nullptr, ev_fdone = nullptr;
  bool fdone_recorded = false;  // ev_fdone: the last planned call's work is queued behind it
  // per-call shard description
  uint64_t lo = 0, hi = 0;        // message/action range
  uint64_t arena_bytes = 0;       // staged arena size (without slack)
  std::vector<uint8_t> direct_mark;  // direct path: granules of the arena this shard touches
  msha_shard_stats st{};          // last host call (msha_get_shard_stats)
  // Multi-GPU host calls: this GPU's share of the host threads (its shard is
  // planned, and its pageable chunks gathered, on them) and planning scratch.
  std::unique_ptr<WorkerPool> gather_pool;
  std::vector<uint32_t> sort_tmp;
  std::vector<uint64_t> tmp_dev;
  // split chaining (kernels.hip): kSplitRing flag arrays of cus*2 entries,
  // allocated once and zeroed, never reallocated (launches may be in flight)
  uint64_t* split_flags = nullptr;
  uint64_t split_epoch = 0;
  void release() {
    gather_pool.reset();
    for (DevBuf* b : {&arena, &off, &len, &order, &out, &err, &idx, &begin, &table, &sm_in, &sm_out, &p_meta,
                      &p_gmap, &p_devoff, &p_table, &p_slot, &p_rep, &p_cnt, &p_small, &f_table, &f_rep,
                      &f_cnt, &f_order, &f_key, &f_tkeys, &f_longs, &probe, &p_head})
      b->release();
    if (split_flags) (void)hipFree(split_flags);
    split_flags = nullptr;
    for (PinBuf* b : {&h_arena, &h_meta, &h_out, &slot[0], &slot[1], &sm_stage, &sm_res, &sm_zc_in, &sm_zc_out, &h_gmap, &h_small, &h_rep,
                      &h_head})
      b->release();
    for (hipEvent_t* e : {&ev0, &ev1, &ev_up0, &ev_up1, &ev_k0, &ev_meta, &ev_plan, &ev_p0, &ev_p1, &slot_free[0],
                          &slot_free[1], &chunk_in, &ev_fork, &ev_fplan, &ev_join, &ev_fdone, &ev_head,
                          &ev_longs, &ev_join2}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
    for (hipEvent_t e : span_ev) (void)hipEventDestroy(e);
    span_ev.clear();
    if (stream) (void)hipStreamDestroy(stream);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (d2h_stream) (void)hipStreamDestroy(d2h_stream);
    if (side_stream) (void)hipStreamDestroy(side_stream);
    if (head_stream) (void)hipStreamDestroy(head_stream);
    if (ev_k) (void)hipEventDestroy(ev_k);
    ev_k = nullptr;
    stream = copy_stream = d2h_stream = side_stream = head_stream = nullptr;
  }
};

// Per-GPU plan of one host-memory call (kept in the context: its vectors are
// reused call after call, so planning does not page-fault fresh memory).
struct Plan {
  uint64_t m = 0;
  bool ordered = false;
  std::vector<uint32_t> perm;       // sorted lane -> shard-local message (pageable path)
  std::vector<uint64_t> lane_cut;   // group boundaries in sorted lanes
  size_t next = 0;                  // next group to issue
  uint64_t launched = 0;            // lanes [0, launched) have a kernel enqueued
  uint64_t lanes = 0;               // messages that get a lane (one per distinct payload)
  std::vector<uint32_t> rep;        // shard-local message -> its lane's message (empty: identity)
  const uint32_t* rep_dev = nullptr;  // direct path: the same, planned on the GPU (pinned copy)
  std::vector<uint64_t> cut_chunk;  // direct mode: upload piece lane group g waits for
  // direct mode: later_min[g] = the lowest message any lane of groups >= g
  // writes (later_min[groups] = m), so once groups < g are hashed the digest
  // slots below later_min[g] are final; d2h_done = slots already D2H'd
  std::vector<uint64_t> later_min;
  uint64_t d2h_done = 0;
  // direct mode: lanes [0, head) are long chains run as heads (launch_head),
  // their digests lane-indexed in Device::p_head, placed by finish_shard
  uint64_t head = 0;
  bool k0 = false;  // the shard's first kernel is queued (Device::ev_k0 recorded)
  bool identity() const { return !ordered && rep.empty(); }  // lane q hashes message q
  const uint32_t* rep_of() const { return rep_dev ? rep_dev : (rep.empty() ? nullptr : rep.data()); }
};

}  // namespace msha

struct msha_ctx {
  // Calls on one context are serialised here (a second caller waits), so a
  // context may be shared between threads; distinct contexts run concurrently.
  mutable std::mutex mu;
  std::vector<msha::Device> devs;
  char err[512] = "";  // last failure on the context (fixed buffer: msha_last_error's pointer stays valid)
  msha_stats stats{};
  msha_parts_stats parts_stats{};  // msha_hash_actions_device (msha_get_parts_stats)
  msha::PartsPlanState parts_plan;  // msha_hash_actions_device_planned (parts_plan.cpp)
  msha_concat_stats concat_stats{};  // msha_concat_lists_device (parts_concat.cpp)
  msha_verify_stats verify_stats{};  // msha_verify_digests_device (verify.cpp)
  msha::PartsRouteState parts_route;  // msha_hash_actions_device_routed (parts_route.cpp)
  msha::GroupState group;  // msha_group_digests_device (group.cpp)
  // allocations handed out by msha_pinned_alloc: (pointer, mapped bytes), 0 =
  // hipHostMalloc, else an mmap striped over NUMA nodes and hipHostRegister'ed
  std::vector<std::pair<void*, uint64_t>> pinned;
  std::vector<uint64_t> tmp_len;
  int kernel_policy = MSHA_KERNEL_AUTO;
  // host planning buffers reused across calls
  std::vector<msha::Plan> plans;
  std::vector<uint64_t> uid;
  std::vector<uint64_t> alias_table, alias_bucket;
  std::vector<uint32_t> alias_tag;
  // Several physical GPUs: the whole-batch planning phases (validation, alias
  // detection, upload marking) run on a pool of the context's full host-thread
  // share (host_threads_total) instead of the process-wide 16; made on first use.
  std::unique_ptr<msha::WorkerPool> wide;
};

namespace msha {

// Sets the context's error text and returns code.
int fail(msha_ctx* ctx, int code, const std::string& msg);

// The physical GPUs under the context's shards (virtual shards share one): what
// host_threads_total (host_plan.hpp) counts 16 host threads for.
inline unsigned distinct_gpus(const msha_ctx* ctx) {
  std::vector<int> ids;
  for (const Device& d : ctx->devs)
    if (std::find(ids.begin(), ids.end(), d.id) == ids.end()) ids.push_back(d.id);
  return (unsigned)ids.size();
}

// A call on the context: msha::guard() (host_call.hpp) with the context's wide pool
// installed for the call's whole-batch phases.
template <class F>
int guarded(msha_ctx* ctx, F&& f) {
  return msha::guard(ctx, [&] {
    std::unique_ptr<WorkerPool> none;  // no context: nothing to install
    PoolScope scope(ctx ? ctx->wide : none, ctx ? distinct_gpus(ctx) : 0);
    f();
  });
}

// Count a kernel launch in the context's counters (atomically: the pageable
// multi-GPU path launches from one thread per GPU) and in the shard's.
void count_launch(msha_ctx* ctx, Device* d, msha::LaunchKind kind);

// Runs f(s) for every shard s of the context: inline for one shard; for
// several, one thread per shard, each with its GPU's share of the host threads
// as its planning pool (tl_pool), so per-GPU work (upload queueing, lane
// planning, pageable gathers) proceeds side by side. Rethrows the first error.
template <class F>
void for_each_shard(msha_ctx* ctx, F&& f) {
  const uint32_t k = (uint32_t)ctx->devs.size();
  if (k == 1) {
    f(0u);
    return;
  }
  const unsigned per = std::max(1u, host_threads_total(distinct_gpus(ctx)) / k);
  for (Device& d : ctx->devs)
    if (!d.gather_pool || d.gather_pool->size() != per) d.gather_pool.reset(new WorkerPool(per - 1));
  std::vector<std::exception_ptr> errs(k);
  std::vector<std::thread> th;
  for (uint32_t s = 0; s < k; ++s)
    th.emplace_back([&, s] {
      tl_pool = ctx->devs[s].gather_pool.get();
      try {
        f(s);
      } catch (...) {
        errs[s] = std::current_exception();
      }
      tl_pool = nullptr;
    });
  for (auto& t : th) t.join();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
}

// Device entry points: the context's first device, its error word zeroed once.
void device_prologue(msha_ctx* ctx, void* stream, hipStream_t* st);

// d's split-chaining flag ring, zeroed (made by msha_ctx_create), and the split plan of an
// n-message launch on d (nullptr: plain launch): ctx.cpp.
void ensure_split_flags(Device& d);
const msha::SplitPlan* split_for(Device& d, uint64_t n, int policy, msha::SplitPlan& sp,
                                 int cap = msha::kMaxSegmentsArena);

// Is p inside page-locked host memory the GPU can DMA from (hipHostMalloc /
// hipHostRegister)? Pageable memory makes the query fail; clear that error.
bool is_pinned_host(const void* p);

// MSHA_TRACE=1: host-side phase timestamps (ms since the call began) on stderr.
inline bool trace_on() {
  static const bool on = getenv("MSHA_TRACE") != nullptr;
  return on;
}
inline void trace(const char* what, double t0) {
  if (trace_on()) fprintf(stderr, "[msha] %-24s %9.2f ms\n", what, now_ms() - t0);
}
// the same, for one shard's thread of a multi-shard call
inline void trace(const char* what, uint32_t shard, double t0) {
  if (trace_on()) fprintf(stderr, "[msha] shard %u %-16s %9.2f ms\n", shard, what, now_ms() - t0);
}

}  // namespace msha
