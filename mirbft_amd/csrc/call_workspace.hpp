// What the device entries of several launches share (msha_hash_actions_device_planned and
// _routed, msha_dstreams_write_jobs_device and _write_routed_device,
// msha_group_digests_device, msha_dmap_add_device): the workspace each
// of them owns, what the two parts entries keep in the context, and the arguments they
// read alike. Host-only.
//
// The workspace rule (DESIGN.md "The workspace of a device call"): one device allocation
// that grows only outside stream capture and never shrinks; a call outside capture is
// ordered after the owner's previous call, whatever stream that was on, by an event; a
// capture that would have to allocate is refused before anything is touched.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <random>
#include <string>

#include "host_call.hpp"
#include "parts_plan.hpp"
#include "workspace_rule.hpp"

#pragma GCC visibility push(hidden)  // the library's own helpers: libmirsha.so exports none of them
namespace msha {

class CallWorkspace {
 public:
  // The refusal of a call on a capturing stream that would have to allocate.
  [[noreturn]] static void refuse(const char* entry) {
    throw MshaError(MSHA_ERR_INVALID_ARG,
                    std::string(entry) + ": the workspace cannot grow while the stream is being captured: "
                                         "make one call of this size outside the capture first");
  }
  // On its own, for an entry that must refuse before something else of its (device_entry).
  void refuse_growth(const char* entry, uint64_t need, bool capturing) const {
    if (growth(need, bytes_, 0, capturing).refuse) refuse(entry);
  }
  // `need` bytes for a call on st: the base. Grows to need + spare where it must.
  uint8_t* acquire(const char* entry, uint64_t need, uint64_t spare, bool capturing, hipStream_t st) {
    const Growth g = growth(need, bytes_, spare, capturing);
    if (g.refuse) refuse(entry);
    if (g.grow) {
      // an earlier call may still be using the old buffer
      if (last_) HIPCHK(hipEventSynchronize(last_));
      if (p_) HIPCHK(hipFree(p_));
      p_ = nullptr;
      bytes_ = 0;
      ran_ = false;
      HIPCHK(hipMalloc(&p_, g.alloc));
      bytes_ = g.alloc;
    }
    if (!last_ && !capturing) HIPCHK(hipEventCreateWithFlags(&last_, hipEventDisableTiming));
    // two streams must not race on the workspace: after the previous call's last kernel
    if (!capturing && ran_) HIPCHK(hipStreamWaitEvent(st, last_, 0));
    return static_cast<uint8_t*>(p_);
  }
  // After the call's last launch on st.
  void commit(hipStream_t st, bool capturing) {
    ran_ = true;
    if (!capturing) HIPCHK(hipEventRecord(last_, st));
  }
  bool ran() const { return ran_; }  // some call has filled the workspace
  const uint8_t* data() const { return static_cast<const uint8_t*>(p_); }  // for the read-back diagnostics
  // With the owner's device current.
  void release() {
    if (last_) {
      (void)hipEventSynchronize(last_);
      (void)hipEventDestroy(last_);
    }
    if (p_) (void)hipFree(p_);
    *this = CallWorkspace();
  }

 private:
  void* p_ = nullptr;
  uint64_t bytes_ = 0;
  hipEvent_t last_ = nullptr;  // recorded after each call outside capture
  bool ran_ = false;
};

// What msha_hash_actions_device_planned (parts_plan.cpp) keeps in the context: its
// workspace, on the first device, and its counters. msha_ctx_destroy releases ws.
struct PartsPlanState {
  CallWorkspace ws;
  uint64_t last_lists = 0;  // n_lists of the last call (msha_parts_plan_read_order)
  msha_parts_plan_stats stats{};
};

// What msha_hash_actions_device_routed (parts_route.cpp) keeps in the context: a
// workspace of its own (a planned and a routed call share no memory), where the last
// call's arrays lie in it (msha_parts_route_read*) and its counters.
struct PartsRouteState {
  CallWorkspace ws;
  uint64_t last_lists = 0, last_slots = 0;  // n_lists and max_long of the last call
  uint64_t at_order = 0, at_chain = 0, at_out_idx = 0, at_claim = 0;  // byte offsets in ws of its arrays
  msha_parts_route_stats stats{};
};

// What msha_group_digests_device (group.cpp) keeps in the context: a workspace of its own
// (the table, the positions, the counts, the ids and the tile totals: group.hpp Layout),
// the seed of its hash, drawn when the context is created, and its counters.
// msha_ctx_destroy releases ws.
inline uint64_t draw_seed() {
  try {
    std::random_device rd;
    return (uint64_t)rd() << 32 ^ (uint64_t)rd();
  } catch (...) {  // no entropy source: the clock still differs from run to run
    return (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() * 0x9E3779B97F4A7C15ull;
  }
}
struct GroupState {
  CallWorkspace ws;
  uint64_t seed = draw_seed();
  msha_group_stats stats{};
};

// MSHA_PARTS_PLAN_WAVE_SUM (A/B runs, read at each call), or parts_plan::kWaveSumParts.
inline uint32_t wave_sum_parts() {
  const int t = env_int("MSHA_PARTS_PLAN_WAVE_SUM", (int)parts_plan::kWaveSumParts);
  return t < 1 ? 1u : (uint32_t)t;
}

// msha_route_opts checked and defaulted (opts null: every default). noun: what a slot
// holds, "list" or "row". cus: the device's compute units, or 0 while the device is not
// known: an entry checks the long_bytes bounds with its other arguments, and calls again
// inside guard() for the max_long bound and its default -- the slots are lanes of the
// eight-lane chain, one workgroup a CU.
inline msha_route_opts route_opts(const char* entry, const char* noun, const msha_route_opts* opts, int cus,
                                  uint32_t default_long_blocks) {
  msha_route_opts o = opts ? *opts : msha_route_opts{0, 0, 0};
  const auto bad = [&](const std::string& what) { return MshaError(MSHA_ERR_INVALID_ARG, std::string(entry) + ": " + what); };
  if (o.long_bytes != 0 && o.long_bytes < 16 + MSHA_DEVICE_ARENA_SLACK)
    throw bad("opts->long_bytes (" + std::to_string(o.long_bytes) + ") holds no " + noun +
              ": it must be 0 or at least " + std::to_string(16 + MSHA_DEVICE_ARENA_SLACK));
  if (o.long_bytes > (1ull << 48)) throw bad("opts->long_bytes (" + std::to_string(o.long_bytes) + ") is above 2^48");
  const uint64_t most = (uint64_t)cus * kChain8MsgsPerWg;
  if (cus && o.max_long > most)
    throw bad("opts->max_long (" + std::to_string(o.max_long) + ") is above 16 x compute units (" +
              std::to_string(most) + ")");
  if (!o.long_blocks) o.long_blocks = default_long_blocks;
  if (!o.max_long) o.max_long = (uint32_t)most;
  if (!o.long_bytes) o.long_bytes = MSHA_ROUTE_LONG_BYTES_DEFAULT;
  return o;
}

// The planned kernels' arguments from a parts entry's and a layout placed in the workspace at ws.
inline PartsPlanArgs plan_args(const uint8_t* d_arena, const uint64_t* d_part_off, const uint64_t* d_part_len,
                               const uint64_t* d_list_part_begin, uint64_t n_lists, const uint32_t* d_action_list,
                               uint64_t n_actions, uint8_t* d_out, uint32_t* err, uint8_t* ws,
                               const parts_plan::Layout& lay) {
  PartsPlanArgs a;
  a.arena = d_arena;
  a.part_off = d_part_off;
  a.part_len = d_part_len;
  a.begin = d_list_part_begin;
  a.n_lists = n_lists;
  a.action_list = d_action_list;
  a.n_actions = n_actions;
  a.info = reinterpret_cast<uint32_t*>(ws);
  a.cnt = a.info + 16;
  a.order = reinterpret_cast<uint32_t*>(ws + lay.order);
  a.key16 = reinterpret_cast<uint16_t*>(ws + lay.key16);
  a.used = d_action_list ? ws + lay.used : nullptr;
  a.table = d_action_list ? ws + lay.table : nullptr;
  a.out = d_out;
  a.err = err;
  a.wave_sum_parts = wave_sum_parts();
  return a;
}

// msha_parts_plan_read_order and msha_parts_route_read_order, with the lock held: the
// lane count of the entry's last call (over last_lists lists) and the order its planner
// left at at_order in ws, once the device has finished.
inline int read_plan_order(msha_ctx* ctx, const CallWorkspace& ws, uint64_t last_lists, uint64_t at_order,
                           uint32_t* order, uint64_t cap, uint64_t* lanes) {
  *lanes = 0;
  if (!ws.ran()) return MSHA_OK;
  return guard(ctx, [&] {
    (void)ctx_first_device(ctx);
    HIPCHK(hipDeviceSynchronize());
    uint32_t n = 0;
    HIPCHK(hipMemcpy(&n, ws.data(), 4, hipMemcpyDeviceToHost));
    if (n > last_lists) n = (uint32_t)last_lists;  // the order holds last_lists positions
    *lanes = n;
    const uint64_t k = n < cap ? n : cap;
    if (k) HIPCHK(hipMemcpy(order, ws.data() + at_order, 4 * k, hipMemcpyDeviceToHost));
  });
}

}  // namespace msha
#pragma GCC visibility pop
