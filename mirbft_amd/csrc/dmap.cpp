// Device digest maps: the host half of msha_dmap_* (include/mirsha.h "Device digest
// maps"; dmap.hip, dmap.hpp). A map owns one device allocation on the context's first
// device, made in create (dmap.hpp Store: head, table, key store, counts), and a per-call
// workspace (dmap.hpp CallLayout) that is a CallWorkspace and follows the workspace rule
// stated in call_workspace.hpp. Add is seven launches on the caller's stream, find and
// clear one each, with nothing else enqueued and no host wait. The host checks what it can
// see; everything the kernels find is in the caller's arrays, and the device error word is
// not used. Size and read are synchronous.
//
// A vote map (msha_dmap_create_voters; dmap_vote.hip, dmap_vote.hpp) is the same object
// with a mask of voters behind each key in the same allocation (VoteStore) and a larger
// workspace (VoteLayout): msha_dmap_vote_device is ten launches, _find_votes_device one,
// through the same scaffold, counted in a struct of their own.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <new>
#include <string>

#include "../../include/mirsha.h"
#include "call_workspace.hpp"
#include "dmap.hpp"
#include "dmap_vote.hpp"

static_assert(sizeof(msha_dmap_result) == 8 * sizeof(uint64_t), "k_dmap_fill writes the result as eight words");
static_assert(sizeof(msha_dmap_vote_result) == msha::dmap_vote::kResultWords * sizeof(uint64_t),
              "k_vote_fill writes the result as eleven words");

struct msha_dmap {
  msha_ctx* ctx = nullptr;
  msha::CtxDevice dev;
  uint64_t max_keys = 0;
  uint32_t max_voters = 0;   // 0: a plain map; else a vote map of that many voters
  uint8_t* store = nullptr;  // dmap.hpp Store; of a vote map dmap_vote.hpp VoteStore
  msha::CallWorkspace ws;    // dmap.hpp CallLayout, of the adds; of a vote map VoteLayout, of the votes
  // of both hashes, drawn at create for the reason GroupState::seed is: the digests come
  // off the wire, and with a fixed function a sender could aim every key at one chain
  uint64_t seed = msha::draw_seed();
  msha_dmap_stats st{};
  msha_dmap_vote_stats vst{};
};

namespace {

namespace dm = msha::dmap;
namespace dv = msha::dmap_vote;

// env_int for a 64-bit value (decimal, or hex with 0x), read at each call.
bool env_u64(const char* name, uint64_t* v) {
  const char* e = getenv(name);
  if (!e || !*e) return false;
  *v = std::strtoull(e, nullptr, 0);
  return true;
}

void release(msha_dmap* m) {
  (void)hipSetDevice(m->dev.id);
  m->ws.release();
  if (m->store) (void)hipFree(m->store);
  m->store = nullptr;
}

// The map's fields of the kernels' arguments. MSHA_DMAP_SEED and MSHA_DMAP_FORCE_HOME
// (diagnostics, tests/test_gpu_dmap.py): another seed, and one home position for every
// key in the map's table. No output depends on either, as long as it keeps one value
// between two clears (a key is looked for where the value in force would have put it).
msha::DmapArgs map_args(const msha_dmap* m) {
  const dm::Store lay(m->max_keys);
  msha::DmapArgs a;
  a.head = reinterpret_cast<uint64_t*>(m->store + lay.head);
  a.table = reinterpret_cast<uint32_t*>(m->store + lay.table);
  a.key_scope = reinterpret_cast<uint32_t*>(m->store + lay.scope);
  a.key_digests = m->store + lay.digests;
  a.count = reinterpret_cast<uint32_t*>(m->store + lay.count);
  a.capacity = lay.cap;
  a.max_keys = m->max_keys;
  if (m->max_voters) {
    const dv::VoteStore v(m->max_keys, m->max_voters);
    a.masks = reinterpret_cast<uint32_t*>(m->store + v.mask);
    a.mask_quads = (v.bytes - v.mask) / 16;
  }
  a.seed = m->seed;
  (void)env_u64("MSHA_DMAP_SEED", &a.seed);
  uint64_t at = 0;
  if (env_u64("MSHA_DMAP_FORCE_HOME", &at)) {
    a.force_home = 1;
    a.force_at = (uint32_t)(at % lay.cap);
  }
  return a;
}

// The call's own slots grouped: the arguments of group.hip's first three kernels on the
// call's table, in a workspace laid out by lay at ws.
msha::GroupArgs group_args(const msha_dmap* m, uint8_t* ws, const dm::CallLayout& lay, const uint8_t* d_digests, uint64_t n,
                           const uint32_t* d_scope) {
  const auto u32 = [&](uint64_t at) { return reinterpret_cast<uint32_t*>(ws + at); };
  msha::GroupArgs g;
  g.digests = d_digests;
  g.n = n;
  g.scope = d_scope;
  g.first = u32(lay.first);
  g.head = reinterpret_cast<uint64_t*>(ws + lay.g.head);
  g.table = u32(lay.g.table);
  g.pos = u32(lay.g.pos);
  g.count = u32(lay.g.count);
  g.id = u32(lay.g.id);
  g.totals = u32(lay.g.totals);
  g.capacity = lay.g.cap;
  // MSHA_GROUP_SEED and MSHA_GROUP_FORCE_HOME act on the call's table, as in group.cpp
  g.seed = m->seed;
  (void)env_u64("MSHA_GROUP_SEED", &g.seed);
  uint64_t at = 0;
  if (env_u64("MSHA_GROUP_FORCE_HOME", &at)) {
    g.force_home = 1;
    g.force_at = (uint32_t)(at % lay.g.cap);
  }
  return g;
}

// The workspace's fields of an add's or a vote's arguments.
void call_args(msha::DmapArgs* a, const msha::GroupArgs& g, uint8_t* ws, const dm::CallLayout& lay) {
  const auto u32 = [&](uint64_t at) { return reinterpret_cast<uint32_t*>(ws + at); };
  a->first = g.first;
  a->members = g.count;
  a->lead_id = g.id;
  a->lead_pos = u32(lay.ppos);
  a->lead_before = u32(lay.before);
  a->tot_new = u32(lay.tot_new);
  a->tot_cross = u32(lay.tot_cross);
  a->best = g.head + msha::group::kHeadBest;
}

// The key arguments add and find share. Call with the lock held.
int check_keys(msha_dmap* m, const char* entry, const uint8_t* d_digests, uint64_t n) {
  if (n > dm::kMaxSlots) return msha::bad_arg(m->ctx, entry, "n must be at most 2^30");
  if (reinterpret_cast<uintptr_t>(d_digests) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(m->ctx, entry, "d_digests must be 16-byte aligned");
  return MSHA_OK;
}

// find and clear: one launch on the caller's stream and nothing else (but what
// MSHA_PARTS_TIMING=1 adds). Call with the lock held.
template <class Launch>
int one_launch(msha_dmap* m, const char* entry, void* stream, const char* what, uint64_t* counter, uint64_t digests,
               Launch&& launch) {
  return msha::guard(m->ctx, [&] {
    msha::CtxDevice d;  // the map's own (m->dev): the context's first device
    const hipStream_t st = msha::device_entry(m->ctx, entry, stream, &d);
    msha::LaunchTimer timer(st);
    msha::launch_check(launch(st), what);
    const float ms = timer.stop();
    (*counter)++;
    m->st.digests += digests;
    m->st.launches++;
    m->st.last_kernel_ms = ms;
  });
}

// Both kinds of map, max_voters 0 the plain one. Call with the lock held.
int create(msha_ctx* ctx, const char* entry, uint64_t max_keys, uint32_t max_voters, msha_dmap** out) {
  if (max_keys == 0 || max_keys > dm::kMaxKeys) return msha::bad_arg(ctx, entry, "a device digest map holds 1 .. 2^30 keys");
  msha_dmap* m = new (std::nothrow) msha_dmap;
  if (!m) return msha::ctx_fail(ctx, MSHA_ERR_OUT_OF_MEMORY, "host allocation failed");
  m->ctx = ctx;
  m->max_keys = max_keys;
  m->max_voters = max_voters;
  const dm::Store lay(max_keys);
  m->st.capacity = lay.cap;
  m->vst.max_voters = max_voters;
  m->vst.mask_words = max_voters ? dv::words(max_voters) : 0;
  const uint64_t bytes = max_voters ? dv::VoteStore(max_keys, max_voters).bytes : lay.bytes;
  const int rc = msha::guard(ctx, [&] {
    m->dev = msha::ctx_first_device(ctx);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&m->store), bytes));
    msha::launch_check(msha::launch_dmap_clear(map_args(m), m->dev.stream), "k_dmap_clear launch");
    HIPCHK(hipStreamSynchronize(m->dev.stream));
  });
  if (rc != MSHA_OK) {
    release(m);
    delete m;
    return rc;
  }
  *out = m;
  return MSHA_OK;
}

// An entry called on the other kind of map. Call with the lock held.
int wrong_kind(msha_dmap* m, const char* entry) {
  return msha::bad_arg(m->ctx, entry,
                       m->max_voters ? "this is a vote map (msha_dmap_create_voters): its count is its voters, use "
                                       "msha_dmap_vote_device"
                                     : "this map keeps no voters: create it with msha_dmap_create_voters");
}

}  // namespace

extern "C" {

int msha_dmap_create(msha_ctx* ctx, uint64_t max_keys, msha_dmap** out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  return create(ctx, "msha_dmap_create", max_keys, 0, out);
}

int msha_dmap_create_voters(msha_ctx* ctx, uint64_t max_keys, uint32_t max_voters, msha_dmap** out) {
  static const char* const kEntry = "msha_dmap_create_voters";
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (max_voters == 0 || max_voters > dv::kMaxVoters) return msha::bad_arg(ctx, kEntry, "a vote map takes 1 .. 1024 voters");
  return create(ctx, kEntry, max_keys, max_voters, out);
}

void msha_dmap_destroy(msha_dmap* m) {
  if (!m) return;
  {
    std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
    release(m);
  }
  delete m;
}

int msha_dmap_add_device(msha_dmap* m, const uint8_t* d_digests, uint64_t n, const uint32_t* d_scope,
                         uint32_t threshold, uint32_t* d_id, uint32_t* d_before, uint32_t* d_after,
                         uint32_t* d_crossed_slot, uint64_t crossed_cap, msha_dmap_result* d_result, void* stream) {
  static const char* const kEntry = "msha_dmap_add_device";
  if (!m) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  if (n == 0) return MSHA_OK;
  if (m->max_voters) return wrong_kind(m, kEntry);
  const int rc = check_keys(m, kEntry, d_digests, n);
  if (rc != MSHA_OK) return rc;
  if (!d_digests || !d_id || !d_result) return msha::bad_arg(m->ctx, kEntry, "null pointer argument");
  if (crossed_cap > 0 && !d_crossed_slot) return msha::bad_arg(m->ctx, kEntry, "d_crossed_slot is null with crossed_cap > 0");

  return msha::guard(m->ctx, [&] {
    // a capturing stream allows no allocation: know that before the context's first
    // device call would make one (the error word) or the workspace would grow
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    const dm::CallLayout lay(n);
    if (capturing && !msha::ctx_first_device_ready(m->ctx)) msha::CallWorkspace::refuse(kEntry);
    m->ws.refuse_growth(kEntry, lay.bytes, capturing);
    msha::CtxDevice d;  // the map's own (m->dev): the context's first device
    const hipStream_t st = msha::device_entry(m->ctx, kEntry, stream, capturing, &d);

    uint8_t* ws = m->ws.acquire(kEntry, lay.bytes, lay.bytes / 4, capturing, st);
    const msha::GroupArgs g = group_args(m, ws, lay, d_digests, n, d_scope);
    msha::DmapArgs a = map_args(m);
    a.digests = d_digests;
    a.n = n;
    a.scope = d_scope;
    a.threshold = threshold;
    a.id = d_id;
    a.before = d_before;
    a.after = d_after;
    a.crossed_slot = d_crossed_slot;
    a.crossed_cap = crossed_cap;
    a.result = reinterpret_cast<uint64_t*>(d_result);
    call_args(&a, g, ws, lay);

    // MSHA_DMAP_STOP_AFTER=k, k in 1 .. 5 (diagnostic, tools/dmap_bench.py): the first k
    // kernels alone, so that each one's share can be timed; the outputs are then
    // incomplete and the map is as it was, since nothing before commit writes to it. Commit
    // never runs without fill (the keys would be in, `entries` not), so any other value
    // is the whole call.
    const int stop = msha::env_int("MSHA_DMAP_STOP_AFTER", 0);
    const uint32_t kernels = stop >= 1 && stop <= 5 ? (uint32_t)stop : dm::kLaunches;

    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    msha::launch_check(msha::launch_group_init(g, st), "k_group_init launch");
    if (kernels > 1) msha::launch_check(msha::launch_group_insert(g, st), "k_group_insert launch");
    if (kernels > 2) msha::launch_check(msha::launch_group_resolve(g, st), "k_group_resolve launch");
    if (kernels > 3) msha::launch_check(msha::launch_dmap_find(a, st), "k_dmap_find launch");
    if (kernels > 4) msha::launch_check(msha::launch_dmap_scan(a, st), "k_dmap_scan launch");
    if (kernels > 5) {
      msha::launch_check(msha::launch_dmap_commit(a, st), "k_dmap_commit launch");
      msha::launch_check(msha::launch_dmap_fill(a, st), "k_dmap_fill launch");
    }
    m->ws.commit(st, capturing);
    const float ms = timer.stop();

    m->st.adds++;
    m->st.digests += n;
    m->st.launches += kernels;
    m->st.last_kernel_ms = ms;
  });
}

int msha_dmap_find_device(msha_dmap* m, const uint8_t* d_digests, uint64_t n, const uint32_t* d_scope, uint32_t* d_id,
                          uint32_t* d_count, void* stream) {
  static const char* const kEntry = "msha_dmap_find_device";
  if (!m) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  if (n == 0) return MSHA_OK;
  const int rc = check_keys(m, kEntry, d_digests, n);
  if (rc != MSHA_OK) return rc;
  if (!d_digests || !d_id) return msha::bad_arg(m->ctx, kEntry, "null pointer argument");
  msha::DmapArgs a = map_args(m);
  a.digests = d_digests;
  a.n = n;
  a.scope = d_scope;
  a.id = d_id;
  a.after = d_count;
  return one_launch(m, kEntry, stream, "k_dmap_lookup launch", &m->st.finds, n,
                    [&](hipStream_t st) { return msha::launch_dmap_lookup(a, st); });
}

int msha_dmap_clear_device(msha_dmap* m, void* stream) {
  if (!m) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  const msha::DmapArgs a = map_args(m);
  return one_launch(m, "msha_dmap_clear_device", stream, "k_dmap_clear launch", &m->st.clears, 0,
                    [&](hipStream_t st) { return msha::launch_dmap_clear(a, st); });
}

int msha_dmap_size(msha_dmap* m, uint64_t* entries) {
  if (!m || !entries) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  return msha::guard(m->ctx, [&] {
    HIPCHK(hipSetDevice(m->dev.id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(entries, m->store + dm::Store(m->max_keys).head + 8 * dm::kHeadEntries, 8, hipMemcpyDeviceToHost));
  });
}

int msha_dmap_read(msha_dmap* m, uint64_t first_id, uint64_t k, uint32_t* scope_out, uint8_t* digests_out,
                   uint32_t* count_out) {
  static const char* const kEntry = "msha_dmap_read";
  if (!m) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  return msha::guard(m->ctx, [&] {
    const dm::Store lay(m->max_keys);
    HIPCHK(hipSetDevice(m->dev.id));
    HIPCHK(hipDeviceSynchronize());
    uint64_t entries = 0;
    HIPCHK(hipMemcpy(&entries, m->store + lay.head + 8 * dm::kHeadEntries, 8, hipMemcpyDeviceToHost));
    if (first_id > entries || k > entries - first_id)
      throw msha::MshaError(MSHA_ERR_INVALID_ARG, std::string(kEntry) + ": ids " + std::to_string(first_id) + " .. " +
                                                      std::to_string(first_id) + " + " + std::to_string(k) +
                                                      " reach past the map's " + std::to_string(entries) + " entries");
    if (k == 0) return;
    if (scope_out) HIPCHK(hipMemcpy(scope_out, m->store + lay.scope + 4 * first_id, 4 * k, hipMemcpyDeviceToHost));
    if (digests_out)
      HIPCHK(hipMemcpy(digests_out, m->store + lay.digests + 32 * first_id, 32 * k, hipMemcpyDeviceToHost));
    if (count_out) HIPCHK(hipMemcpy(count_out, m->store + lay.count + 4 * first_id, 4 * k, hipMemcpyDeviceToHost));
  });
}

int msha_dmap_vote_device(msha_dmap* m, const uint8_t* d_digests, uint64_t n, const uint32_t* d_scope,
                          const uint32_t* d_voter, uint32_t threshold, uint32_t* d_id, uint32_t* d_counted,
                          uint32_t* d_before, uint32_t* d_after, uint32_t* d_crossed_slot, uint64_t crossed_cap,
                          msha_dmap_vote_result* d_result, void* stream) {
  static const char* const kEntry = "msha_dmap_vote_device";
  if (!m) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  if (n == 0) return MSHA_OK;
  if (!m->max_voters) return wrong_kind(m, kEntry);
  const int rc = check_keys(m, kEntry, d_digests, n);
  if (rc != MSHA_OK) return rc;
  if (!d_digests || !d_voter || !d_id || !d_result) return msha::bad_arg(m->ctx, kEntry, "null pointer argument");
  if (crossed_cap > 0 && !d_crossed_slot) return msha::bad_arg(m->ctx, kEntry, "d_crossed_slot is null with crossed_cap > 0");

  return msha::guard(m->ctx, [&] {
    // as in add: a capturing stream allows no allocation
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    const dv::VoteLayout lay(n);
    if (capturing && !msha::ctx_first_device_ready(m->ctx)) msha::CallWorkspace::refuse(kEntry);
    m->ws.refuse_growth(kEntry, lay.bytes, capturing);
    msha::CtxDevice d;  // the map's own (m->dev): the context's first device
    const hipStream_t st = msha::device_entry(m->ctx, kEntry, stream, capturing, &d);

    uint8_t* ws = m->ws.acquire(kEntry, lay.bytes, lay.bytes / 4, capturing, st);
    const auto u32 = [&](uint64_t at) { return reinterpret_cast<uint32_t*>(ws + at); };
    const msha::GroupArgs g = group_args(m, ws, lay.c, d_digests, n, d_scope);
    msha::DmapVoteArgs a;
    static_cast<msha::DmapArgs&>(a) = map_args(m);
    a.digests = d_digests;
    a.n = n;
    a.scope = d_scope;
    a.threshold = threshold;
    a.id = d_id;
    a.before = d_before;
    a.after = d_after;
    a.crossed_slot = d_crossed_slot;
    a.crossed_cap = crossed_cap;
    a.result = reinterpret_cast<uint64_t*>(d_result);
    call_args(&a, g, ws, lay.c);
    a.voter = d_voter;
    a.counted_out = d_counted;
    a.max_voters = m->max_voters;
    a.mask_words = dv::words(m->max_voters);
    a.pair_table = u32(lay.pair_table);
    a.pair_pos = u32(lay.pair_pos);
    a.counted = u32(lay.counted);
    a.fresh = u32(lay.fresh);
    a.tot_counted = u32(lay.tot_counted);
    a.tot_repeats = u32(lay.tot_repeats);
    a.tot_bad = u32(lay.tot_bad);
    a.vhead = reinterpret_cast<uint64_t*>(ws + lay.head);
    a.pair_capacity = lay.pair_cap;
    // the pair table is the call's, as group's: the same seed places both
    a.pair_seed = g.seed;
    uint64_t at = 0;
    if (env_u64("MSHA_DMAP_PAIR_FORCE_HOME", &at)) {
      a.pair_force_home = 1;
      a.pair_force_at = (uint32_t)(at % lay.pair_cap);
    }

    // MSHA_DMAP_VOTE_STOP_AFTER=k, k in 1 .. 8 (diagnostic, tools/dmap_vote_bench.py): the
    // first k kernels alone, as MSHA_DMAP_STOP_AFTER does for an add. Nothing before commit
    // writes to the map, and commit never runs without fill.
    const int stop = msha::env_int("MSHA_DMAP_VOTE_STOP_AFTER", 0);
    const uint32_t kernels = stop >= 1 && stop <= 8 ? (uint32_t)stop : dv::kLaunches;

    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    msha::launch_check(msha::launch_group_init(g, st), "k_group_init launch");
    if (kernels > 1) msha::launch_check(msha::launch_group_insert(g, st), "k_group_insert launch");
    if (kernels > 2) msha::launch_check(msha::launch_group_resolve(g, st), "k_group_resolve launch");
    if (kernels > 3) msha::launch_check(msha::launch_vote_find(a, st), "k_vote_find launch");
    if (kernels > 4) msha::launch_check(msha::launch_vote_pair(a, st), "k_vote_pair launch");
    if (kernels > 5) msha::launch_check(msha::launch_vote_count(a, st), "k_vote_count launch");
    if (kernels > 6) msha::launch_check(msha::launch_vote_totals(a, st), "k_vote_totals launch");
    if (kernels > 7) msha::launch_check(msha::launch_vote_scan(a, st), "k_vote_scan launch");
    if (kernels > 8) {
      msha::launch_check(msha::launch_vote_commit(a, st), "k_vote_commit launch");
      msha::launch_check(msha::launch_vote_fill(a, st), "k_vote_fill launch");
    }
    m->ws.commit(st, capturing);
    const float ms = timer.stop();

    m->vst.votes++;
    m->vst.slots += n;
    m->vst.launches += kernels;
    m->vst.last_kernel_ms = ms;
  });
}

int msha_dmap_find_votes_device(msha_dmap* m, const uint8_t* d_digests, uint64_t n, const uint32_t* d_scope,
                                const uint32_t* d_voter, uint32_t* d_id, uint32_t* d_count, uint32_t* d_voted,
                                void* stream) {
  static const char* const kEntry = "msha_dmap_find_votes_device";
  if (!m) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  if (n == 0) return MSHA_OK;
  if (!m->max_voters) return wrong_kind(m, kEntry);
  const int rc = check_keys(m, kEntry, d_digests, n);
  if (rc != MSHA_OK) return rc;
  if (!d_digests || !d_voter || !d_id || !d_voted) return msha::bad_arg(m->ctx, kEntry, "null pointer argument");
  msha::DmapVoteArgs a;
  static_cast<msha::DmapArgs&>(a) = map_args(m);
  a.digests = d_digests;
  a.n = n;
  a.scope = d_scope;
  a.id = d_id;
  a.after = d_count;
  a.voter = d_voter;
  a.counted_out = d_voted;
  a.max_voters = m->max_voters;
  a.mask_words = dv::words(m->max_voters);
  return msha::guard(m->ctx, [&] {
    msha::CtxDevice d;  // the map's own (m->dev): the context's first device
    const hipStream_t st = msha::device_entry(m->ctx, kEntry, stream, &d);
    msha::LaunchTimer timer(st);
    msha::launch_check(msha::launch_vote_lookup(a, st), "k_vote_lookup launch");
    const float ms = timer.stop();
    m->vst.vote_finds++;
    m->vst.slots += n;
    m->vst.launches++;
    m->vst.last_kernel_ms = ms;
  });
}

int msha_dmap_read_voters(msha_dmap* m, uint64_t first_id, uint64_t k, uint32_t* masks_out) {
  static const char* const kEntry = "msha_dmap_read_voters";
  if (!m) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  if (!m->max_voters) return wrong_kind(m, kEntry);
  return msha::guard(m->ctx, [&] {
    const dv::VoteStore lay(m->max_keys, m->max_voters);
    HIPCHK(hipSetDevice(m->dev.id));
    HIPCHK(hipDeviceSynchronize());
    uint64_t entries = 0;
    HIPCHK(hipMemcpy(&entries, m->store + lay.head + 8 * dm::kHeadEntries, 8, hipMemcpyDeviceToHost));
    if (first_id > entries || k > entries - first_id)
      throw msha::MshaError(MSHA_ERR_INVALID_ARG, std::string(kEntry) + ": ids " + std::to_string(first_id) + " .. " +
                                                      std::to_string(first_id) + " + " + std::to_string(k) +
                                                      " reach past the map's " + std::to_string(entries) + " entries");
    if (k == 0 || !masks_out) return;
    HIPCHK(hipMemcpy(masks_out, m->store + lay.mask + 4 * lay.mask_words * first_id, 4 * lay.mask_words * k,
                     hipMemcpyDeviceToHost));
  });
}

int msha_dmap_get_vote_stats(const msha_dmap* m, msha_dmap_vote_stats* out) {
  if (!m || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  *out = m->vst;
  return MSHA_OK;
}

int msha_dmap_get_stats(const msha_dmap* m, msha_dmap_stats* out) {
  if (!m || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(m->ctx));
  *out = m->st;
  return MSHA_OK;
}

}  // extern "C"
