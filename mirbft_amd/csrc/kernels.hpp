// Host-side launchers for the gfx950 SHA-256 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace msha {

// Bytes that must be readable after the last message of a device arena: the
// kernels read a message's final block as one whole 64-byte block.
constexpr uint64_t kArenaSlack = 64;

// How a lane brings its message blocks in from HBM (all modes are bit-identical):
//  kSingle   load block b at the top of iteration b; latency hidden by the
//            other waves of the SIMD (high occupancy)
//  kPrefetch load block b+1 while block b is compressed (16 more live VGPRs):
//            for few, long messages, where there are too few waves to hide it
//  kPair     at even b load blocks b and b+1 together: both halves of a
//            128-byte line are requested back to back, so the line is read
//            from HBM once instead of being evicted and re-fetched between
//            the two half-line requests (lane stride >= 128 B is the norm)
// (Rejected after A/B, profiles/r01_ab_modes, r01_ab_nt: an LDS-DMA prefetch
// mode, 6 % slower on c2, and nontemporal payload loads, 5-10 % slower.)
enum LoadMode { kSingle = 0, kPrefetch = 1, kPair = 2, kPipe = 3 };

// Fewer than ~3 waves per SIMD cannot hide HBM latency by occupancy: use the
// register-prefetching variant then; otherwise pair loads. At one wave per
// SIMD or less the pipelined kernel (kPipe, k_digest_batch_pipe) gives the lone
// wave independent work: c4 2.78 -> 2.64 ms; at 1.5, 2 and 3 waves per SIMD it
// ties or loses (profiles/r01_ab_pipe/). For A/B measurements MSHA_LOAD_MODE
// (0/1/2/3) forces the load mode.
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline int pick_mode(uint64_t n, int cus) {
  static const int forced = env_int("MSHA_LOAD_MODE", -1);
  if (forced >= kSingle && forced <= kPipe) return forced;
  if (n <= (uint64_t)cus * 4 * 64) return kPipe;
  return n < (uint64_t)cus * 4 * 64 * 3 ? kPrefetch : kPair;
}

// Lane i hashes message m = order ? order[i] : i (arena + off[m], len[m]) into
// digest slot o = out_idx ? out_idx[i] : m (out + 32 o). The device API passes
// order (message-indexed metadata); the host pipeline passes lane-indexed
// metadata and out_idx. policy: MSHA_KERNEL_AUTO / _LANE / _COOP (mirsha.h).
//
// split (may be null): run the launch as split chaining (kernels.hip), planned
// by plan_split(); the caller fills flags/epoch (see SplitPlan).
struct SplitPlan {
  uint64_t n_main = 0;      // messages [0, n_main) run one lane each, to completion
  uint32_t chains = 0;      // surplus waves: messages [n_main, n) in chains of 64
  uint32_t segments = 0;    // segments per chain
  uint32_t groups = 0;      // segment workgroups per segment (4 chains each, padded)
  uint32_t stall_chain = 0xFFFFFFFFu;  // failure-path test only (MSHA_SPLIT_STALL=1):
                                       // this chain's first segment never hands over
  uint64_t epoch = 0;       // unique (mod 2^24) among the launches that share flags
  uint64_t* flags = nullptr;  // device, >= chains entries, one word per chain:
                              // epoch | segments done | progress beat (kernels.hip)
};
// Segment caps of split chaining: arena messages / digest-of-digests (kernels.hip).
constexpr int kMaxSegmentsArena = 12;
constexpr int kMaxSegmentsDod = 12;
bool plan_split(uint64_t n, int cus, int policy, SplitPlan* sp, int cap);

// Which kernel a launcher ran (msha_stats launch counters; tests assert them).
// kLaunchChain2 / kLaunchChain8 count as cooperative launches too (launches_coop).
// kLaunchLaneWs (the work-stealing lane kernel) counts as a lane launch too.
enum LaunchKind { kLaunchNone = 0, kLaunchLane, kLaunchPipe, kLaunchCoop, kLaunchSplit, kLaunchDod,
                  kLaunchChain2, kLaunchChain8, kLaunchLaneWs };

// GPU-planned device launches (plan.hip: msha_digest_batch_device_planned). The
// planner's lane order holds kNoLane at positions it leaves unused (folded
// aliases, at the end), and *head (device memory, known only on the GPU) lanes
// at the front are long chains routed to the cooperative kernel. A gated launch
// over the whole order either is that head (head_part: cooperative, lanes at or
// past *head idle) or the rest (lanes below *head idle); neither splits.
constexpr uint32_t kNoLane = 0xFFFFFFFFu;
constexpr uint32_t kWsSlots = 64, kWsStride = 16;  // work-stealing tile counters, 64 B apart
// The planner's two-level grid reductions (plan.hip grid_reduce_last): 16 group
// slots and a top slot, 64 B each, zeroed words
constexpr uint32_t kGridGroups = 16, kGridWords = (kGridGroups + 1) * 16;
struct LaneGate {
  const uint32_t* head = nullptr;
  bool head_part = false;
  bool two_lane = false;  // head_part: k_digest_chain2 instead of the cooperative kernel
  bool eight_lane = false;  // head_part: k_digest_chain8 (eight lanes a message, 24 a CU)
  // the body (not head_part): kWsSlots x kWsStride zeroed device words -> the
  // work-stealing lane kernel (k_digest_batch_ws), with `lanes` (device, may be
  // null) the positions worth visiting
  uint32_t* ws_ctr = nullptr;
  const uint32_t* lanes = nullptr;
};

hipError_t launch_digest_batch(const uint8_t* arena, const uint64_t* off, const uint64_t* len,
                               const uint32_t* order, const uint32_t* out_idx, uint64_t n,
                               uint8_t* out, uint32_t* err, int cus, int policy, hipStream_t st,
                               const SplitPlan* split = nullptr, LaunchKind* kind = nullptr,
                               const LaneGate* gate = nullptr);
// Does launch_digest_batch use cooperative chaining for an n-message launch?
bool uses_coop(uint64_t n, int cus, int policy);
// Messages per workgroup of the cooperative kernel (one workgroup per CU) and
// of the two-lane head chain (k_digest_chain2).
constexpr unsigned kCoopMsgsPerWg = 128;
constexpr unsigned kChain2MsgsPerWg = 64;
constexpr unsigned kChain8MsgsPerWg = 16;
hipError_t launch_digest_uniform(const uint8_t* arena, uint64_t stride, uint64_t msg_len,
                                 uint64_t n, uint8_t* out, uint32_t* err, int cus,
                                 hipStream_t st, LaunchKind* kind = nullptr);
// err: device error word (bit 2: a split-chaining handoff timed out).
hipError_t launch_digest_of_digests(const uint8_t* table, const uint32_t* idx,
                                    const uint64_t* begin, uint64_t n, uint8_t* out,
                                    uint32_t* err, hipStream_t st,
                                    const SplitPlan* split = nullptr, LaunchKind* kind = nullptr);

// Direct (pinned-arena) host calls upload a shard's byte ranges in device-space
// pieces of 2^kDirectChunkShift bytes (64 MiB), one event each.
constexpr unsigned kDirectChunkShift = 26;

// Device-side planning of one shard of a direct host call (plan.hip). Every
// array is device memory of the shard's GPU; m messages, shard-local indices.
struct PlanArgs {
  const uint64_t* off;    // caller offsets (raw, as passed to msha_digest_batch)
  const uint64_t* len;
  const uint64_t* gmap;   // uploaded granule g (caller offset glo + g << gshift) -> device
                          // offset, indexed g - gbase
  uint64_t glo = 0, gbase = 0;
  uint32_t gshift = 16;
  uint64_t m = 0;
  uint64_t* dev_off;      // out: device offset of each message
  uint32_t* table;        // alias table, tmask + 1 zeroed entries; null: no aliases
  uint64_t tmask = 0;
  uint32_t* slot;         // m: each message's table slot (with table)
  uint32_t* rep;          // out, m: the first message with the same (off, len)
  uint64_t pieces = 1;    // upload pieces of the shard
  uint32_t piece_shift = kDirectChunkShift;  // a piece is 2^piece_shift device bytes
  // Lane groups: one per (region, piece), region 0 = long chains (blocks >=
  // long_blocks; long_blocks 0: no such region), region 1 = the rest; group
  // g = region * pieces + piece, chunks = the number of groups.
  uint64_t long_blocks = 0;
  uint64_t chunks = 1;
  uint64_t B = 1;         // block-count classes per group (1: groups only)
  uint64_t bmax = 0;      // largest block count (key = group * B + bmax - blocks)
  uint64_t nb = 1;        // chunks * B buckets
  uint32_t* cnt;          // nb zeroed counters -> bucket starts
  uint32_t* gmin;         // chunks entries, 0xFFFFFFFF-filled: lowest lane index per group
  uint32_t* cut;          // out, chunks + 1: first lane of each group
  uint32_t* info;         // out: [0] = lanes
  uint64_t* lane_off;     // out, per lane: device offset, length, digest slot
  uint64_t* lane_len;
  uint32_t* lane_slot;
};
hipError_t launch_plan(const PlanArgs& a, hipStream_t st);

// The planner kernels' tiling: 256 threads, kPlanItems messages each. The host sizes
// the per-tile scratch (apairs / acount, tkeys / tkcount, tstat) from it.
constexpr uint32_t kPlanItems = 16;
constexpr uint32_t kPlanTile = 256 * kPlanItems;

// Device-side planning of a device-resident batch (plan.hip,
// msha_digest_batch_device_planned): every array is device memory of one GPU.
// Lanes = messages, or with a table only the first of each (off, len) key
// (aliases fold into it); the order lists lanes by descending block count,
// kNoLane past the last; info[1] = the head of lanes whose chains would outlast
// the lane kernel's throughput time, for the cooperative kernel (at most
// head_cap). Block-count buckets: exact below 4,096 blocks, powers of two above.
// Classes, ascending: a message shorter than kFoldExactLen bytes by its exact
// length (a wave of one length hashes its padding block's schedule on the
// scalar unit, kernels.hip compress_uniform_pad), then exact block counts in
// [kFoldLowBlocks, 4096), then powers of two. Keys are descending classes.
constexpr uint32_t kFoldExactLen = 1024;
constexpr uint32_t kFoldLowBlocks = 16;   // (blocks of kFoldExactLen bytes: 17; 16 keeps the count even)
constexpr uint32_t kFoldBigBuckets = 52;  // the power-of-two classes (>= 4,096 blocks): keys [0, 52)
constexpr uint32_t kFoldBuckets = kFoldExactLen + (4096 - kFoldLowBlocks) + kFoldBigBuckets;
static_assert(kFoldBuckets % 2 == 0, "FoldArgs::big follows the counters 8-byte aligned");
struct FoldArgs {
  const uint64_t* off;
  const uint64_t* len;
  uint64_t n = 0;
  uint64_t* table = nullptr;  // tmask + 1 slots (epoch << 32 | message + 1); null: no folding
  uint64_t tmask = 0;
  uint32_t epoch = 1;         // this call's tag: a slot of another epoch is empty (never 0)
  // (with table) the folded messages, per tile of 4,096: apairs[tile * 4096 + k] =
  // rep << 32 | i for k < acount[tile] -- message i's digest is message rep's
  uint64_t* apairs = nullptr;
  uint32_t* acount = nullptr;
  // (with table) the insert finds the largest offset before its tile itself, by a
  // decoupled look-back over ceil(n / 4096) zeroed status words (plan.hip
  // tile_lookback); then one more zeroed word: look-backs that gave up waiting
  // (0 expected; see tile_lookback)
  uint64_t* tstat = nullptr;
  // 2 x kGridWords zeroed words: k_fold_longs' then k_fold_longs_gate's grid reduction
  uint32_t* grid_ws = nullptr;
  uint32_t* cnt;              // kFoldBuckets zeroed counters (by key) -> bucket starts
  uint64_t* big = nullptr;    // 2 x kFoldBigBuckets zeroed: per power-of-two key, the largest
                              // block count and the block sum (the head's cost model needs the
                              // real longest chain, not the class's lower bound)
  uint32_t* order;            // n, kNoLane-filled -> position -> message index
  uint16_t* key16 = nullptr;  // n: message i's key when it is a lane, else 0xFFFF (written by the
                              // insert or the counts, read by the scatter instead of len and rep)
  // Per tile of 4,096 messages, the keys its lanes hold and the tile's offset in
  // each key's bucket, taken when the insert (or the counts) added its lanes to
  // the bucket counters: tkeys[tile * 4096 + k] = key << 32 | offset for k <
  // tkcount[tile]. The scatter places lanes at bucket start + offset + rank with
  // no global atomics of its own.
  uint64_t* tkeys = nullptr;
  uint32_t* tkcount = nullptr;
  uint32_t* info;             // [0] lanes, [1] positions the lane kernel skips (the head's),
                              // [2] distinct long payloads, [3] unused,
                              // [4] the early head's lanes (0: none), [5] the late head's,
                              // [6] the first decision (0: no early head), by
                              // k_fold_longs_gate, [7..15] unused (the list's and the
                              // gate's sums: grid_ws),
                              // [16] lanes of >= long_blocks blocks, [17] the scan's cut (the
                              // scatter resolves [1] and [5] from them and [4])
                              // (all 32 words zeroed by the caller)
  // The early head (folding only; long_blocks 0: off), on a stream of its own
  // forked right after the planner's memsets: k_fold_longs_gate, a pass over len
  // alone, sizes the batch (info[6]: 0 when the short messages alone outlast the
  // longest chain); unless it stood down there, k_fold_longs claims every message
  // of >= long_blocks blocks in the alias table beside the insert, listing each
  // distinct one in longs; when there are at most long_cap, and their chain
  // outlasts the lane kernel's share, they are the head (info[4]), launched right
  // then over longs instead of after the scan and scatter, and k_fold_insert never
  // takes a long message as fresh (so its representative is the listed one).
  uint32_t* longs = nullptr;
  // off and len both 16-byte aligned: the per-thread runs of 16 messages load as
  // 16-byte vectors (plan.hip load_run)
  uint32_t vec = 0;
  uint32_t long_blocks = 0;
  uint32_t long_cap = 0;
  uint32_t head_cap = 0;      // 0: no head
  uint32_t simds = 1024;
  // The head: the cut of the longest lanes that minimises the launch's
  // estimated end (plan.hip head_cost), in SIMD cycles per block, measured (c5
  // slices, rocprofv3 timelines, profiles/r03_planned/): the lane kernel's
  // throughput on a storm's mixed lanes ~6,500 per wave-block (uniform batches:
  // 5,700); a long chain on the lane kernel among loaded SIMDs ~8,000 (7,000 as
  // the oldest wave of a lightly loaded one); on the cooperative consumer, alone
  // on its CU at top priority, ~4,200 (the two-lane head ~3,500 since round 4). A sweep of the
  // first two (MSHA_PLAN_LANE_CYCLES / MSHA_PLAN_WAVE_CYCLES,
  // profiles/r03_planned/calibration/): 8,000 / 6,500 ran c5 over 8 GPUs 3.00 ->
  // 2.85 ms, equal at 2 and 4. head_pct scales the head's term (A/B).
  uint32_t wave_block_cycles = 6500;
  uint32_t lane_cycles = 8000;
  uint32_t coop_cycles = 4200;
  uint32_t early_cycles = 3500;  // the same for the early head's kernel (its stand-down rule)
  uint32_t head_pct = 100;
  uint32_t head_per_wg = 128;    // messages per head workgroup (one CU each)
#ifdef MSHA_FOLD_RACE_TEST
  // test build only (MSHA_FOLD_LONGS_SKIP_ODD=1): k_fold_longs leaves every long
  // payload whose table hash is odd unlisted, a state the product kernels cannot
  // reach, to exercise the scan/scatter defensive check
  uint32_t race_test = 0;
#endif
};
// launch_fold_plan: the insert (or, unfolded, the counts) and the scan on st; the
// scatter on sst (the side stream of the late head: when it is not st, st records
// `fork` after the scan and sst waits for it), after scatter_after (may be null:
// the early head's list, against which the scatter resolves the heads).
hipError_t launch_fold_plan(const FoldArgs& a, hipStream_t st, hipStream_t sst, hipEvent_t fork,
                            hipEvent_t scatter_after);
// The early head's first decision and list (k_fold_longs_gate, k_fold_longs): on
// the head's stream, beside the alias insert (both claim through the same table).
hipError_t launch_fold_longs(const FoldArgs& a, int cus, hipStream_t st);
// out[i] = out[rep] for every folded message (FoldArgs::apairs), after the hashing.
hipError_t launch_fold_fill(const FoldArgs& a, uint8_t* out, hipStream_t st);

// Stream sets (stream_kernels.hip): SHA-256 resumed from a chaining state. Lane i
// works on state row r = row ? row[i] : i (state + 8 r: eight host-order words; a
// launch names a row at most once) and on the bytes at arena + off[i] (16-byte
// aligned, kArenaSlack readable bytes after the last lane's; a misaligned start
// sets bit 0 of *err and the lane changes nothing / zeroes its digest).
//  absorb: compresses nblocks[i] whole blocks, no padding, and writes the state
//          back; a lane with no block touches nothing.
//  finish: hashes the last len[i] bytes of a message whose first prefix[i] bytes
//          (a multiple of 64; prefix null: 0) are in the state (state null: the
//          IV), pads for prefix + len bytes and stores the digest at out + 32 i;
//          the state is not written.
// mode (may be null): the load mode the launch ran (pick_mode(n, cus); kPipe runs
// as kPrefetch: these kernels have no software-pipelined variant).
hipError_t launch_stream_absorb(uint32_t* state, const uint8_t* arena, const uint64_t* off,
                                const uint64_t* nblocks, const uint32_t* row, uint64_t n, uint32_t* err,
                                int cus, hipStream_t st, int* mode = nullptr);
hipError_t launch_stream_finish(const uint32_t* state, const uint64_t* prefix, const uint8_t* arena,
                                const uint64_t* off, const uint64_t* len, const uint32_t* row, uint64_t n,
                                uint8_t* out, uint32_t* err, int cus, hipStream_t st, int* mode = nullptr);
// State rows of a set, moved in bulk: state[row[i]] = vals ? vals[i] : the IV (row
// null: row i), and out[i] = state[row[i]]; eight words a row.
hipError_t launch_stream_rows_set(uint32_t* state, const uint32_t* row, const uint32_t* vals, uint64_t n,
                                  hipStream_t st);
hipError_t launch_stream_rows_get(const uint32_t* state, const uint32_t* row, uint32_t* out, uint64_t n,
                                  hipStream_t st);

// absorb on the eight-lane chain (kernels.hip k_absorb_chain8, msha_absorb_chain_device):
// launch_stream_absorb's lanes, rules and result with eight lanes and a producer's share
// a lane, 16 lanes a workgroup, one workgroup a CU. row[i] == kNoLane: lane i is idle.
// One launch, any n < 2^32.
hipError_t launch_absorb_chain8(uint32_t* state, const uint8_t* arena, const uint64_t* off, const uint64_t* nblocks,
                                const uint32_t* row, uint64_t n, uint32_t* err, hipStream_t st);

// Device stream sets (stream_device.hip, msha_dstreams_*): a stream is row s of three
// device arrays -- state + 8 s (eight host-order words), tail + 64 s (the buffered
// length % 64 bytes, zero past them) and length + s. Lane i works on stream
// s = row ? row[i] : i (a launch names a stream at most once); s >= n sets kErrStreamRow
// in *err and touches no stream (finish zeroes the digest). One launch each, no other
// stream, no host wait: capturable.
//  write:  stream s appends the parts [begin[i], begin[i + 1]) of the arena (rules of
//          launch_digest_parts below); a decreasing range sets kErrPartsBegin and
//          leaves the stream as it was.
//  finish: out + 32 i = the digest of everything written to s; snap: the stream then
//          is New() followed by Write(that digest).
//  reset:  the streams return to New().
//  rows_get / rows_set: whole streams to and from packed rows of 26 dwords (state,
//          tail, length low and high); ids checked by the host, id null: row i.
constexpr uint32_t kErrStreamRow = 32u;  // device error word: a row of msha_dstreams_* names a stream >= n
struct DstreamRows {
  uint32_t* state = nullptr;
  uint8_t* tail = nullptr;
  uint64_t* length = nullptr;
  uint64_t n = 0;
};
hipError_t launch_dstream_write(const DstreamRows& r, const uint8_t* arena, const uint64_t* part_off,
                                const uint64_t* part_len, const uint64_t* begin, const uint32_t* row,
                                uint64_t n_rows, uint32_t* err, hipStream_t st);
hipError_t launch_dstream_finish(const DstreamRows& r, const uint32_t* row, uint64_t n_rows, uint8_t* out, bool snap,
                                 uint32_t* err, hipStream_t st);
hipError_t launch_dstream_reset(const DstreamRows& r, const uint32_t* row, uint64_t n_rows, uint32_t* err,
                                hipStream_t st);
hipError_t launch_dstream_rows_get(const DstreamRows& r, const uint32_t* id, uint64_t k, uint32_t* packed,
                                   hipStream_t st);
hipError_t launch_dstream_rows_set(const DstreamRows& r, const uint32_t* id, uint64_t k, const uint32_t* packed,
                                   hipStream_t st);

// Write jobs grouped by stream (stream_jobs.hip, msha_dstreams_write_jobs_device): the
// n_jobs jobs (job_stream[j], job_off[j], job_len[j]) sorted stably by min(stream,
// n_streams) in `passes` radix passes through the two pair buffers (key, job index),
// then goff / glen = the offsets and lengths in that order and begin[t] = the first
// position of a key >= t for t in [0, n_streams]: the CSR launch_dstream_write takes
// with row NULL. A job whose stream is >= n_streams sorts behind begin[n_streams] and
// sets kErrStreamRow. 3 launches a pass and 2 more, all on st; no workgroup waits on
// another. The buffers are laid out by stream_jobs.hpp Layout.
struct StreamJobsArgs {
  const uint32_t* job_stream = nullptr;
  const uint64_t* job_off = nullptr;
  const uint64_t* job_len = nullptr;
  uint64_t n_jobs = 0, n_streams = 0;
  uint2* pairs[2] = {nullptr, nullptr};
  uint64_t* goff = nullptr;
  uint64_t* glen = nullptr;
  uint32_t* counts = nullptr;
  uint64_t* begin = nullptr;
  uint32_t* err = nullptr;
  uint32_t passes = 0;
};
hipError_t launch_stream_jobs(const StreamJobsArgs& a, hipStream_t st, uint32_t* sort_launches,
                              uint32_t* row_launches);

// Write with its long rows routed to the eight-lane chain (stream_chain.hip,
// msha_dstreams_write_routed_device). A routed row holds a slot k < max_long:
// slot_row[k] its row, slot_stream[k] its stream (schain::kNoStream when nobody filled
// the slot), slot_t[k] the bytes the stream buffered, msg_len[k] = slot_t[k] + the sum of
// its part lengths, its message at flat + msg_off[k], blocks[k] the whole blocks the
// chain compresses; taken[r] = 1 marks row r as the chain's. Decisions and layout:
// stream_chain.hpp; claim rules: parts_route.hpp.
struct StreamRouteArgs {
  DstreamRows rows;
  const uint8_t* arena = nullptr;
  const uint64_t* part_off = nullptr;
  const uint64_t* part_len = nullptr;
  const uint64_t* begin = nullptr;  // n_rows + 1
  const uint32_t* row = nullptr;    // n_rows, or null
  uint64_t n_rows = 0;
  uint32_t long_blocks = 0;  // >= 1
  uint32_t max_long = 0;     // slots
  uint64_t long_bytes = 0;   // bytes of the flatten buffer
  uint8_t* taken = nullptr;           // n_rows, rounded up to words
  uint32_t* slot_row = nullptr;       // max_long each:
  uint32_t* slot_stream = nullptr;
  uint32_t* slot_t = nullptr;
  uint64_t* msg_off = nullptr;
  uint64_t* msg_len = nullptr;
  uint64_t* blocks = nullptr;
  unsigned long long* claim = nullptr;  // parts_route::kClaimWords counters
  uint8_t* flat = nullptr;
  uint32_t* err = nullptr;
  uint32_t wave_sum_parts = 0;  // rows of this many parts or more are summed by their wave
};
// One launch each, in the order of the call: init, measure; copy; (the chain:
// launch_absorb_chain8 over the slots); tail; write (Write's row body over the rows with
// taken == 0).
hipError_t launch_sroute_init(const StreamRouteArgs& a, hipStream_t st);
hipError_t launch_sroute_measure(const StreamRouteArgs& a, hipStream_t st);
hipError_t launch_sroute_copy(const StreamRouteArgs& a, hipStream_t st);
hipError_t launch_sroute_tail(const StreamRouteArgs& a, hipStream_t st);
hipError_t launch_dstream_write_rest(const StreamRouteArgs& a, hipStream_t st);

// Multi-part actions (parts_kernels.hip k_digest_parts, msha_hash_actions_device): lane
// i hashes action a = order ? order[i] : i, the concatenation of the parts
// [begin[a], begin[a + 1]) (part j = arena[part_off[j] : part_off[j] + part_len[j]], any
// start, any length), into out + 32 a. arena is 16-byte aligned; the kernel reads only
// the aligned 16-byte granules that hold a byte of a non-empty part
// (parts_gather.hpp). begin[a + 1] < begin[a] sets kErrPartsBegin in *err and zeroes
// the digest. One launch, no other stream, no host wait: capturable.
constexpr uint32_t kErrPartsBegin = 4u;  // device error word; 1 and 2 are the alignment and split-timeout flags
hipError_t launch_digest_parts(const uint8_t* arena, const uint64_t* part_off, const uint64_t* part_len,
                               const uint64_t* begin, const uint32_t* order, uint64_t n, uint8_t* out,
                               uint32_t* err, hipStream_t st);

// Multi-part actions through part lists, planned on the GPU (parts_plan.hip,
// msha_hash_actions_device_planned). List l owns the parts [begin[l], begin[l + 1]);
// action i names list action_list[i] (null: action i is list i, n_actions == n_lists).
// The lanes are the lists some action names, each hashed once, in descending
// block-count class (parts_plan.hpp); the workspace arrays are the caller's, device
// memory, and everything runs on one stream with no host wait: capturable.
constexpr uint32_t kErrPartsList = 8u;  // device error word: an action_list entry >= n_lists
struct PartsPlanArgs {
  const uint8_t* arena = nullptr;
  const uint64_t* part_off = nullptr;
  const uint64_t* part_len = nullptr;
  const uint64_t* begin = nullptr;        // n_lists + 1
  uint64_t n_lists = 0;
  const uint32_t* action_list = nullptr;  // n_actions, or null
  uint64_t n_actions = 0;
  uint8_t* used = nullptr;    // (with action_list) n_lists bytes (rounded up to words) -> 1: some action
                              // names the list
  uint16_t* key16 = nullptr;  // n_lists: out, the list's class key, parts_plan::kNoKey when unused
  uint32_t* cnt = nullptr;    // info + 16: parts_plan::kKeys counters -> bucket starts -> bucket ends
  uint32_t* info = nullptr;   // 16 words: [0] lanes, [2..3] the lanes' block sum (64-bit)
  uint32_t* order = nullptr;  // n_lists: position -> list, kNoLane past the lanes
  uint8_t* table = nullptr;   // (with action_list) 32 n_lists bytes: list l's digest
  uint8_t* out = nullptr;     // 32 n_actions bytes
  uint32_t* err = nullptr;
  uint32_t wave_sum_parts = 0;  // lists of this many parts or more are summed by their wave
};
// init (resets the workspace), mark (with action_list), measure, scan, scatter; *launches = how many kernels that was.
hipError_t launch_parts_plan(const PartsPlanArgs& a, hipStream_t st, uint32_t* launches);
// k_digest_parts_planned over a.order: digests to a.table (with action_list) or a.out.
hipError_t launch_digest_parts_planned(const PartsPlanArgs& a, hipStream_t st);
// (with action_list) out[i] = table[action_list[i]], zeros for an entry out of range.
hipError_t launch_parts_fill(const PartsPlanArgs& a, hipStream_t st);

// The planned call with its long lists routed to the eight-lane chain (parts_plan.hip
// k_route_init / k_route_measure, msha_hash_actions_device_routed): what the routing adds
// to PartsPlanArgs. A routed list l holds a slot s < max_long: sel[s] = l, its bytes go
// to flat + msg_off[s] (msg_len[s] of them, parts_concat.hip k_concat_copy over
// sel / msg_off / msg_len), and lane s of the chain launch (order = chain_order,
// out_idx) hashes them into row l. Claim rules and the unfilled slot: parts_route.hpp.
struct RouteArgs {
  uint32_t long_blocks = 0;  // >= 1
  uint32_t max_long = 0;     // slots
  uint64_t long_bytes = 0;   // bytes of the flatten buffer
  uint32_t* sel = nullptr;          // max_long
  uint64_t* msg_off = nullptr;      // max_long
  uint64_t* msg_len = nullptr;      // max_long
  uint32_t* chain_order = nullptr;  // max_long: slot s -> s, kNoLane when unfilled
  uint32_t* out_idx = nullptr;      // max_long: slot s -> its list
  unsigned long long* claim = nullptr;  // parts_route::kClaimWords counters
};
// init (resets the planned workspace and the route's arrays), mark (with action_list),
// route measure, scan, scatter; *launches = how many kernels that was.
hipError_t launch_parts_route_plan(const PartsPlanArgs& a, const RouteArgs& r, hipStream_t st, uint32_t* launches);

// Part lists flattened into contiguous messages (parts_concat.hip,
// msha_concat_lists_device). Message k is list select[k] (null: list k); its parts go
// back to back to dst + msg_off[k], msg_off a running sum of round16(msg_len). Three
// kernels on one stream, no workspace and no host wait: capturable.
constexpr uint32_t kErrPartsConcat = 16u;  // device error word: a message of msha_concat_lists_device was refused
struct ConcatArgs {
  const uint8_t* arena = nullptr;
  const uint64_t* part_off = nullptr;
  const uint64_t* part_len = nullptr;
  const uint64_t* begin = nullptr;   // n_lists + 1
  uint64_t n_lists = 0;
  const uint32_t* select = nullptr;  // n_select, or null
  uint64_t n_select = 0;
  uint8_t* dst = nullptr;
  uint64_t dst_bytes = 0;
  uint64_t* msg_off = nullptr;       // n_select: between measure and scan, 1 marks an invalid message
  uint64_t* msg_len = nullptr;       // n_select
  uint32_t* err = nullptr;
  uint32_t wave_sum_parts = 0;       // lists of this many parts or more are summed by their wave
};
// k_concat_measure, k_concat_scan, k_concat_copy, in that order; one launch each.
hipError_t launch_concat_measure(const ConcatArgs& a, hipStream_t st);
hipError_t launch_concat_scan(const ConcatArgs& a, hipStream_t st);
hipError_t launch_concat_copy(const ConcatArgs& a, hipStream_t st);

// Digests verified against expected ones (verify.hip, msha_verify_digests_device): slot i
// of got against row expected_idx[i] (null: row i) of expected, 32 bytes a row. The
// compare writes the mask, bit i % 64 of word i / 64 set where slot i differs, all
// ceil(n / 64) words; the scan, one workgroup, writes the first min(bad, list_cap)
// differing slots to bad_list in ascending order and the five words of result. Layout and
// walk: verify.hpp. Two kernels on one stream, no workspace, no device error bit and no
// host wait: capturable.
struct VerifyArgs {
  const uint8_t* got = nullptr;
  uint64_t n = 0;
  const uint8_t* expected = nullptr;
  uint64_t n_expected = 0;
  const uint32_t* expected_idx = nullptr;  // n, or null
  uint64_t* bad_mask = nullptr;            // ceil(n / 64)
  uint32_t* bad_list = nullptr;            // list_cap, null when that is 0
  uint64_t list_cap = 0;
  uint64_t* result = nullptr;              // msha_verify_result as five words
};
// k_verify_compare, then k_verify_scan; one launch each.
hipError_t launch_verify_compare(const VerifyArgs& a, hipStream_t st);
hipError_t launch_verify_scan(const VerifyArgs& a, hipStream_t st);

// Digests grouped by value (group.hip, msha_group_digests_device): slot i's key is
// (scope[i] or 0, the 32 bytes of row i); first[i] the smallest slot with slot i's key,
// group[i] the group's number in order of first occurrence, members[i] its size, the
// first min(groups, group_cap) groups' leaders and sizes in group_first / group_count and
// the five words of result. The table, the positions, the counts, the ids and the tile
// totals are the workspace's (group.hpp Layout). Six kernels on one stream, every
// dependency a kernel boundary, no device error bit and no host wait: capturable.
struct GroupArgs {
  const uint8_t* digests = nullptr;
  uint64_t n = 0;
  const uint32_t* scope = nullptr;    // n, or null: every scope 0
  uint32_t* first = nullptr;          // n
  uint32_t* group = nullptr;          // n
  uint32_t* members = nullptr;        // n, or null
  uint32_t* group_first = nullptr;    // group_cap, null when that is 0
  uint32_t* group_count = nullptr;    // group_cap, null when that is 0
  uint64_t group_cap = 0;
  uint64_t* result = nullptr;         // msha_group_result as five words
  uint64_t* head = nullptr;           // the workspace: group.hpp Layout
  uint32_t* table = nullptr;
  uint32_t* pos = nullptr;
  uint32_t* count = nullptr;
  uint32_t* id = nullptr;
  uint32_t* totals = nullptr;
  uint64_t capacity = 0;              // table positions: group::capacity(n)
  uint64_t seed = 0;                  // of the hash
  uint32_t force_home = 0, force_at = 0;  // MSHA_GROUP_FORCE_HOME: every key's home is force_at
};
// k_group_init, _insert, _resolve, _scan, _rank, _fill, in this order; one launch each.
hipError_t launch_group_init(const GroupArgs& a, hipStream_t st);
hipError_t launch_group_insert(const GroupArgs& a, hipStream_t st);
hipError_t launch_group_resolve(const GroupArgs& a, hipStream_t st);
hipError_t launch_group_scan(const GroupArgs& a, hipStream_t st);
hipError_t launch_group_rank(const GroupArgs& a, hipStream_t st);
hipError_t launch_group_fill(const GroupArgs& a, hipStream_t st);

// A device digest map (dmap.hip, msha_dmap_*): the keys, their counts and the table that
// finds them live in the map's own allocation (dmap.hpp Store) from create to destroy. An
// add groups the call's slots with launch_group_init, _insert and _resolve on a GroupArgs
// that points into the map's per-call workspace (dmap.hpp CallLayout: first, members), and
// then only the leaders touch the map: find (read-only), scan (one workgroup: the numbers
// and the decision), commit (nothing when the call is refused) and fill. Seven kernels on
// one stream, every dependency a kernel boundary, no device error bit and no host wait:
// capturable.
struct DmapArgs {
  const uint8_t* digests = nullptr;
  uint64_t n = 0;
  const uint32_t* scope = nullptr;     // n, or null: every scope 0
  uint32_t threshold = 0;
  uint32_t* id = nullptr;              // n
  uint32_t* before = nullptr;          // n, or null
  uint32_t* after = nullptr;           // n, or null
  uint32_t* crossed_slot = nullptr;    // crossed_cap, null when that is 0
  uint64_t crossed_cap = 0;
  uint64_t* result = nullptr;          // msha_dmap_result as eight words
  // the call's workspace: dmap.hpp CallLayout
  const uint32_t* first = nullptr;     // n: the smallest slot of the call with slot i's key
  const uint32_t* members = nullptr;   // n: at a leader, the call's slots with its key
  uint32_t* lead_id = nullptr;         // n: at a leader, the key's id (kNew until commit numbers it)
  uint32_t* lead_pos = nullptr;        // n: at a leader, where find stopped
  uint32_t* lead_before = nullptr;     // n: at a leader, the key's count before the call
  uint32_t* tot_new = nullptr;         // tiles(n)
  uint32_t* tot_cross = nullptr;       // tiles(n)
  uint64_t* best = nullptr;            // one word, zeroed by k_group_init: the largest (after, ~id)
  // the map: dmap.hpp Store
  uint64_t* head = nullptr;
  uint32_t* table = nullptr;
  uint32_t* key_scope = nullptr;
  uint8_t* key_digests = nullptr;
  uint32_t* count = nullptr;
  uint64_t capacity = 0;               // table positions: dmap::capacity(max_keys)
  uint64_t max_keys = 0;
  uint64_t seed = 0;                   // of the hash that places keys in the map's table
  uint32_t force_home = 0, force_at = 0;  // MSHA_DMAP_FORCE_HOME: every key's home is force_at
  // a vote map's masks (dmap_vote.hpp VoteStore), null and 0 on a plain map: k_dmap_clear zeroes them
  uint32_t* masks = nullptr;           // uint32[max_keys][mask_words], by id
  uint64_t mask_quads = 0;             // 16-byte pieces of the mask store (it is laid out in whole 256 bytes)
};
// k_dmap_find, _scan, _commit, _fill, in this order behind group's first three; one launch each.
hipError_t launch_dmap_find(const DmapArgs& a, hipStream_t st);
hipError_t launch_dmap_scan(const DmapArgs& a, hipStream_t st);
hipError_t launch_dmap_commit(const DmapArgs& a, hipStream_t st);
hipError_t launch_dmap_fill(const DmapArgs& a, hipStream_t st);
// k_dmap_lookup (msha_dmap_find_device): a lane a slot, read-only; id and count (count may
// be null) of slot i's key, or kNoId and 0. k_dmap_clear: the table EMPTY, entries 0.
// Both read the map's fields of a alone, and lookup digests, n, scope, id and after (the count).
hipError_t launch_dmap_lookup(const DmapArgs& a, hipStream_t st);
hipError_t launch_dmap_clear(const DmapArgs& a, hipStream_t st);

// A vote call on a vote map (dmap_vote.hip, msha_dmap_vote_device): a DmapArgs as an add
// fills it (of which `members` is not read), and what dmap_vote.hpp adds: the voters, the
// pair table and the per-slot scratch of VoteLayout. Ten kernels on one stream behind one
// another, the first three group's: capturable as an add is.
struct DmapVoteArgs : DmapArgs {
  const uint32_t* voter = nullptr;     // n
  uint32_t* counted_out = nullptr;     // n, or null
  uint32_t max_voters = 0, mask_words = 0;
  // the call's workspace: dmap_vote.hpp VoteLayout
  uint32_t* pair_table = nullptr;
  uint32_t* pair_pos = nullptr;        // n
  uint32_t* counted = nullptr;         // n
  uint32_t* fresh = nullptr;           // n: at a leader, the counted slots of its key
  uint32_t* tot_counted = nullptr;     // tiles(n)
  uint32_t* tot_repeats = nullptr;     // tiles(n)
  uint32_t* tot_bad = nullptr;         // tiles(n)
  uint64_t* vhead = nullptr;           // dmap_vote::kHeadWords
  uint64_t pair_capacity = 0;          // group::capacity(n)
  uint64_t pair_seed = 0;
  uint32_t pair_force_home = 0, pair_force_at = 0;  // MSHA_DMAP_PAIR_FORCE_HOME
};
// k_vote_find, _pair, _count, _totals, _scan, _commit, _fill, in this order behind group's
// first three; one launch each. k_vote_lookup (msha_dmap_find_votes_device): k_dmap_lookup
// plus the voter's bit into counted_out.
hipError_t launch_vote_find(const DmapVoteArgs& a, hipStream_t st);
hipError_t launch_vote_pair(const DmapVoteArgs& a, hipStream_t st);
hipError_t launch_vote_count(const DmapVoteArgs& a, hipStream_t st);
hipError_t launch_vote_totals(const DmapVoteArgs& a, hipStream_t st);
hipError_t launch_vote_scan(const DmapVoteArgs& a, hipStream_t st);
hipError_t launch_vote_commit(const DmapVoteArgs& a, hipStream_t st);
hipError_t launch_vote_fill(const DmapVoteArgs& a, hipStream_t st);
hipError_t launch_vote_lookup(const DmapVoteArgs& a, hipStream_t st);

// Clock probe (msha_clock_probe): `workgroups` x 256 lanes compress `blocks`
// register-resident blocks each; stamps gets (memtime, memrealtime) at start and
// end per workgroup, 4 words each.
hipError_t launch_clock_probe(uint32_t blocks, uint32_t workgroups, uint64_t* stamps, uint32_t* sink,
                              hipStream_t st);

}  // namespace msha
