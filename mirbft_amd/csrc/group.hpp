// How msha_group_digests_device (include/mirsha.h "Digests grouped by value on the GPU";
// group.hip) finds the groups, lays out its workspace and numbers its answer.
//
//   key      slot i's key is (scope[i] or 0, the 32 bytes of row i): Key, nine dwords. Two
//            slots are one group iff same() holds, the OR of the XOR of all nine. Nothing
//            else ever joins two slots.
//   table    capacity(n) = bit_ceil(2 n), at least kMinCapacity, entries of 4 bytes: EMPTY
//            or the smallest slot seen so far of the key that owns the position. It is
//            never more than half full, so a probe always ends.
//   insert   probe(): from home(), linear with wrap-around. A relaxed load; a claim
//            (EMPTY -> i) only where EMPTY was seen; on an owner j the full compare with
//            slot j's key; equal: min only when i < j, and stop; different: the next
//            position. A key holds ONE position (the claim's loser sees the winner and
//            compares), and once every lane is through, the entry there is the key's
//            smallest slot, whatever order the lanes ran in. Only where the lanes stop
//            depends on the hash, its seed and the order; nothing written for the caller
//            does.
//   resolve  first[i] = table[pos[i]]; slot i leads iff first[i] == i. A tile of kTile
//            slots counts its leaders and adds its members to the leaders' counters, the
//            adds to one leader joined in a tile table (tile_slot) first.
//   scan     ONE workgroup of kScanThreads threads turns the tile totals into exclusive
//            bases, kScanTiles a chunk with a carry (scan_walk), and leaves `groups`.
//   rank     a leader's group id is its tile's base + the leaders before it in the tile
//            (rank_in_tile over the waves' ballots): ascending leaders, so first
//            occurrence order. best_key() packs (count, ~id): its maximum is the largest
//            group, the smallest id among equals.
//   fill     group[i] = id[first[i]], members[i] = count[first[i]], and result_words().
//
// This header compiles for the host as well: tests/cpp/group_check.cpp runs probe,
// resolve, scan, rank and fill with it under AddressSanitizer + UBSan, every array at
// exactly its contract size, the insert in three slot orders.
#pragma once
#include <stdint.h>

#include "parts_gather.hpp"
#include "workspace_rule.hpp"

namespace msha {
namespace group {

constexpr uint32_t kTile = 256;           // slots a workgroup of the per-slot kernels takes: a lane a slot
constexpr uint32_t kTileWaves = 4;        // kTile / 64
constexpr uint32_t kTileSlots = 512;      // the tile table: a tile holds at most kTile leaders, so it is never full
constexpr uint32_t kScanThreads = 256;    // k_group_scan: one workgroup ...
constexpr uint32_t kScanTiles = kScanThreads;  // ... of one tile total a thread and chunk
constexpr uint32_t kMinCapacity = 64;     // one wave's worth
constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // a table entry nobody owns; no slot (n <= 2^30)
constexpr uint64_t kMaxSlots = uint64_t(1) << 30;
constexpr uint32_t kLaunches = 6;         // init, insert, resolve, scan, rank, fill

static_assert(kTile == 64 * kTileWaves, "a tile is whole waves");
static_assert(kTileSlots >= 2 * kTile && (kTileSlots & (kTileSlots - 1)) == 0, "the tile table stays half empty");

// Table positions for n slots (n <= kMaxSlots): a power of two, at least 2 n.
MSHA_HD uint64_t capacity(uint64_t n) {
  uint64_t c = kMinCapacity;
  while (c < 2 * n) c <<= 1;
  return c;
}
MSHA_HD uint64_t tiles(uint64_t n) { return (n + kTile - 1) / kTile; }

// The workspace of a call over n slots, as byte offsets from its base (256-aligned
// each). head: two 8-byte words, kHeadBest and kHeadGroups.
constexpr uint32_t kHeadBest = 0, kHeadGroups = 1;
struct Layout {
  uint64_t cap, head, table, pos, count, id, totals, bytes;
  MSHA_HD explicit Layout(uint64_t n) {
    cap = capacity(n);
    head = 0;
    table = round256(16);                     // uint32[cap]: EMPTY or the key's smallest slot so far
    pos = table + round256(4 * cap);          // uint32[n]: where slot i's probe stopped
    count = pos + round256(4 * n);            // uint32[n]: members, at the leader's slot
    id = count + round256(4 * n);             // uint32[n]: group id, at the leader's slot
    totals = id + round256(4 * n);            // uint32[tiles(n)]: leaders a tile, then the leaders before it
    bytes = totals + round256(4 * tiles(n));
  }
};

struct Key {
  uint32_t scope;
  parts::Granule lo, hi;  // row bytes 0..15 and 16..31
};

// The full compare: all 36 bytes.
MSHA_HD bool same(const Key& a, const Key& b) {
  uint32_t acc = a.scope ^ b.scope;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t k = 0; k < 4; ++k) acc |= (a.lo.d[k] ^ b.lo.d[k]) | (a.hi.d[k] ^ b.hi.d[k]);
  return acc == 0;
}

// The keyed hash: the seed is the state the nine dwords are folded into, a dword pair a
// step, each step a xor, an odd multiply and a shift that brings the high half down, and
// it is added again before the last step. Which keys share a home depends on the seed.
MSHA_HD uint64_t fold(uint64_t h, uint64_t v) {
  h = (h ^ v) * 0xBF58476D1CE4E5B9ull;
  return h ^ (h >> 29);
}
MSHA_HD uint64_t hash(uint64_t seed, const Key& k) {
  uint64_t h = fold(seed ^ 0x9E3779B97F4A7C15ull, k.scope);
  h = fold(h, (uint64_t)k.lo.d[0] | (uint64_t)k.lo.d[1] << 32);
  h = fold(h, (uint64_t)k.lo.d[2] | (uint64_t)k.lo.d[3] << 32);
  h = fold(h, (uint64_t)k.hi.d[0] | (uint64_t)k.hi.d[1] << 32);
  h = fold(h, (uint64_t)k.hi.d[2] | (uint64_t)k.hi.d[3] << 32);
  h = (h + seed) * 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}

// How a call places its keys. force_home (MSHA_GROUP_FORCE_HOME, a diagnostic): every
// key's home is force_at.
struct Placement {
  uint64_t seed = 0;
  uint32_t mask = 0;  // capacity - 1
  uint32_t force_home = 0, force_at = 0;
};
MSHA_HD uint32_t home_of(const Placement& p, uint64_t hashed) {  // hashed: hash(p.seed, key)
  return p.force_home ? (p.force_at & p.mask) : ((uint32_t)hashed & p.mask);
}
MSHA_HD uint32_t home(const Placement& p, const Key& k) { return home_of(p, hash(p.seed, k)); }

// Slot i's insert: the position it stopped at. load(p): the entry at p, a relaxed atomic
// load; claim(p, i): compare-and-swap EMPTY -> i, returns what the entry held; lower(p, i):
// atomic min; same_as(j): is slot j's key slot i's (the full compare).
template <class Load, class Claim, class Lower, class SameAs>
MSHA_HD uint32_t probe(uint32_t i, uint32_t home_pos, uint32_t mask, Load&& load, Claim&& claim, Lower&& lower,
                       SameAs&& same_as) {
  uint32_t p = home_pos;
  for (;;) {
    uint32_t v = load(p);
    if (v == kEmpty) v = claim(p, i);
    if (v == kEmpty) return p;  // claimed: slot i owns p until a smaller slot of its key comes
    if (same_as(v)) {
      if (i < v) lower(p, i);
      return p;
    }
    p = (p + 1) & mask;
  }
}

// The tile table of resolve: the position of leader `first` among kTileSlots, claimed on
// first sight. key(h): the entry at h (kEmpty: free); claim(h, first): compare-and-swap
// kEmpty -> first, returns what the entry held.
MSHA_HD uint32_t tile_home(uint32_t first) { return (first * 0x9E3779B1u) >> (32 - 9); }  // 9 = log2(kTileSlots)
static_assert(kTileSlots == 1u << 9, "tile_home keeps nine bits");
template <class KeyAt, class Claim>
MSHA_HD uint32_t tile_slot(uint32_t first, KeyAt&& key, Claim&& claim) {
  uint32_t h = tile_home(first);
  for (;;) {
    uint32_t cur = key(h);
    if (cur == kEmpty) cur = claim(h, first);
    if (cur == kEmpty || cur == first) return h;
    h = (h + 1) & (kTileSlots - 1);
  }
}

// Thread t's part of the scan over `count` tile totals: load(k) the leaders of tile k,
// store(k, before) the leaders of the tiles before it; prefix(c, &before, &all) the sum of
// c over the threads below t and over all threads of this chunk (every thread calls it
// once a chunk, so it may hold barriers). Returns the number of leaders: `groups`.
template <class Load, class Prefix, class Store>
MSHA_HD uint64_t scan_walk(uint64_t count, uint32_t t, Load&& load, Prefix&& prefix, Store&& store) {
  uint64_t base = 0;
  for (uint64_t k0 = 0; k0 < count; k0 += kScanTiles) {
    const uint64_t k = k0 + t;
    const uint32_t c = k < count ? load(k) : 0;
    uint32_t before = 0, all = 0;
    prefix(c, &before, &all);
    if (k < count) store(k, (uint32_t)(base + before));
    base += all;
  }
  return base;
}

// The leaders before lane `lane` of wave `wave` in its tile, from the tile's ballots of
// "leads" (bit l of ballots[w]: lane l of wave w).
MSHA_HD uint32_t rank_in_tile(const uint64_t (&ballots)[kTileWaves], uint32_t wave, uint32_t lane) {
  const uint64_t below = (uint64_t(1) << lane) - 1u;
  uint32_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t w = 0; w < kTileWaves; ++w) {  // (no entry is picked by a run-time index)
    if (w < wave) r += (uint32_t)__builtin_popcountll(ballots[w]);
    if (w == wave) r += (uint32_t)__builtin_popcountll(ballots[w] & below);
  }
  return r;
}

// (count, id) ordered by count, then by the smaller id: the maximum over the groups is
// max_count and max_group. 0 is below every group's key (a group has a member).
MSHA_HD uint64_t best_key(uint32_t count, uint32_t id) { return (uint64_t)count << 32 | (uint32_t)~id; }
MSHA_HD uint64_t best_count(uint64_t key) { return key >> 32; }
MSHA_HD uint64_t best_group(uint64_t key) { return (uint32_t)~(uint32_t)key; }

// msha_group_result's five words, in its field order.
MSHA_HD void result_words(uint64_t n, uint64_t groups, uint64_t group_cap, uint64_t best, uint64_t (&r)[5]) {
  r[0] = n;
  r[1] = groups;
  r[2] = groups < group_cap ? groups : group_cap;
  r[3] = best_count(best);
  r[4] = best_group(best);
}

}  // namespace group
}  // namespace msha
