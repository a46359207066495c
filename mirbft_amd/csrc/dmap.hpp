// How a device digest map (include/mirsha.h "Device digest maps"; dmap.hip, dmap.cpp)
// keeps its keys across calls, lays out its memory and numbers its answer.
//
//   key      as in group.hpp: (scope, 32 bytes), nine dwords, joined by group::same()
//            alone -- between the slots of a call and against the stored keys.
//   store    what the map owns from create to destroy (Store): a head of 8-byte words,
//            the table, and the key store and the counts, indexed by ENTRY ID: a key's
//            position in order of first occurrence since the last clear.
//   table    capacity(max_keys) = bit_ceil(2 max_keys), at least 64, entries of 4 bytes:
//            EMPTY or an id. At most max_keys ids are ever in it, so it is never more
//            than half full and a probe always ends. Nothing is ever taken out (no erase:
//            open addressing would need tombstones), so every position between a key's
//            home and where it lies stays occupied, and a walk from home that meets
//            EMPTY has proven the key absent.
//   add      first the call's own slots are grouped with group.hpp's insert and resolve
//            on a table of the call's (CallLayout): first[i], and the members at each
//            leader. From there on ONLY LEADERS touch the map's table, so no two probing
//            lanes ever hold the same key.
//   find     find_probe(): read-only, from home. An id whose stored key is the lane's:
//            found. EMPTY: new, and the position is remembered.
//   number   a new leader's id is entries_before + the new leaders before it in the call
//            (new_id): existing keys between two new ones use up no number. The call is
//            refused whole when refuse() holds; nothing of the map is written then.
//   commit   insert_probe(): from the remembered position, compare-and-swap EMPTY -> id,
//            stepping past anything else WITHOUT a compare: the existing keys were all
//            compared in find, and the other new ones are other leaders, other keys.
//            Where an id lands depends on the order the lanes ran in; nothing the caller
//            or msha_dmap_read sees does.
//   counts   after = sat_add(before, the key's slots in this call); a key crossed iff
//            crossed(threshold, before, after).
//
// This header compiles for the host as well: tests/cpp/dmap_check.cpp runs both probes,
// the numbering, crossed, sat_add, refuse and result_words with it under AddressSanitizer
// + UBSan, every array at exactly its contract size, the insert in three slot orders.
#pragma once
#include <stdint.h>

#include "group.hpp"

namespace msha {
namespace dmap {

constexpr uint32_t kEmpty = group::kEmpty;  // a table entry nobody owns; no id (max_keys <= 2^30)
constexpr uint32_t kNew = 0xFFFFFFFFu;      // find's answer for a key the map does not hold
constexpr uint32_t kNoId = 0xFFFFFFFFu;     // d_id of a refused call and of an absent key
constexpr uint64_t kMaxKeys = uint64_t(1) << 30;
constexpr uint64_t kMaxSlots = group::kMaxSlots;
constexpr uint32_t kLaunches = 7;  // group's init, insert, resolve; find, scan, commit, fill
constexpr uint32_t kTile = group::kTile;
constexpr uint32_t kTileWaves = group::kTileWaves;

// Table positions of a map of max_keys keys (max_keys <= kMaxKeys): a power of two, at
// least 2 max_keys.
MSHA_HD uint64_t capacity(uint64_t max_keys) { return group::capacity(max_keys); }

// The head's 8-byte words. kHeadEntries is the map's; the others are what one add's
// kernels hand to one another (scan writes them, commit and fill read them).
constexpr uint32_t kHeadEntries = 0, kHeadAdded = 1, kHeadCrossed = 2, kHeadFull = 3, kHeadWords = 4;

// What a map owns, as byte offsets from the base of its one allocation (256-aligned each).
struct Store {
  uint64_t cap, head, table, scope, digests, count, bytes;
  MSHA_HD explicit Store(uint64_t max_keys) {
    cap = capacity(max_keys);
    head = 0;
    table = round256(8 * kHeadWords);            // uint32[cap]: EMPTY or an id
    scope = table + round256(4 * cap);           // uint32[max_keys]: the key's scope, by id
    digests = scope + round256(4 * max_keys);    // 32 bytes a key, by id, 16-byte aligned
    count = digests + round256(32 * max_keys);   // uint32[max_keys]: the key's count, by id
    bytes = count + round256(4 * max_keys);
  }
};

// The workspace of an add over n slots: group's own for its three kernels (of which
// `count` holds the members at each leader, `id` the leader's entry id and head[kHeadBest]
// the largest (after, ~id)), then first[], and at each leader where find stopped and the
// key's count before the call, and two totals a tile.
struct CallLayout {
  group::Layout g;
  uint64_t first, ppos, before, tot_new, tot_cross, bytes;
  MSHA_HD explicit CallLayout(uint64_t n) : g(n) {
    first = g.bytes;                                         // uint32[n]
    ppos = first + round256(4 * n);                          // uint32[n]
    before = ppos + round256(4 * n);                         // uint32[n]
    tot_new = before + round256(4 * n);                      // uint32[tiles(n)]: new leaders a tile, then those before it
    tot_cross = tot_new + round256(4 * group::tiles(n));     // uint32[tiles(n)]: the same for crossing leaders
    bytes = tot_cross + round256(4 * group::tiles(n));
  }
};

// Where find stopped: the id found there, or kNew at an EMPTY position.
struct Found {
  uint32_t id, pos;
};

// A leader's read-only walk. load(p): the entry at p, a relaxed atomic load; same_as(e):
// is stored key e the lane's key (the full compare).
template <class Load, class SameAs>
MSHA_HD Found find_probe(uint32_t home_pos, uint32_t mask, Load&& load, SameAs&& same_as) {
  uint32_t p = home_pos;
  for (;;) {
    const uint32_t v = load(p);
    if (v == kEmpty) return Found{kNew, p};
    if (same_as(v)) return Found{v, p};
    p = (p + 1) & mask;
  }
}

// A new leader's insert, from where its find stopped. claim(p, id): compare-and-swap
// EMPTY -> id, returns what the entry held. Returns the position taken.
template <class Claim>
MSHA_HD uint32_t insert_probe(uint32_t id, uint32_t from, uint32_t mask, Claim&& claim) {
  uint32_t p = from;
  while (claim(p, id) != kEmpty) p = (p + 1) & mask;
  return p;
}

// The id of the new leader that has `rank` new leaders of this call before it.
MSHA_HD uint32_t new_id(uint64_t entries_before, uint64_t rank) { return (uint32_t)(entries_before + rank); }

// The call is refused whole: its new keys do not all fit.
MSHA_HD bool refuse(uint64_t entries_before, uint64_t added, uint64_t max_keys) { return entries_before + added > max_keys; }

MSHA_HD uint32_t sat_add(uint32_t before, uint32_t slots) {
  const uint64_t s = (uint64_t)before + slots;
  return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
}

MSHA_HD bool crossed(uint32_t threshold, uint32_t before, uint32_t after) {
  return threshold > 0 && before < threshold && threshold <= after;
}

// msha_dmap_result's eight words, in its field order. best: the largest
// group::best_key(after, id) over the keys the call touched (0: none was).
MSHA_HD void result_words(uint64_t n, uint64_t entries_before, uint64_t added, bool full, uint64_t crossed_keys,
                          uint64_t crossed_cap, uint64_t best, uint64_t (&r)[8]) {
  const uint64_t c = full ? 0 : crossed_keys;
  r[0] = n;
  r[1] = full ? entries_before : entries_before + added;
  r[2] = added;
  r[3] = full ? 1 : 0;
  r[4] = c;
  r[5] = c < crossed_cap ? c : crossed_cap;
  r[6] = full || best == 0 ? 0 : group::best_count(best);
  r[7] = full || best == 0 ? 0 : group::best_group(best);
}

}  // namespace dmap
}  // namespace msha
