// How a vote map (include/mirsha.h "Device digest maps that count voters"; dmap_vote.hip,
// dmap.cpp) counts each voter once a key: what it keeps beside a plain map's store, the
// workspace of a vote call, and the rules its kernels run. Everything of dmap.hpp holds
// unchanged: the key, the table, the ids, find_probe, insert_probe, refuse, crossed.
//
//   mask     uint32 mask[max_keys][words], words = ceil(max_voters / 32), by entry id: bit
//            v % 32 of word v / 32 is voter v. count[id] == popcount(mask[id]) at every
//            kernel boundary outside a vote call. EMPTY MASKS ARE CLEAR'S AND CREATE'S:
//            k_dmap_clear zeroes the whole mask store (create runs it), and only a counted
//            slot of a call that is not refused ever sets a bit, at an id below `entries`;
//            so the mask of an id not yet given out is empty and commit has none to empty.
//   pair     slot i's pair is (first[i], voter[i]): the call's leader of its key and its
//            sender, 8 bytes. A second table of the call's, capacity group::capacity(n),
//            joins equal pairs with group::probe as it stands: an entry is EMPTY or the
//            smallest slot of the pair so far. Slots whose voter is out of range do not
//            enter. Slot i is a PAIR LEADER iff its entry holds i after the launch.
//   counted  counted(): a pair leader whose voter's bit is not in the key's mask as the
//            call found it (a key the map does not hold has an empty mask). The smallest
//            slot of equal votes, whatever order the lanes ran in.
//   fresh    fresh[leader] = the counted slots of the leader's key in this call; after =
//            before + fresh, at most max_voters: nothing saturates.
//   chain    kLaunches kernels: group's init, insert, resolve; find (the leaders' read-only
//            walk; it also empties the pair table and zeroes fresh, which nothing before
//            it reads), pair, count, totals, scan, commit, fill. A counted slot's bit is
//            set by fill, a launch behind commit, so the new id and its empty mask are
//            there first; commit and fill do nothing to the map when the call is refused.
//
// This header compiles for the host as well: tests/cpp/dmap_vote_check.cpp replays it under
// AddressSanitizer + UBSan, every array at exactly its contract size, the pair insert in
// three slot orders.
#pragma once
#include <stdint.h>

#include "dmap.hpp"

namespace msha {
namespace dmap_vote {

constexpr uint32_t kMaxVoters = 1024;
constexpr uint32_t kLaunches = 10;  // group's init, insert, resolve; find, pair, count, totals, scan, commit, fill
constexpr uint32_t kResultWords = 11;

MSHA_HD uint32_t words(uint32_t max_voters) { return (max_voters + 31u) / 32u; }
MSHA_HD uint32_t mask_word(uint32_t voter) { return voter / 32u; }
MSHA_HD uint32_t mask_bit(uint32_t voter) { return 1u << (voter % 32u); }

// What a vote map owns: a plain map's store, then the masks (256-aligned).
struct VoteStore : dmap::Store {
  uint64_t mask_words, mask;
  MSHA_HD VoteStore(uint64_t max_keys, uint32_t max_voters) : dmap::Store(max_keys) {
    mask_words = words(max_voters);
    mask = bytes;                                    // uint32[max_keys][mask_words], by id
    bytes = mask + round256(4 * mask_words * max_keys);
  }
};

// The workspace's own 8-byte words: scan's sums of the three tile totals below.
constexpr uint32_t kHeadCounted = 0, kHeadRepeats = 1, kHeadBad = 2, kHeadWords = 3;

// The workspace of a vote over n slots: an add's (of which g.count is not used: `fresh`
// stands where an add has the members), then the pair table, where each slot's pair
// insert stopped, counted and fresh, three more totals a tile and three sums.
struct VoteLayout {
  dmap::CallLayout c;
  uint64_t pair_cap, pair_table, pair_pos, counted, fresh, tot_counted, tot_repeats, tot_bad, head, bytes;
  MSHA_HD explicit VoteLayout(uint64_t n) : c(n) {
    pair_cap = group::capacity(n);
    pair_table = c.bytes;                                           // uint32[pair_cap]: EMPTY or the pair's smallest slot so far
    pair_pos = pair_table + round256(4 * pair_cap);                 // uint32[n]: where slot i's pair insert stopped
    counted = pair_pos + round256(4 * n);                           // uint32[n]: 0 or 1
    fresh = counted + round256(4 * n);                              // uint32[n]: at a leader, the counted slots of its key
    tot_counted = fresh + round256(4 * n);                          // uint32[tiles(n)]
    tot_repeats = tot_counted + round256(4 * group::tiles(n));      // uint32[tiles(n)]
    tot_bad = tot_repeats + round256(4 * group::tiles(n));          // uint32[tiles(n)]
    head = tot_bad + round256(4 * group::tiles(n));                 // uint64[kHeadWords]
    bytes = head + round256(8 * kHeadWords);
  }
};

// The pair's hash: group::fold over the eight bytes, keyed like group::hash.
MSHA_HD uint64_t pair_hash(uint64_t seed, uint32_t first, uint32_t voter) {
  uint64_t h = group::fold(seed ^ 0x9E3779B97F4A7C15ull, (uint64_t)first | (uint64_t)voter << 32);
  h = (h + seed) * 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}
MSHA_HD bool pair_same(uint32_t first_a, uint32_t voter_a, uint32_t first_b, uint32_t voter_b) {
  return ((first_a ^ first_b) | (voter_a ^ voter_b)) == 0;
}

MSHA_HD bool in_range(uint32_t voter, uint32_t max_voters) { return voter < max_voters; }

// COUNTED of the contract. pair_leader: the slot's pair entry holds the slot (which implies
// a voter in range); word: the key's mask word mask_word(voter) as the call found it, 0 for
// a key the map does not hold.
MSHA_HD bool counted(bool pair_leader, uint32_t word, uint32_t voter) { return pair_leader && (word & mask_bit(voter)) == 0; }

// msha_dmap_vote_result's eleven words, in its field order: add's eight, then counted,
// repeats, bad_voters, which a refused call reports as well.
MSHA_HD void result_words(uint64_t n, uint64_t entries_before, uint64_t added, bool full, uint64_t crossed_keys,
                          uint64_t crossed_cap, uint64_t best, uint64_t counted_slots, uint64_t repeats,
                          uint64_t bad_voters, uint64_t (&r)[kResultWords]) {
  uint64_t head[8];
  dmap::result_words(n, entries_before, added, full, crossed_keys, crossed_cap, best, head);
  for (uint32_t k = 0; k < 8; ++k) r[k] = head[k];
  r[8] = counted_slots;
  r[9] = repeats;
  r[10] = bad_voters;
}

}  // namespace dmap_vote
}  // namespace msha
