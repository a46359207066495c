// The decisions of msha_hash_actions_device_routed (parts_plan.hip k_route_measure):
// which list is long, what a long list must claim to be routed, and what a slot nobody
// filled holds.
//
// A long list claims a SLOT first (one of max_long: its row in sel / msg_off / msg_len
// and its lane of the chain kernel), then ROOM in the flatten buffer. A slot is claimed
// by counting up: tickets at or past max_long lose, and the counter going on past it
// harms nothing. Room is claimed by compare-and-swap on the bytes given out so far, and
// only where the list fits behind them (parts_concat.hpp fits), so the counter is at
// every moment the exact sum of round16(len) over the lists that were given room, never
// runs past long_bytes and cannot overflow. A list that wins a slot and then finds no
// room leaves its slot unfilled; an unfilled slot is an inactive lane of the chain
// kernel and a message of no bytes to the copy.
//
// This header compiles for the host as well: tests/cpp/parts_route_check.cpp drives it
// under AddressSanitizer + UBSan, and tests/cpp/call_workspace_check.cpp the workspace
// layout.
#pragma once
#include <stdint.h>

#include "parts_concat.hpp"
#include "parts_plan.hpp"

namespace msha {
namespace parts_route {

// The claim counters, 64-bit words of RouteArgs::claim (all zeroed by the init kernel).
constexpr uint32_t kClaimBytes = 0;   // bytes of the flatten buffer given out
constexpr uint32_t kClaimSlots = 1;   // slot tickets drawn (may pass max_long)
constexpr uint32_t kClaimRouted = 2;  // lists routed
constexpr uint32_t kClaimWords = 8;

// What an unfilled slot holds: no bytes for the copy, no lane for the chain.
constexpr uint64_t kUnfilledLen = 0;
constexpr uint32_t kUnfilledOrder = 0xFFFFFFFFu;  // kernels.hpp kNoLane

// Is a valid, named list of `blocks` blocks long? (long_blocks >= 1.)
MSHA_HD bool is_long(uint64_t blocks, uint32_t long_blocks) { return blocks >= long_blocks; }

// Does slot ticket `ticket` win one of max_long slots?
MSHA_HD bool slot_ok(uint64_t ticket, uint32_t max_long) { return ticket < max_long; }

// Can a list of `len` bytes be given room behind the `given` bytes already given out?
// On success *next is what the counter becomes. given + round16(len) + slack <=
// long_bytes, without overflow for any len.
MSHA_HD bool room_ok(uint64_t given, uint64_t len, uint64_t long_bytes, uint64_t slack, uint64_t* next) {
  if (!parts_concat::fits(given, len, long_bytes, slack)) return false;
  *next = given + parts_concat::round16(len);
  return true;
}

// The workspace of a call over n lists with m slots (n, m < 2^32) and a flatten buffer of
// flat_bytes (<= 2^48: the sum stays far below 2^64), byte offsets from its base: info
// and the counters, one array to k_route_init, lie at 0; the claim counters; the slots'
// five arrays; the planned call's order, keys, used flags and digest table (plan, placed
// behind the slots); the buffer. The members are initialised in this order.
struct Layout {
  uint64_t claim, msg_off, msg_len, sel, chain, out_idx;
  parts_plan::Layout plan;
  uint64_t flat, bytes;
  MSHA_HD Layout(uint64_t n, uint64_t m, uint64_t flat_bytes, bool with_list)
      : claim(parts_plan::head_bytes()),
        msg_off(claim + round64(8ull * kClaimWords)),
        msg_len(msg_off + round64(8 * m)),
        sel(msg_len + round64(8 * m)),
        chain(sel + round64(4 * m)),
        out_idx(chain + round64(4 * m)),
        plan(n, with_list, out_idx + round64(4 * m)),
        flat(round256(plan.bytes)),
        bytes(flat + flat_bytes) {}
};

}  // namespace parts_route
}  // namespace msha
