// The decisions of the eight-lane absorb chain (kernels.hip k_absorb_chain8,
// msha_absorb_chain_device) and of msha_dstreams_write_routed_device (stream_chain.hip):
//   - which producer schedules which block, which LDS slot it fills and after which
//     blocks a producer calls the workgroup barrier, with the number of barrier calls of
//     either role as a function of NB (the workgroup's longest lane, in blocks) and per
//     (blocks a barrier): a mismatch between the roles is a hang, so the two counts are
//     compared on the host before the kernel ever runs;
//   - which row of a routed write is LONG, what its message in the flatten buffer is
//     (the stream's t buffered bytes, then its parts), which of the message's bytes
//     become the stream's new tail row, and the new length;
//   - where the arrays of the set's route workspace lie.
// The claim rules (slot, then room) are parts_route.hpp's, unchanged.
//
// This header compiles for the host as well: tests/cpp/stream_chain_check.cpp drives it
// under AddressSanitizer + UBSan.
#pragma once
#include <stdint.h>

#include "parts_route.hpp"
#include "stream_device.hpp"

namespace msha {
namespace schain {

// ---- the barrier schedule of k_absorb_chain8 (chain8_body's, without its tail blocks) ----

constexpr uint32_t kProducers = 2;       // producer waves: even and odd blocks (kernels.hip kC8Producers)
constexpr uint32_t kPairMinBlocks = 64;  // NB from which a barrier covers two blocks (kernels.hip kC2PairMinBlocks)

// Blocks a barrier: 2 for a workgroup whose longest lane has kPairMinBlocks blocks or
// more, when the kernel has the pair path at all (max_per 2), else 1.
MSHA_HD uint32_t per_for(uint32_t NB, uint32_t max_per) { return max_per == 2 && NB >= kPairMinBlocks ? 2u : 1u; }
// The producer wave that schedules block b.
MSHA_HD uint32_t producer_of(uint32_t b) { return b % kProducers; }
// Block b's K+W go to kw[slot_of(b, per)][sub_of(b, per)]: group g = b / per fills slot g & 1.
MSHA_HD uint32_t slot_of(uint32_t b, uint32_t per) { return (b / per) & 1u; }
MSHA_HD uint32_t sub_of(uint32_t b, uint32_t per) { return b % per; }
// Does a producer call the barrier after block b of NB? (After a group's last block.)
MSHA_HD bool producer_barrier_after(uint32_t b, uint32_t NB, uint32_t per) { return b % per == per - 1 || b + 1 == NB; }
// Groups of `per` blocks in NB blocks, without overflow.
MSHA_HD uint32_t groups(uint32_t NB, uint32_t per) { return NB / per + (NB % per != 0 ? 1u : 0u); }
// May a producer prefetch block `next` of a lane of nb blocks? Never one past its last.
MSHA_HD bool prefetch_ok(uint32_t next, uint32_t nb) { return next < nb; }

// Barrier calls of a producer wave for a workgroup of NB > 0 blocks, counted by the
// kernel's own loop: one after every group, and the consumers' last (they wait one
// group ahead). Both producers walk every b, so the count does not depend on the wave.
MSHA_HD uint64_t producer_barrier_calls(uint32_t NB, uint32_t per) {
  uint64_t calls = 0;
  for (uint32_t b = 0; b < NB; ++b)
    if (producer_barrier_after(b, NB, per)) ++calls;
  return calls + 1;
}
// The same for a consumer wave: barrier 0 before its first read, then one per group
// (pair path: per pair of blocks) before the group's rounds.
MSHA_HD uint64_t consumer_barrier_calls(uint32_t NB, uint32_t per) {
  uint64_t calls = 1;
  if (per == 2) {
    const uint32_t NP = groups(NB, 2);
    for (uint32_t g = 0; g < NP; ++g) {
      ++calls;
      if (++g == NP) break;
      ++calls;
    }
    return calls;
  }
  for (uint32_t b = 0; b < NB; ++b) {
    ++calls;
    if (++b == NB) break;
    ++calls;
  }
  return calls;
}

// ---- a routed row ----

// Part sums above this are no real list's (the arena is smaller); such a row is a lane.
constexpr uint64_t kMaxSum = 1ull << 62;

// Whole blocks a write of `sum` bytes compresses on a stream that buffers t (< 64) bytes.
MSHA_HD uint64_t whole_blocks(uint32_t t, uint64_t sum) { return sum / 64 + (t + sum % 64) / 64; }
// Bytes the stream buffers afterwards.
MSHA_HD uint32_t new_tail(uint32_t t, uint64_t sum) { return (uint32_t)((t + sum % 64) % 64); }
// Is a valid row (stream < n, part range valid) LONG? long_blocks >= 1.
MSHA_HD bool is_long_row(uint32_t t, uint64_t sum, uint32_t long_blocks) {
  return sum <= kMaxSum && parts_route::is_long(whole_blocks(t, sum), long_blocks);
}
// The routed row's message in the flatten buffer: t buffered bytes, then the parts.
MSHA_HD uint64_t message_len(uint32_t t, uint64_t sum) { return (uint64_t)t + sum; }  // sum <= kMaxSum
// The stream's length after the write: hash.Hash counts modulo 2^64, as Write's kernel does.
MSHA_HD uint64_t new_length(uint64_t length, uint64_t sum) { return length + sum; }

// The new tail row of a routed stream from its message of `total` bytes, `whole` blocks
// of which were compressed: message bytes [64 whole, total) and zeros up to 64. Granule
// g (0..3) of the row is read from the message only when it holds one of those bytes.
MSHA_HD uint32_t tail_bytes(uint64_t total, uint64_t whole) { return (uint32_t)(total - 64 * whole); }  // < 64
MSHA_HD bool tail_granule_read(uint32_t g, uint32_t rem) { return 16u * g < rem; }
// Dword j (0..15) of the row from the message's dword at 64 whole + 4 j (0 where the
// granule is not read): dstream::tail_dword zeroes the bytes at or past rem.
MSHA_HD uint32_t tail_row_dword(uint32_t message_dword, uint32_t j, uint32_t rem) {
  return dstream::tail_dword(message_dword, j, rem);
}

// ---- the set's route workspace ----

// What an unfilled slot holds: no stream for the chain and the tail, no bytes for the copy.
constexpr uint32_t kNoStream = 0xFFFFFFFFu;  // kernels.hpp kNoLane

// Byte offsets for a call of n_rows rows, m slots and a flatten buffer of flat_bytes
// (n_rows < 2^32, m < 2^32, flat_bytes <= 2^48: the sum stays far below 2^64): the claim
// words, a flag byte a row, six arrays a slot, the buffer.
struct Layout {
  uint64_t claim, taken, slot_row, slot_stream, slot_t, msg_off, msg_len, blocks, flat, bytes;
  bool ok;
  MSHA_HD Layout(uint64_t n_rows, uint64_t m, uint64_t flat_bytes) {
    ok = n_rows < (1ull << 32) && m < (1ull << 32) && flat_bytes <= (1ull << 48);
    claim = 0;
    taken = round64(8ull * parts_route::kClaimWords);
    slot_row = taken + round64(n_rows);
    slot_stream = slot_row + round64(4 * m);
    slot_t = slot_stream + round64(4 * m);
    msg_off = slot_t + round64(4 * m);
    msg_len = msg_off + round64(8 * m);
    blocks = msg_len + round64(8 * m);
    flat = round256(blocks + round64(8 * m));
    bytes = flat + flat_bytes;
  }
};

}  // namespace schain
}  // namespace msha
