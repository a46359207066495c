// One row's work in the device stream sets (msha_dstreams_*, stream_device.hip): a
// stream whose chaining state, 64-byte buffer and byte count all live in device memory
// appends a list of parts gathered from an arena at any byte offset.
//
// hash.Hash.Write (pkg/processor/serial.go:21-23; recorder.go:348,
// ActiveHash.Write(digest)) keeps the bytes that do not fill a block until the next
// Write. Here those t = length % 64 buffered bytes are a stream's tail row, and a write
// treats them as a virtual first part in front of the row's real ones: the cursor of
// parts_gather.hpp starts with that part already open, at the tagged offset kTailTag,
// and the load callback reads a tagged offset from the tail row instead of the arena.
// parts::fill_block itself is used unchanged. kTailTag is bit 63, a multiple of 16, so
// the granule arithmetic of fill_block holds; real part offsets are below 2^63.
//
// Everything but compress() is in this header, which compiles for the host as well
// (tests/cpp/stream_device_check.cpp runs it under AddressSanitizer against a
// memcpy-and-hash restatement): the tagged load dispatch, the cursor's start, the block
// loop of one row's write and the tail / length update.
#pragma once
#include <stdint.h>

#include "parts_gather.hpp"

namespace msha {
namespace dstream {

constexpr uint64_t kTailTag = 1ull << 63;
constexpr uint32_t kRowDwords = 26;  // a packed row (export / import): 8 state words, 16 tail dwords, length lo, hi

MSHA_HD bool tagged(uint64_t off) { return (off & kTailTag) != 0; }
// The byte offset in the 64-byte tail row of the granule a tagged offset names: 0, 16,
// 32 or 48 whatever the other bits hold, so a tagged load never leaves the row.
MSHA_HD uint32_t tail_granule(uint64_t off) { return (uint32_t)off & 48u; }

// The tagged load dispatch, as the address the one 16-byte load reads: a granule of the
// stream's own tail row for a tagged offset, of the arena otherwise. (An address, not
// two loads to choose from: a lane's step has one load and no branch around it.)
MSHA_HD const uint8_t* tagged_address(uint64_t off, const uint8_t* arena, const uint8_t* tail_row) {
  return tagged(off) ? tail_row + tail_granule(off) : arena + off;
}

// Is [j0, jend) a part range a row may have? (It must not decrease, and holds fewer
// than 2^32 parts.)
MSHA_HD bool range_ok(uint64_t j0, uint64_t jend) { return jend >= j0 && jend - j0 <= 0xffffffffull; }

// The cursor of a write: the t buffered bytes open as the first part, the n_parts real
// parts from j0 behind them.
MSHA_HD void cursor_init(parts::Cursor& c, uint32_t t, uint64_t j0, uint32_t n_parts, const uint64_t* part_off,
                         const uint64_t* part_len) {
  parts::cursor_init(c, j0, n_parts, part_off, part_len);
  c.cur = kTailTag;
  c.rem = t;
}

// Dword j of a tail row holding r bytes, from the slot fill_block left (dwords at or
// past r's are stale or partial there): bytes past r are zero.
MSHA_HD uint32_t tail_dword(uint32_t slot_dword, uint32_t j, uint32_t r) {
  const int k = (int)r - 4 * (int)j;  // valid bytes in dword j
  if (k >= 4) return slot_dword;
  if (k <= 0) return 0u;
  return parts::low_bytes(slot_dword, (uint32_t)k);
}

struct Written {
  uint32_t tail = 0;      // bytes the stream buffers now (in the slot, see tail_dword)
  uint32_t blocks = 0;    // whole blocks handed to block()
  uint64_t appended = 0;  // bytes of the real parts
};

// One row's write: t bytes are buffered (read through load at tagged offsets, all of
// them inside the first fill_block); every whole block assembled in the slot is handed
// to block() (which reads the slot and compresses it); what is left below 64 bytes,
// possibly nothing, stays in the slot as the new tail.
template <class SlotWrite, class Load, class Block>
MSHA_HD Written write_row(uint32_t t, uint64_t j0, uint32_t n_parts, const uint64_t* part_off,
                          const uint64_t* part_len, SlotWrite&& slot, Load&& load, Block&& block) {
  parts::Cursor c;
  cursor_init(c, t, j0, n_parts, part_off, part_len);
  Written w;
  uint64_t gathered = 0;
  uint32_t r;
  while ((r = parts::fill_block(c, part_off, part_len, slot, load)) == 64) {
    block();
    ++w.blocks;
    gathered += 64;
  }
  w.tail = r;
  w.appended = gathered + r - t;
  return w;
}

}  // namespace dstream
}  // namespace msha
